"""fp8 (MX-scaled e4m3, unit scales) GEMM on a real MI355X."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X"),
]


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a

    assert a.probe_available()
    return a


def _fp8(t):
    return t.to(torch.float8_e4m3fn)


def test_fp8_gemm_integer_exact(attest):
    """Small integers are exact in e4m3; fp32 accumulation on both
    sides -> bitwise agreement with the torch fp32 reference."""
    m = n = 256
    k = 512
    torch.manual_seed(7)
    a = _fp8(torch.randint(-2, 2, (m, k), device="cuda").float())
    bt = _fp8(torch.randint(-2, 2, (n, k), device="cuda").float())
    ref = a.float() @ bt.float().t()
    for trial in range(5):
        c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
        attest.mfma_gemm_fp8(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
        torch.cuda.synchronize()
        assert torch.equal(c, ref), f"trial {trial}: max diff {(c-ref).abs().max()}"


def test_fp8_deep_kernel_race_screen(attest):
    """Production dispatch at a 16-block grid (<= 1 block/CU, K%128)
    reaches the producer/consumer kernel mfma_gemm_fp8_128pc: bitwise
    integer race screen of its LDS-flag handoff across repeated runs.
    (The forced variants are screened in test_fp8_variants_bitwise.)"""
    m = n = 512
    k = 768  # nk = 6: both buffers wrap three times
    a = _fp8(torch.randint(-2, 2, (m, k), device="cuda").float())
    bt = _fp8(torch.randint(-2, 2, (n, k), device="cuda").float())
    ref = a.float() @ bt.float().t()
    for trial in range(10):
        c = torch.empty(m, n, device="cuda", dtype=torch.float32)
        attest.mfma_gemm_fp8(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
        torch.cuda.synchronize()
        assert torch.equal(c, ref), f"trial {trial}"


def _variant_bitwise_screen(attest, which, m, n, k):
    torch.manual_seed(which)
    a = _fp8(torch.randint(-2, 2, (m, k), device="cuda").float())
    bt = _fp8(torch.randint(-2, 2, (n, k), device="cuda").float())
    ref = a.float() @ bt.float().t()
    for trial in range(5):
        c = torch.empty(m, n, device="cuda", dtype=torch.float32)
        attest.mfma_gemm_fp8_variant(
            0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, which
        )
        torch.cuda.synchronize()
        assert torch.equal(c, ref), f"which={which} trial={trial}"


FORCED = [3, 5, 7, 8, 9, 10, 11, 12, 13]


@pytest.mark.parametrize("which", FORCED)
def test_fp8_variants_bitwise(attest, which):
    """Every forced fp8 variant (kFp8Forced in gemm_dispatch.hip: 3, 5
    and 7 the kernels production launches, 8-12 the option arms of the
    p/c and 4-blk kernels, 13 the 256-tile 1-blk kernel) must agree
    bitwise with the fp32 reference on integer data."""
    _variant_bitwise_screen(attest, which, 512, 512, 1024)


@pytest.mark.parametrize("which", FORCED)
def test_fp8_variants_bitwise_nonsquare(attest, which):
    """The same screen at m=256, n=512, k=512: 2x4 blocks for the
    128-tile kernels and 1x2 for the 256-tile ones, so a swapped M/N in
    the shared epilogue or block mapping shows as a mismatch."""
    _variant_bitwise_screen(attest, which, 256, 512, 512)


@pytest.mark.parametrize(
    "which,m,n,k",
    [(3, 128, 256, 64), (5, 128, 256, 128), (7, 128, 256, 128), (13, 256, 512, 128)],
)
def test_fp8_variants_single_k_tile(attest, which, m, n, k):
    """nk = 1 for the kernels production can launch and the 256-tile
    one: the K loops run only their prologue or first buffer (no
    prefetch, no buffer wrap, no cons_done wait). Grids are 1x2 blocks,
    so the M/N mapping is still exercised."""
    _variant_bitwise_screen(attest, which, m, n, k)


def test_fp8_past_one_block_per_cu_reaches_128u(attest):
    """17 x 16 = 272 blocks (> 256) with K%128 == 0 takes production
    dispatch to mfma_gemm_fp8_128u; the ~19 MiB working set keeps the XCD
    remap off, as at 8192^3 short of the cache rule. nk = 2. Bitwise
    against the torch fp32 reference on integer data."""
    m, n, k = 2176, 2048, 256
    torch.manual_seed(2176)
    a = _fp8(torch.randint(-2, 2, (m, k), device="cuda").float())
    bt = _fp8(torch.randint(-2, 2, (n, k), device="cuda").float())
    ref = a.float() @ bt.float().t()
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
    attest.mfma_gemm_fp8(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    assert torch.equal(c, ref)


def test_fp8_single_block_odd_nk_reaches_pc_kernel(attest):
    """A one-block grid with K%128 == 0 (nk = 3, odd) also goes to the
    producer/consumer kernel, not to the BK=64 fall-back."""
    m, n, k = 128, 128, 384
    a = _fp8(torch.randint(-2, 2, (m, k), device="cuda").float())
    bt = _fp8(torch.randint(-2, 2, (n, k), device="cuda").float())
    ref = a.float() @ bt.float().t()
    c = torch.empty(m, n, device="cuda", dtype=torch.float32)
    attest.mfma_gemm_fp8(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    assert torch.equal(c, ref)


def test_fp8_k64_only_reaches_bk64_kernel(attest):
    """K a multiple of 64 but not of 128 (k = 192: one block, nk = 3):
    production dispatch falls back to mfma_gemm_fp8_128s. Bitwise
    against the torch fp32 reference on integer data."""
    m, n, k = 128, 128, 192
    torch.manual_seed(192)
    a = _fp8(torch.randint(-2, 2, (m, k), device="cuda").float())
    bt = _fp8(torch.randint(-2, 2, (n, k), device="cuda").float())
    ref = a.float() @ bt.float().t()
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
    attest.mfma_gemm_fp8(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    assert torch.equal(c, ref)


@pytest.mark.parametrize("which", [0, 2, 4, 6, 14, 15, -1])
def test_fp8_retired_variant_refused(attest, which):
    """A number that names no kernel (0, 2, 4, 6 and 14 did once, before
    those kernels were removed) is refused with rc=-2 and nothing is
    launched: c stays as it was."""
    m, n, k = 256, 256, 256
    a = _fp8(torch.ones(m, k, device="cuda"))
    bt = _fp8(torch.ones(n, k, device="cuda"))
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
    with pytest.raises(attest.AttestationError, match="rc=-2"):
        attest.mfma_gemm_fp8_variant(
            0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, which
        )
    torch.cuda.synchronize()
    assert torch.isnan(c).all()


@pytest.mark.parametrize("m,n,k", [(256, 512, 256), (512, 256, 1024)])
def test_fp8_gemm_random_matches_reference(attest, m, n, k):
    torch.manual_seed(m + n + k)
    a = _fp8(torch.randn(m, k, device="cuda"))
    bt = _fp8(torch.randn(n, k, device="cuda"))
    ref = a.float() @ bt.float().t()
    c = torch.empty(m, n, device="cuda", dtype=torch.float32)
    attest.mfma_gemm_fp8(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    err = (c - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 1e-3 * max(scale, 1.0), f"err={err} scale={scale}"
