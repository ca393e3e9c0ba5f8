"""2:4 sparse bf16 GEMM on a real MI355X, both SMFMAC shapes (0 =
32x32x32, 1 = 16x16x64); data convention in docs/KERNELS.md, "Sparse
leg". The host reference is a float64 matmul of sp24_dense(ac, am) with
bt; on the exact value set it is cast to fp32 and compared bitwise."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X")]

SHAPES = pytest.mark.parametrize("shape", [0, 1], ids=["32x32x32", "16x16x64"])
SENTINEL = -6.02e23  # an element the kernel never wrote shows
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a
    assert a.probe_available()
    return a


def pack(attest, nib_idx):
    """Am bytes from legal-nibble numbers [M, K/4]: even group low."""
    nib = torch.tensor(attest.SP24_NIBBLES)[nib_idx]
    return (nib[:, 0::2] | nib[:, 1::2] << 4).to(torch.uint8)


def host_ref(attest, ac, am, bt):
    return attest.sp24_dense(ac, am).double() @ bt.double().t()


def run(fn, ac, am, bt, *extra):
    """fn on device copies of the CPU operands; C comes back to the CPU."""
    m, k, n = ac.shape[0], 2 * ac.shape[1], bt.shape[0]
    dac, dam, dbt = ac.cuda(), am.cuda(), bt.cuda()
    c = torch.full((m, n), SENTINEL, device="cuda")
    fn(0, dac.data_ptr(), dam.data_ptr(), dbt.data_ptr(), c.data_ptr(), m, n, k,
       *extra)
    torch.cuda.synchronize()
    return c.cpu()


def assert_bitwise(c, want):
    diff = c.view(torch.int32) != want.contiguous().view(torch.int32)
    assert not diff.any(), f"{diff.sum()} elements differ"


def draw_exact(g, rows, cols):
    """{0, 0.5, 1, 1.5, 2, 3} with both signs, -0 included."""
    mags = torch.tensor([0, 0.5, 1, 1.5, 2, 3])
    v = mags[torch.randint(0, 6, (rows, cols), generator=g)]
    return (v * (1.0 - 2.0 * torch.randint(0, 2, (rows, cols), generator=g))).to(BF16)


@pytest.fixture(scope="module")
def case_2x3(attest):
    # 2x3 blocks, 3 K-tiles
    g = torch.Generator().manual_seed(3)
    m, n, k = 256, 384, 384
    ac, bt = draw_exact(g, m, k // 2), draw_exact(g, n, k)
    nib_idx = torch.randint(0, 6, (m, k // 4), generator=g)
    assert nib_idx.unique().numel() == 6  # all six legal nibbles
    assert (ac.view(torch.int16) == -32768).any()  # -0
    am = pack(attest, nib_idx)
    return ac, am, bt, host_ref(attest, ac, am, bt).float()


@SHAPES
def test_random_exact(attest, case_2x3, shape):
    ac, am, bt, ref = case_2x3
    assert_bitwise(run(attest.mfma_gemm_sp24, ac, am, bt, shape), ref)


def test_valu_reference_matches_host_reference(attest, case_2x3):
    ac, am, bt, ref = case_2x3
    assert_bitwise(run(attest.ref_gemm_sp24_f32, ac, am, bt), ref)


@SHAPES
def test_identity_on_b_returns_decompressed_a(attest, shape):
    """Adjacent kept values differ and the nibble walks all six with row and
    group: pins the value order in a pair, the nibble and bit order, the
    index-half select and the A/B group correspondence."""
    m, j, grp = torch.arange(256)[:, None], torch.arange(64), torch.arange(32)
    ac = (1 + (m + j) % 127).to(BF16)
    am = pack(attest, (m + grp) % 6)
    c = run(attest.mfma_gemm_sp24, ac, am, torch.eye(128, dtype=BF16), shape)
    assert_bitwise(c, attest.sp24_dense(ac, am).float())


@SHAPES
def test_identity_on_a_returns_b(attest, shape):
    """The 128x128 identity, 2:4 compressed: row m keeps position m % 4 of
    group m // 4 (the one) and another position that varies with m (a
    zero); all other groups keep zeros under a walking nibble."""
    m, grp = torch.arange(128), torch.arange(32)
    p = m % 4
    q = (p + 1 + (m // 4) % 3) % 4
    nib = torch.tensor(attest.SP24_NIBBLES)[(m[:, None] + grp) % 6]
    nib[m, m // 4] = torch.minimum(p, q) | torch.maximum(p, q) << 2
    am = (nib[:, 0::2] | nib[:, 1::2] << 4).to(torch.uint8)
    ac = torch.zeros(128, 64, dtype=BF16)
    ac[m, 2 * (m // 4) + (p > q).long()] = 1
    assert torch.equal(attest.sp24_dense(ac, am), torch.eye(128, dtype=BF16))
    n, k = torch.arange(256)[:, None], torch.arange(128)
    bt = (1 + (n + k) % 127).to(BF16)
    assert_bitwise(run(attest.mfma_gemm_sp24, ac, am, bt, shape), bt.t().float())


@pytest.mark.parametrize("m,k,shape,skew", [
    (64, 128, 0, 0), (128, 192, 1, 0), (128, 128, 2, 0), (128, 128, 1, 1)],
    ids=["m64", "k192", "shape2", "misaligned"])
def test_refusal(attest, m, k, shape, skew):
    ac = torch.ones(128, 128, device="cuda", dtype=BF16)
    am = torch.full((129, 32), 0x44, device="cuda", dtype=torch.uint8)
    bt = torch.ones(128, 256, device="cuda", dtype=BF16)
    c = torch.full((128, 128), SENTINEL, device="cuda")
    with pytest.raises(attest.AttestationError, match=r"rc=-2$"):
        attest.mfma_gemm_sp24(0, ac.data_ptr(), am.data_ptr() + skew,
                              bt.data_ptr(), c.data_ptr(), m, 128, k, shape)
    torch.cuda.synchronize()
    assert (c == SENTINEL).all()  # nothing was launched


@SHAPES
def test_attest_sparse(attest, shape):
    first = attest.attest_sparse(0, gemm_dim=256, shape=shape)
    assert first.ok and first.mx_dim == 256 and first.mx_tflops > 0
    assert first.mx_max_abs_err == 0.0
    again = attest.attest_sparse(0, gemm_dim=256, shape=shape)
    assert again.ok and again.mx_ref_ms == 0.0  # cached reference
    assert again.mx_checksum == first.mx_checksum


@SHAPES
def test_random_normal_within_bound(attest, shape):
    """Standard normals rounded to bf16, 128x256x512. Products of two bf16
    are exact in fp32; a sum of K/2 terms in any order is within
    gamma_(K/2) * (|A_dense| |Bt|^T) of the true sum, and (K/2) * 2^-23
    is above gamma_(K/2) = (K/2) u / (1 - (K/2) u), u = 2^-24: derived, not
    measured."""
    g = torch.Generator().manual_seed(9)
    m, n, k = 128, 256, 512
    ac = torch.randn(m, k // 2, generator=g).to(BF16)
    bt = torch.randn(n, k, generator=g).to(BF16)
    am = pack(attest, torch.randint(0, 6, (m, k // 4), generator=g))
    bound = (k // 2) * 2.0**-23 * (
        attest.sp24_dense(ac, am).double().abs() @ bt.double().abs().t())
    c = run(attest.mfma_gemm_sp24, ac, am, bt, shape)
    err = (c.double() - host_ref(attest, ac, am, bt)).abs()
    print(f"largest |C - ref| / bound: {(err / bound).max():.4f}")
    assert (err <= bound).all()
