"""FP16 GEMM on a real MI355X, both f16 MFMA shapes (0 = 32x32x16,
1 = 16x16x32); data convention in docs/KERNELS.md, "FP16 leg". The host
reference is a float64 matmul, exact in every bitwise case: the sums there
fit fp32's 24 bits by construction."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X")]

BK = 64  # the kernel's K-tile, elements
SHAPES = pytest.mark.parametrize("shape", [0, 1], ids=["32x32x16", "16x16x32"])
SENTINEL = -1515870811  # 0xA5A5A5A5: an element the kernel never wrote shows


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a
    assert a.probe_available()
    return a


def host_ref(a, bt):
    return (a.double() @ bt.double().t()).float()


def run(fn, a, bt, *extra):
    (m, k), n = a.shape, bt.shape[0]
    c = torch.full((m, n), SENTINEL, device="cuda", dtype=torch.int32)
    fn(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, *extra)
    torch.cuda.synchronize()
    return c.view(torch.float32)


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def row_scaled(rows, k, step, seed):
    """(j/4) * 2^e(row): j uniform in -31..31, one element in 64 replaced by
    -0, e = (row * step) mod 36 - 22 (step coprime to 36: all of -22..13)."""
    g = gen(seed)
    j = torch.randint(-31, 32, (rows, k), device="cuda", generator=g)
    e = (torch.arange(rows, device="cuda") * step) % 36 - 22
    v = j.double() / 4 * torch.exp2(e.double())[:, None]
    v[torch.rand(rows, k, device="cuda", generator=g) < 1 / 64] = -0.0
    h = v.half()
    assert (h.double() == v).all() and (h.view(torch.int16) == -32768).any()
    return h


@pytest.fixture(scope="module")
def case_2x3():
    # 2x3 blocks, 3 K-tiles; |sum| <= 192 * 961 < 2^18 before the row factors
    a, bt = row_scaled(256, 3 * BK, 5, 3), row_scaled(384, 3 * BK, 7, 4)
    return a, bt, host_ref(a, bt)


@SHAPES
def test_random_exact_row_exponents(attest, case_2x3, shape):
    a, bt, ref = case_2x3
    c = run(attest.mfma_gemm_f16, a, bt, shape)
    assert torch.equal(c, ref), f"{(c != ref).sum()} elements differ"


def test_valu_reference_matches_host_reference(attest, case_2x3):
    a, bt, ref = case_2x3
    c = run(attest.ref_gemm_f16_f32, a, bt)
    assert torch.equal(c, ref), f"{(c != ref).sum()} elements differ"


@SHAPES
@pytest.mark.parametrize("side", ["A", "B"])
def test_decode_all_codes(attest, shape, side):
    """Code (r + 1024 k) mod 65536 at (r, k) of the swept side (exponent 31
    replaced by code 0): every finite code, subnormals included, at every k
    of a tile and every register position. The other side is the identity,
    so C is the swept operand in fp32, transposed for side B."""
    r = torch.arange(65536, device="cuda")[:, None]
    code = (r + 1024 * torch.arange(BK, device="cuda")[None, :]) % 65536
    code[(code >> 10) % 32 == 31] = 0
    swept = ((code + 32768) % 65536 - 32768).to(torch.int16).view(torch.float16)
    eye = torch.zeros(128, BK, device="cuda", dtype=torch.float16)
    eye[:BK] = torch.eye(BK, device="cuda", dtype=torch.float16)
    a, bt = (swept, eye) if side == "A" else (eye, swept)
    c = run(attest.mfma_gemm_f16, a, bt, shape)
    got = c if side == "A" else c.t()  # [65536, 128]
    want = swept.cpu().float().cuda()  # the host's conversion
    assert torch.equal(got[:, :BK], want), \
        f"{(got[:, :BK] != want).sum()} elements differ"
    assert (got[:, BK:] == 0).all()


@SHAPES
def test_full_width_products(attest, shape):
    """Integers of magnitude 1024..2047 (all 11 significand bits), four per
    row of A: a product has up to 22 bits and a sum stays below 2^24, so the
    products must arrive unrounded."""
    g = gen(5)

    def ints(rows, k):
        mag = torch.randint(1024, 2048, (rows, k), device="cuda", generator=g)
        sign = torch.randint(0, 2, (rows, k), device="cuda", generator=g) * 2 - 1
        return (mag * sign).half()

    keep = torch.rand(128, 3 * BK, device="cuda", generator=g).argsort(1)[:, :4]
    a = torch.zeros(128, 3 * BK, device="cuda", dtype=torch.float16)
    a.scatter_(1, keep, ints(128, 4))
    bt = ints(128, 3 * BK)
    ref = host_ref(a, bt)
    assert ref.abs().max() < 2**24
    assert ((ref.abs() > 2**22) & (ref % 2 == 1)).any()
    c = run(attest.mfma_gemm_f16, a, bt, shape)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


@SHAPES
def test_random_normal_within_bound(attest, shape):
    """Standard normal data: |C - ref64| <= K * 2^-23 * (|A| . |Bt|^T), one
    rounding per add (products of two binary16 are exact in fp32). Measured:
    the largest ratio to that bound is 0.0014 (32x32x16) and 0.0013
    (16x16x32)."""
    g = gen(6)
    a = torch.randn(128, 512, device="cuda", generator=g).half()
    bt = torch.randn(256, 512, device="cuda", generator=g).half()
    ref = a.double() @ bt.double().t()
    bound = 512 * 2.0**-23 * (a.double().abs() @ bt.double().abs().t())
    c = run(attest.mfma_gemm_f16, a, bt, shape)
    ratio = ((c.double() - ref).abs() / bound).max().item()
    print(f"fp16 shape {shape}: max |C - ref64| / bound = {ratio:.4g}")
    assert ratio <= 1.0


@pytest.mark.parametrize("m,k,shape,skew", [
    (64, BK, 0, 0), (128, 96, 1, 0), (128, BK, 2, 0), (128, BK, 1, 2)],
    ids=["m64", "k96", "shape2", "misaligned"])
def test_refusal(attest, m, k, shape, skew):
    a = torch.ones(129, 2 * BK, device="cuda", dtype=torch.float16)
    bt = torch.ones(128, 2 * BK, device="cuda", dtype=torch.float16)
    c = torch.full((128, 128), SENTINEL, device="cuda", dtype=torch.int32)
    with pytest.raises(attest.AttestationError, match=r"rc=-2$"):
        attest.mfma_gemm_f16(0, a.data_ptr() + skew, bt.data_ptr(),
                             c.data_ptr(), m, 128, k, shape)
    torch.cuda.synchronize()
    assert (c == SENTINEL).all()  # nothing was launched


def test_attest_refuses_inexact_dim(attest):
    with pytest.raises(attest.AttestationError, match=r"rc=-2: .*16384"):
        attest.attest_fp16(0, gemm_dim=16512)  # K * 961 would pass 2^24


@SHAPES
def test_attest_fp16(attest, shape):
    first = attest.attest_fp16(0, gemm_dim=256, shape=shape)
    assert first.ok and first.mx_dim == 256 and first.mx_tflops > 0
    assert first.mx_max_abs_err == 0.0
    again = attest.attest_fp16(0, gemm_dim=256, shape=shape)
    assert again.ok and again.mx_ref_ms == 0.0  # cached reference
    assert again.mx_checksum == first.mx_checksum
    other = attest.attest_fp16(0, gemm_dim=256, shape=1 - shape)
    assert other.ok and other.mx_ref_ms == 0.0  # both shapes share it
