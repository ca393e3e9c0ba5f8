"""INT8 GEMM on a real MI355X, both integer MFMA shapes (0 = 32x32x32,
1 = 16x16x64); data convention in docs/KERNELS.md, "INT8 leg". Every
comparison is bitwise on int32: the host reference is a float64 matmul,
exact because every sum is far below 2^53."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X")]

BK = 128  # the kernel's K-tile
SHAPES = pytest.mark.parametrize("shape", [0, 1], ids=["32x32x32", "16x16x64"])
SENTINEL = -1515870811  # 0xA5A5A5A5: an element the kernel never wrote shows


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a
    assert a.probe_available()
    return a


def host_ref(a, bt):
    return (a.double() @ bt.double().t()).to(torch.int32)


def run(fn, a, bt, *extra):
    (m, k), n = a.shape, bt.shape[0]
    c = torch.full((m, n), SENTINEL, device="cuda", dtype=torch.int32)
    fn(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, *extra)
    torch.cuda.synchronize()
    return c


def draw(rows, k, lo, hi, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi + 1, (rows, k), device="cuda", generator=g,
                         dtype=torch.int8)


@pytest.fixture(scope="module")
def case_2x3():
    # 2x3 blocks, 3 K-tiles, uniform over the full range -128..127
    a, bt = draw(256, 3 * BK, -128, 127, 3), draw(384, 3 * BK, -128, 127, 4)
    assert a.min() == -128 and bt.min() == -128
    return a, bt, host_ref(a, bt)


@SHAPES
def test_random_full_range(attest, case_2x3, shape):
    a, bt, ref = case_2x3
    c = run(attest.mfma_gemm_i8, a, bt, shape)
    assert torch.equal(c, ref), f"{(c != ref).sum()} elements differ"


def test_valu_reference_matches_host_reference(attest, case_2x3):
    a, bt, ref = case_2x3
    c = run(attest.ref_gemm_i8_i32, a, bt)
    assert torch.equal(c, ref), f"{(c != ref).sum()} elements differ"


@SHAPES
@pytest.mark.parametrize("side", ["A", "B"])
def test_identity_returns_the_operand(attest, shape, side):
    """((row + k) mod 256) - 128 on the swept side (256 rows, K = 128: every
    code at every byte of every lane's registers), the identity on the
    other: C is the swept operand, transposed for side B."""
    r = torch.arange(256, device="cuda")[:, None]
    swept = ((r + torch.arange(BK, device="cuda")[None, :]) % 256 - 128).to(torch.int8)
    eye = torch.eye(BK, device="cuda", dtype=torch.int8)
    a, bt = (swept, eye) if side == "A" else (eye, swept)
    want = (swept if side == "A" else swept.t()).to(torch.int32)
    c = run(attest.mfma_gemm_i8, a, bt, shape)
    assert torch.equal(c, want), f"{(c != want).sum()} elements differ"


@SHAPES
def test_accumulator_is_a_32_bit_integer(attest, shape):
    """Operands in 101..127 over K = 2048: every sum is above 2048 * 10201 >
    2^24, which no fp32 accumulate reproduces bitwise."""
    a, bt = draw(128, 2048, 101, 127, 5), draw(128, 2048, 101, 127, 6)
    ref = host_ref(a, bt)
    assert ref.min() > 2**24 and (ref % 2 == 1).any()
    c = run(attest.mfma_gemm_i8, a, bt, shape)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


@pytest.mark.parametrize("m,k,shape,skew", [
    (64, BK, 0, 0), (128, 192, 1, 0), (128, 131072, 0, 0), (128, BK, 2, 0),
    (128, BK, 1, 1)], ids=["m64", "k192", "k131072", "shape2", "misaligned"])
def test_refusal(attest, m, k, shape, skew):
    a, bt = draw(129, 2 * BK, -128, 127, 1), draw(128, 2 * BK, -128, 127, 2)
    c = torch.full((128, 128), SENTINEL, device="cuda", dtype=torch.int32)
    with pytest.raises(attest.AttestationError, match=r"rc=-2$"):
        attest.mfma_gemm_i8(0, a.data_ptr() + skew, bt.data_ptr(), c.data_ptr(),
                            m, 128, k, shape)
    torch.cuda.synchronize()
    assert (c == SENTINEL).all()  # nothing was launched


@SHAPES
def test_attest_int8(attest, shape):
    first = attest.attest_int8(0, gemm_dim=256, shape=shape)
    assert first.ok and first.mx_dim == 256 and first.mx_tflops > 0
    assert first.mx_max_abs_err == 0.0
    again = attest.attest_int8(0, gemm_dim=256, shape=shape)
    assert again.ok and again.mx_ref_ms == 0.0  # cached reference
    assert again.mx_checksum == first.mx_checksum
