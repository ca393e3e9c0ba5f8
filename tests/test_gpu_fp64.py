"""FP64 MFMA GEMM on a real MI355X; data convention in docs/KERNELS.md,
"FP64 leg". The host reference is a float64 matmul on the CPU. On
integer-valued data every sum is exact, so those comparisons are
equalities."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X")]

BK = 16  # the kernel's K-tile, in doubles
SENTINEL = -6.02e23  # an element the kernel never wrote shows
LIM = 2**20 - 1


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a
    assert a.probe_available()
    return a


def run(fn, a, bt):
    """fn on device copies of the CPU operands; C comes back to the CPU."""
    (m, k), n = a.shape, bt.shape[0]
    da, dbt = a.cuda(), bt.cuda()
    c = torch.full((m, n), SENTINEL, device="cuda", dtype=torch.float64)
    fn(0, da.data_ptr(), dbt.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    return c.cpu()


@pytest.fixture(scope="module")
def case_2x3():
    # 2x3 blocks, 3 K-tiles, integers uniform in +-(2^20 - 1)
    g = torch.Generator().manual_seed(3)
    a = torch.randint(-LIM, LIM + 1, (256, 3 * BK), generator=g).double()
    bt = torch.randint(-LIM, LIM + 1, (384, 3 * BK), generator=g).double()
    ref = a @ bt.t()
    assert a.abs().max() > 2**19 and bt.abs().max() > 2**19
    assert ((ref.abs() > 2**24) & (ref % 2 == 1)).any()  # beyond fp32
    return a, bt, ref


@pytest.mark.parametrize("fn", ["mfma_gemm_f64", "ref_gemm_f64"])
def test_random_exact(attest, case_2x3, fn):
    a, bt, ref = case_2x3
    c = run(getattr(attest, fn), a, bt)
    assert torch.equal(c, ref), f"{(c != ref).sum()} elements differ"


@pytest.mark.parametrize("side", ["A", "B"])
def test_identity_returns_the_operand(attest, side):
    """row * 128 + k + 1 on the swept side (256 rows, K = 128, every element
    distinct), the identity on the other: C is the swept operand,
    transposed for side B. Pins the operand row and k maps and the C/D map."""
    swept = (torch.arange(256)[:, None] * 128 + torch.arange(128)[None, :]
             + 1).double()
    eye = torch.eye(128, dtype=torch.float64)
    a, bt = (swept, eye) if side == "A" else (eye, swept)
    want = swept if side == "A" else swept.t()
    c = run(attest.mfma_gemm_f64, a, bt)
    assert torch.equal(c, want), f"{(c != want).sum()} elements differ"


def test_row_exponents_commute(attest, case_2x3):
    """Row m of A times 2^e_m, row n of Bt times 2^f_n, e and f in
    -400..400: scaling by a power of two commutes with every rounding and
    |e + f| + 53 < 1023, so C is ldexp(ref, e_m + f_n) exactly. Drives the
    11-bit exponent path."""
    a, bt, ref = case_2x3
    rng = np.random.default_rng(5)
    e = rng.integers(-400, 401, (a.shape[0], 1))
    f = rng.integers(-400, 401, (bt.shape[0], 1))
    want = torch.from_numpy(np.ldexp(ref.numpy(), e + f.T))
    c = run(attest.mfma_gemm_f64, torch.from_numpy(np.ldexp(a.numpy(), e)),
            torch.from_numpy(np.ldexp(bt.numpy(), f)))
    assert torch.equal(c, want), f"{(c != want).sum()} elements differ"


def test_random_normal_within_bound(attest):
    """Standard-normal doubles, 128x128x256. Each of the two computations
    is within gamma_K * (|A| |Bt|^T) of the true sum, gamma_K = K u /
    (1 - K u), u = 2^-53: the bound is twice that, derived, not measured."""
    g = torch.Generator().manual_seed(9)
    k = 256
    a = torch.randn(128, k, generator=g, dtype=torch.float64)
    bt = torch.randn(128, k, generator=g, dtype=torch.float64)
    ku = k * 2.0**-53
    bound = 2 * ku / (1 - ku) * (a.abs() @ bt.abs().t())
    err = (run(attest.mfma_gemm_f64, a, bt) - a @ bt.t()).abs()
    print(f"largest |C - ref| / bound: {(err / bound).max():.4f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("m,k,skew,leg_dim", [
    (64, BK, 0, None), (128, 24, 0, None), (128, BK, 8, None),
    (128, BK, 0, 8320)], ids=["m64", "k24", "misaligned", "leg8320"])
def test_refusal(attest, m, k, skew, leg_dim):
    a = torch.ones(129, 2 * BK, device="cuda", dtype=torch.float64)
    bt = torch.ones(128, 2 * BK, device="cuda", dtype=torch.float64)
    c = torch.full((128, 128), SENTINEL, device="cuda", dtype=torch.float64)
    with pytest.raises(attest.AttestationError, match=r"rc=-2\b"):
        if leg_dim:
            attest.attest_fp64(0, gemm_dim=leg_dim)
        else:
            attest.mfma_gemm_f64(0, a.data_ptr() + skew, bt.data_ptr(),
                                 c.data_ptr(), m, 128, k)
    torch.cuda.synchronize()
    assert (c == SENTINEL).all()  # nothing was launched


def test_attest_fp64(attest):
    first = attest.attest_fp64(0, gemm_dim=256)
    assert first.ok and first.mx_dim == 256 and first.mx_tflops > 0
    assert first.mx_max_abs_err == 0.0
    again = attest.attest_fp64(0, gemm_dim=256)
    assert again.ok and again.mx_ref_ms == 0.0  # cached reference
    assert again.mx_checksum == first.mx_checksum
