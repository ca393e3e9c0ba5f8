"""MXFP8 GEMM on a real MI355X, the four format pairs (0 = e4m3, 1 = e5m2
per operand); data convention in docs/KERNELS.md, "MXFP8 leg"."""

import math

import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X")]

BK = 128  # the kernel's K-tile
NAMES = ["e4m3", "e5m2"]
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]
IDS = [f"{NAMES[a]}-{NAMES[b]}" for a, b in PAIRS]
FMTS = pytest.mark.parametrize("fa,fb", PAIRS, ids=IDS)
MIXED = pytest.mark.parametrize("fa,fb", PAIRS[1:3], ids=IDS[1:3])
# the magnitudes both formats hold and the gate's fill uses
EXACT = [s * v for s in (1.0, -1.0) for v in (0.0, 0.5, 1.0, 1.5, 2.0, 3.0)]


def table(fmt):
    """The 256 values from the field definition: e4m3 (bias 7, NaN at
    S.1111.111) or e5m2 (bias 15, Inf and NaN at exponent 31)."""
    mb, bias = (3, 7) if fmt == 0 else (2, 15)
    out = []
    for code in range(256):
        e, m = (code >> mb) & (127 >> mb), code & ((1 << mb) - 1)
        v = (1 + m / 2**mb) * 2.0 ** (e - bias) if e else m / 2**mb * 2.0 ** (1 - bias)
        if (fmt == 0 and e == 15 and m == 7) or (fmt == 1 and e == 31):
            v = math.nan if fmt == 0 or m else math.inf
        out.append(-v if code & 128 else v)
    return out


def codes_of(fmt, values):  # the sign bit keeps -0.0 apart from 0.0
    t = table(fmt)
    return torch.tensor([t.index(abs(v)) | (128 if str(v)[0] == "-" else 0)
                         for v in values], device="cuda", dtype=torch.uint8)


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a
    assert a.probe_available()
    return a


def dequant(fmt, codes, scales, absolute=False):  # float64 [rows, K]
    vals = torch.tensor(table(fmt), dtype=torch.float64, device="cuda")[codes.long()]
    vals = vals * (2.0 ** (scales.double() - 127.0)).repeat_interleave(32, dim=1)
    return vals.abs() if absolute else vals


def host_ref64(fa, fb, a, sa, bt, sb):
    return dequant(fa, a, sa) @ dequant(fb, bt, sb).t()


def run(fn, fa, fb, a, sa, bt, sb, m, n, k):
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
    fn(0, a.data_ptr(), sa.data_ptr(), bt.data_ptr(), sb.data_ptr(),
       c.data_ptr(), m, n, k, fa, fb)
    torch.cuda.synchronize()
    return c


def unit_scales(rows, k):
    return torch.full((rows, k // 32), 127, device="cuda", dtype=torch.uint8)


def random_case(fa, fb, m, n, k, seed, lo=126, hi=128, all_codes=False):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def draw(fmt, rows):
        pool = codes_of(fmt, EXACT)
        if all_codes:  # every finite code, ascending
            pool = torch.tensor([c for c, v in enumerate(table(fmt))
                                 if math.isfinite(v)], device="cuda", dtype=torch.uint8)
        return pool[torch.randint(0, len(pool), (rows, k), device="cuda",
                                  generator=g)].contiguous()

    def scales(rows):
        return torch.randint(lo, hi + 1, (rows, k // 32), device="cuda",
                             generator=g, dtype=torch.uint8)

    a, bt = draw(fa, m), draw(fb, n)
    return a, scales(m), bt, scales(n)


@pytest.fixture(scope="module", params=PAIRS, ids=IDS)
def case_3x2(request):
    # 3x2 blocks, 3 K-tiles of random exact data and the host reference
    (fa, fb), (m, n, k) = request.param, (256, 384, 3 * BK)
    ops = random_case(fa, fb, m, n, k, seed=3)
    return fa, fb, (m, n, k), ops, host_ref64(fa, fb, *ops).float()


@pytest.mark.parametrize("fmt", [0, 1], ids=NAMES)
@pytest.mark.parametrize("side", ["A", "B"])
def test_decode_all_codes(attest, fmt, side):
    """Code (row + k) mod 256 (non-finite ones 0x00) on the swept side, the
    identity on the other: C is the decoded operand."""
    r = torch.arange(256, device="cuda")[:, None]
    swept = ((r + torch.arange(BK, device="cuda")[None, :]) % 256).to(torch.uint8)
    finite = torch.isfinite(torch.tensor(table(fmt), device="cuda"))
    swept = torch.where(finite[swept.long()], swept, torch.zeros_like(swept))
    eye = (torch.eye(BK, device="cuda") * codes_of(fmt, [1.0])).to(torch.uint8)
    a, bt = (swept, eye) if side == "A" else (eye, swept)
    m, n = a.shape[0], bt.shape[0]
    sa, sb = unit_scales(m, BK), unit_scales(n, BK)
    ref = host_ref64(fmt, fmt, a, sa, bt, sb).float()
    c = run(attest.mfma_gemm_mxfp8, fmt, fmt, a, sa, bt, sb, m, n, BK)
    assert torch.equal(c, ref), f"{(c != ref).sum()} elements differ"


@FMTS
@pytest.mark.parametrize("patterned", ["A", "B"])
def test_scale_map_structured(attest, fa, fb, patterned):
    """All values 1.0, one operand's scales patterned by row and K block
    over two K-tiles."""
    m, n, k = 128, 128, 2 * BK
    a = codes_of(fa, [1.0]).expand(m, k).contiguous()
    bt = codes_of(fb, [1.0]).expand(n, k).contiguous()
    r = torch.arange(m, device="cuda")[:, None]
    kb = torch.arange(k // 32, device="cuda")[None, :]
    sa, sb = unit_scales(m, k), unit_scales(n, k)
    if patterned == "A":
        sa = (126 + (r + 2 * kb) % 3).to(torch.uint8)
    else:
        sb = (126 + (2 * r + kb) % 3).to(torch.uint8)
    ref = host_ref64(fa, fb, a, sa, bt, sb).float()
    c = run(attest.mfma_gemm_mxfp8, fa, fb, a, sa, bt, sb, m, n, k)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


def test_random_exact_race_screen(attest, case_3x2):
    """Five runs, bitwise (exact while K * 576 < 2^24): a k in the wrong
    scale block, i.e. a wrong operand image, changes the sums."""
    fa, fb, (m, n, k), ops, ref = case_3x2
    for trial in range(5):
        c = run(attest.mfma_gemm_mxfp8, fa, fb, *ops, m, n, k)
        assert torch.equal(c, ref), f"trial {trial}: {(c - ref).abs().max()}"


@MIXED
def test_random_exact_k2048(attest, fa, fb):  # one block, 16 K-tiles
    m, n, k = 128, 128, 2048
    ops = random_case(fa, fb, m, n, k, seed=11)
    c = run(attest.mfma_gemm_mxfp8, fa, fb, *ops, m, n, k)
    assert torch.equal(c, host_ref64(fa, fb, *ops).float())


def test_valu_reference_matches_host_reference(attest, case_3x2):
    fa, fb, (m, n, k), ops, ref = case_3x2
    c = run(attest.ref_gemm_mxfp8_f32, fa, fb, *ops, m, n, k)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


@FMTS
def test_wide_scales_within_accumulation_bound(attest, fa, fb):
    """All finite codes, scale bytes in [117,137]: |c - ref| <= c0 * K *
    2^-23 * (|A| |Bt|^T); c0 = 1 is one truncation per add."""
    # Measured, (A, B): e4m3-e4m3 4.12 of the bound, e4m3-e5m2 4.34,
    # e5m2-e4m3 3.50, e5m2-e5m2 3.00 (the e3m2 effect, docs/KERNELS.md);
    # c0 is the next power of two above, the margin covers data dependence.
    c0 = {(0, 0): 8.0, (0, 1): 8.0, (1, 0): 4.0, (1, 1): 4.0}[fa, fb]
    m, n, k = 128, 256, 512
    a, sa, bt, sb = random_case(fa, fb, m, n, k, 17, 117, 137, all_codes=True)
    ref = host_ref64(fa, fb, a, sa, bt, sb)
    bound = k * 2.0 ** -23 * (dequant(fa, a, sa, True) @ dequant(fb, bt, sb, True).t())
    c = run(attest.mfma_gemm_mxfp8, fa, fb, a, sa, bt, sb, m, n, k)
    assert not torch.isnan(c).any()
    ratio = ((c.double() - ref).abs() / bound).max().item()
    print(f"fmt ({fa}, {fb}): largest error / bound = {ratio:.3g}")
    assert ratio <= c0, f"error is {ratio} of the bound"


@pytest.mark.parametrize("m,n,k,fa,fb", [
    (128, 128, BK // 2, 0, 0), (128, 128, 3 * BK // 2, 1, 0),
    (64, 128, BK, 0, 1), (128, 128, BK, 2, 0), (128, 128, BK, 1, 2)])
def test_refusal(attest, m, n, k, fa, fb):
    a, sa, bt, sb = random_case(0, 0, 128, 128, 2 * BK, seed=1)
    c = torch.zeros(128, 128, device="cuda", dtype=torch.float32)
    with pytest.raises(attest.AttestationError, match=r"rc=-2$"):
        attest.mfma_gemm_mxfp8(0, a.data_ptr(), sa.data_ptr(), bt.data_ptr(),
                               sb.data_ptr(), c.data_ptr(), m, n, k, fa, fb)
    torch.cuda.synchronize()
    assert not c.any()  # nothing was launched


@FMTS
@pytest.mark.parametrize("dim", [256, 1024])
def test_attest_mxfp8(attest, dim, fa, fb):
    assert attest.attest_device(0, 256).ok
    first = attest.attest_mxfp8(0, dim, fa, fb)
    assert first.ok and first.mx_dim == dim and first.mx_tflops > 0
    assert first.mx_max_abs_err == 0.0
    again = attest.attest_mxfp8(0, dim, fa, fb)
    assert again.ok and again.mx_ref_ms == 0.0  # cached reference
    assert again.mx_checksum == first.mx_checksum
    other = attest.attest_mxfp8(0, dim, fa, 1 - fb)  # same dim, another pair
    assert other.ok and other.mx_ref_ms > 0.0  # recomputed
    assert attest.attest_device(0, 256).ok


def test_attestor_hook_runs_mxfp8_leg(attest, monkeypatch):
    """CC_ATTEST_MXFP8=1 through the real hook: exactly two more keys."""
    from k8s_cc_manager_amd.device.shadow import ShadowBackend
    devices, _ = ShadowBackend(device_indices=[0]).find_devices()
    monkeypatch.setenv("CC_ATTEST_GEMM_DIM", "512")
    for name in ("DEEP", "MXFP4", "MXFP6", "MXFP8"):
        monkeypatch.delenv("CC_ATTEST_" + name, raising=False)
    plain = attest.attest_device_by_bdf(devices[0])
    assert "mxfp8_tflops" not in plain and "mxfp8_bitwise_ok" not in plain
    monkeypatch.setenv("CC_ATTEST_MXFP8", "1")
    summary = attest.attest_device_by_bdf(devices[0])
    assert set(summary) == set(plain) | {"mxfp8_tflops", "mxfp8_bitwise_ok"}
    assert summary["mxfp8_bitwise_ok"] is True and summary["mxfp8_tflops"] > 0
