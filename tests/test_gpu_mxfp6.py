"""MXFP6 GEMM (e2m3 or e3m2 values, E8M0 scale per 32 elements of K) on
a real MI355X: operand decode, scale lane map, exactness, the VALU
reference and the opt-in attestation leg, for both formats.

Data convention (docs/KERNELS.md, "MXFP6 leg"): A[M,K] and Bt[N,K] hold
3K/4 bytes per row, every 32-element block is 24 bytes read as one
little-endian number with element j in bits 6j..6j+5; SA[M,K/32],
SB[N,K/32] uint8, byte s = 2^(s-127)."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X"),
]

BK = 128  # the kernel's K-tile
FMTS = pytest.mark.parametrize("fmt", [2, 3], ids=["e2m3", "e3m2"])


def table(fmt):
    """The 64 values of a format from its field definition: sign, then
    e2m3 (2-bit exponent, bias 1) or e3m2 (3-bit exponent, bias 3),
    subnormals, no Inf or NaN."""
    mb, bias = (3, 1) if fmt == 2 else (2, 3)
    out = []
    for code in range(64):
        e, m = (code >> mb) & (31 >> mb), code & ((1 << mb) - 1)
        v = (1 + m / 2**mb) * 2.0 ** (e - bias) if e else m / 2**mb * 2.0 ** (1 - bias)
        out.append(-v if code & 32 else v)
    return out


def codes_of(fmt, values):
    """Codes of `values`; the sign bit keeps -0.0 apart from 0.0."""
    t = table(fmt)
    return torch.tensor([t.index(abs(v)) | (32 if str(v)[0] == "-" else 0)
                         for v in values], device="cuda")


# the magnitudes both formats hold and the gate's fill uses
EXACT = [s * v for s in (1.0, -1.0) for v in (0.0, 0.5, 1.0, 1.5, 2.0, 3.0)]


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a

    assert a.probe_available()
    return a


def pack(codes):
    """[rows, K] codes 0..63 -> [rows, 3K/4] bytes: four codes are 24 bits."""
    c = codes.to(torch.int32).reshape(codes.shape[0], -1, 4)
    word = c[..., 0] | c[..., 1] << 6 | c[..., 2] << 12 | c[..., 3] << 18
    b = torch.stack([word & 255, word >> 8 & 255, word >> 16], dim=2)
    return b.reshape(codes.shape[0], -1).to(torch.uint8).contiguous()


def dequant(fmt, packed, scales, absolute=False):
    """Host reference decode, plain torch ops, float64 [rows, K]."""
    b = packed.to(torch.int64).reshape(packed.shape[0], -1, 3)
    word = b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16
    codes = torch.stack([word >> s & 63 for s in (0, 6, 12, 18)], dim=2)
    vals = torch.tensor(table(fmt), dtype=torch.float64, device="cuda")[
        codes.reshape(packed.shape[0], -1)]
    vals = vals * (2.0 ** (scales.double() - 127.0)).repeat_interleave(32, dim=1)
    return vals.abs() if absolute else vals


def host_ref64(fmt, a, sa, bt, sb):
    return dequant(fmt, a, sa) @ dequant(fmt, bt, sb).t()


def run(fn, fmt, a, sa, bt, sb, m, n, k):
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
    fn(0, a.data_ptr(), sa.data_ptr(), bt.data_ptr(), sb.data_ptr(),
       c.data_ptr(), m, n, k, fmt)
    torch.cuda.synchronize()
    return c


def unit_scales(rows, k):
    return torch.full((rows, k // 32), 127, device="cuda", dtype=torch.uint8)


def random_case(fmt, m, n, k, seed, lo=126, hi=128, all_codes=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    pool = torch.arange(64, device="cuda") if all_codes else codes_of(fmt, EXACT)

    def draw(rows):
        return pack(pool[torch.randint(0, len(pool), (rows, k), device="cuda",
                                       generator=g)])

    def scales(rows):
        return torch.randint(lo, hi + 1, (rows, k // 32), device="cuda",
                             generator=g, dtype=torch.uint8)

    a, bt = draw(m), draw(n)
    return a, scales(m), bt, scales(n)


@pytest.fixture(scope="module", params=[2, 3], ids=["e2m3", "e3m2"])
def case_3x2(request):
    """256x384x384 random exact data (3x2 blocks, 3 K-tiles) and its host
    reference, shared by the race screen and the VALU reference check."""
    fmt, (m, n, k) = request.param, (256, 384, 3 * BK)
    ops = random_case(fmt, m, n, k, seed=3)
    return fmt, (m, n, k), ops, host_ref64(fmt, *ops).float()


@FMTS
@pytest.mark.parametrize("side", ["A", "B"])
def test_decode_all_codes(attest, fmt, side):
    """The side under test holds code (row + k) mod 64: every code at
    every position of a block. The other side holds +-0.5, +-1, +-2, so
    products are multiples of 2^-5 of at most 56 and the sums are exact."""
    m = n = 128
    r = torch.arange(m, device="cuda")[:, None]
    kk = torch.arange(BK, device="cuda")[None, :]
    swept = pack((r + kk) % 64)
    other = pack(codes_of(fmt, [0.5, -1.0, 2.0, -0.5, 1.0, -2.0])[
        (3 * r + 5 * kk + 1) % 6])
    a, bt = (swept, other) if side == "A" else (other, swept)
    sa, sb = unit_scales(m, BK), unit_scales(n, BK)
    ref = host_ref64(fmt, a, sa, bt, sb).float()
    c = run(attest.mfma_gemm_mxfp6, fmt, a, sa, bt, sb, m, n, BK)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


@FMTS
@pytest.mark.parametrize("patterned", ["A", "B"])
def test_scale_map_structured(attest, fmt, patterned):
    """All values 1.0, one operand's scales patterned by row and K block
    over two K-tiles, the other's at 2^0: a wrong lane-to-row map, byte
    select, tile step or A/B scale swap changes the sums."""
    m, n, k = 128, 128, 2 * BK
    ones = pack(codes_of(fmt, [1.0]).expand(m, k))
    r = torch.arange(m, device="cuda")[:, None]
    kb = torch.arange(k // 32, device="cuda")[None, :]
    sa, sb = unit_scales(m, k), unit_scales(n, k)
    if patterned == "A":
        sa = (126 + (r + 2 * kb) % 3).to(torch.uint8)
    else:
        sb = (126 + (2 * r + kb) % 3).to(torch.uint8)
    ref = host_ref64(fmt, ones, sa, ones, sb).float()
    c = run(attest.mfma_gemm_mxfp6, fmt, ones, sa, ones, sb, m, n, k)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


def test_random_exact_race_screen(attest, case_3x2):
    """Five runs, bitwise: pins which k belongs to which scale block."""
    fmt, (m, n, k), ops, ref = case_3x2
    for trial in range(5):
        c = run(attest.mfma_gemm_mxfp6, fmt, *ops, m, n, k)
        assert torch.equal(c, ref), f"trial {trial}: {(c - ref).abs().max()}"


@FMTS
def test_random_exact_k2048(attest, fmt):
    """One block, 16 K-tiles: terms are multiples of 2^-4 of at most 36,
    so every partial sum fits 24 bits in any order."""
    m, n, k = 128, 128, 2048
    ops = random_case(fmt, m, n, k, seed=11)
    ref = host_ref64(fmt, *ops).float()
    c = run(attest.mfma_gemm_mxfp6, fmt, *ops, m, n, k)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


def test_valu_reference_matches_host_reference(attest, case_3x2):
    fmt, (m, n, k), ops, ref = case_3x2
    c = run(attest.ref_gemm_mxfp6_f32, fmt, *ops, m, n, k)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


@FMTS
def test_wide_scales_within_accumulation_bound(attest, fmt):
    """All 64 codes, scale bytes in [117,137]: sums are no longer exact
    in fp32. With one truncation per add, |c - ref| <= c0 * K * 2^-23 *
    (|A| |Bt|^T) elementwise; c0 = 1 as for MXFP4 where the device meets
    it."""
    # e2m3 measured 0.0023 of the bound, e3m2 1.63: its products span
    # 2^-8 .. 784 inside one instruction, and the MFMA aligns the 64
    # products to the largest in a window narrower than fp32's 24 bits,
    # dropping low bits of the small ones that one truncation per add
    # keeps. c0 is the next power of two above the measured ratio.
    c0 = {2: 1.0, 3: 2.0}[fmt]
    m, n, k = 128, 256, 512
    a, sa, bt, sb = random_case(fmt, m, n, k, seed=17, lo=117, hi=137,
                                all_codes=True)
    ref = host_ref64(fmt, a, sa, bt, sb)
    bound = k * 2.0 ** -23 * (
        dequant(fmt, a, sa, True) @ dequant(fmt, bt, sb, True).t())
    c = run(attest.mfma_gemm_mxfp6, fmt, a, sa, bt, sb, m, n, k)
    assert not torch.isnan(c).any()
    ratio = ((c.double() - ref).abs() / bound).max().item()
    print(f"fmt {fmt}: largest error / bound = {ratio:.3g}")
    assert ratio <= c0, f"error is {ratio} of the bound"


@pytest.mark.parametrize("m,n,k,fmt", [(128, 128, BK // 2, 2), (128, 128, 3 * BK // 2, 3),
                                       (64, 128, BK, 2), (128, 128, BK, 4)])
def test_refusal(attest, m, n, k, fmt):
    a, sa, bt, sb = random_case(2, 128, 128, 2 * BK, seed=1)
    c = torch.zeros(128, 128, device="cuda", dtype=torch.float32)
    with pytest.raises(attest.AttestationError, match=r"rc=-2$"):
        attest.mfma_gemm_mxfp6(0, a.data_ptr(), sa.data_ptr(), bt.data_ptr(),
                               sb.data_ptr(), c.data_ptr(), m, n, k, fmt)
    torch.cuda.synchronize()
    assert not c.any()  # nothing was launched


@FMTS
@pytest.mark.parametrize("dim", [256, 1024])
def test_attest_mxfp6(attest, dim, fmt):
    assert attest.attest_device(0, 256).ok
    first = attest.attest_mxfp6(0, dim, fmt)
    assert first.ok and first.mx_dim == dim
    assert first.mx_max_abs_err == 0.0
    assert first.mx_tflops > 0
    again = attest.attest_mxfp6(0, dim, fmt)
    assert again.ok
    assert again.mx_ref_ms == 0.0  # cached reference
    assert again.mx_checksum == first.mx_checksum
    other = attest.attest_mxfp6(0, dim, 5 - fmt)  # same dim, the other format
    assert other.ok and other.mx_ref_ms > 0.0  # recomputed
    assert attest.attest_device(0, 256).ok


def test_attestor_hook_runs_mxfp6_leg(attest, monkeypatch):
    """CC_ATTEST_MXFP6=1 through the real attestor hook on device 0: the
    summary gains exactly the two MXFP6 keys, else none."""
    from k8s_cc_manager_amd.device.shadow import ShadowBackend
    devices, _ = ShadowBackend(device_indices=[0]).find_devices()
    monkeypatch.setenv("CC_ATTEST_GEMM_DIM", "512")
    for name in ("CC_ATTEST_DEEP", "CC_ATTEST_MXFP4", "CC_ATTEST_MXFP6"):
        monkeypatch.delenv(name, raising=False)
    plain = attest.attest_device_by_bdf(devices[0])
    assert "mxfp6_tflops" not in plain and "mxfp6_bitwise_ok" not in plain
    monkeypatch.setenv("CC_ATTEST_MXFP6", "1")
    summary = attest.attest_device_by_bdf(devices[0])
    assert set(summary) == set(plain) | {"mxfp6_tflops", "mxfp6_bitwise_ok"}
    assert summary["mxfp6_bitwise_ok"] is True
    assert summary["mxfp6_tflops"] > 0
