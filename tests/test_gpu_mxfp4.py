"""MXFP4 GEMM (e2m1 values, E8M0 scale per 32 elements of K) on a real
MI355X: operand decode, scale lane map, exactness, the VALU reference
and the opt-in attestation leg.

Data convention (docs/KERNELS.md, "MXFP4 leg"): A[M,K] and Bt[N,K]
packed two fp4 per byte, low nibble = even k; SA[M,K/32], SB[N,K/32]
uint8, byte s = 2^(s-127)."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X"),
]

# OCP e2m1: sign, 2-bit exponent, 1-bit mantissa
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
        -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a

    assert a.probe_available()
    return a


def pack(codes):
    """[rows, K] uint8 codes 0..15 -> [rows, K/2] packed bytes."""
    codes = codes.to(torch.uint8)
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def dequant(packed, scales, absolute=False):
    """Host reference decode, plain torch ops, float64 [rows, K]."""
    table = torch.tensor(E2M1, dtype=torch.float64, device=packed.device)
    lo = (packed & 0xF).long()
    hi = (packed >> 4).long()
    codes = torch.stack([lo, hi], dim=2).reshape(packed.shape[0], -1)
    vals = table[codes]
    s = 2.0 ** (scales.to(torch.float64) - 127.0)
    vals = vals * s.repeat_interleave(32, dim=1)
    return vals.abs() if absolute else vals


def host_ref64(a, sa, bt, sb):
    return dequant(a, sa) @ dequant(bt, sb).t()


def run(attest, fn, a, sa, bt, sb, m, n, k):
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
    fn(0, a.data_ptr(), sa.data_ptr(), bt.data_ptr(), sb.data_ptr(),
       c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    return c


def unit_scales(rows, k):
    return torch.full((rows, k // 32), 127, device="cuda", dtype=torch.uint8)


def random_case(m, n, k, seed, lo=126, hi=128):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = pack(torch.randint(0, 16, (m, k), device="cuda", generator=g))
    bt = pack(torch.randint(0, 16, (n, k), device="cuda", generator=g))
    sa = torch.randint(lo, hi + 1, (m, k // 32), device="cuda", generator=g,
                       dtype=torch.uint8)
    sb = torch.randint(lo, hi + 1, (n, k // 32), device="cuda", generator=g,
                       dtype=torch.uint8)
    return a, sa, bt, sb


@pytest.fixture(scope="module")
def case_3x2():
    """256x384x768 random exact data and its host reference, shared by
    the MFMA race screen and the VALU reference check."""
    m, n, k = 256, 384, 768
    a, sa, bt, sb = random_case(m, n, k, seed=3)
    return (m, n, k), (a, sa, bt, sb), host_ref64(a, sa, bt, sb).float()


def test_decode_table(attest):
    """One block, one K-tile, unit scales; every pair of the 16 codes
    meets (the code pairs cycle with period 16 in k and every residue
    of (i - 3j - 1) mod 16 occurs)."""
    m, n, k = 128, 128, 256
    i = torch.arange(m, device="cuda")[:, None]
    kk = torch.arange(k, device="cuda")[None, :]
    a_codes = (i + kk) % 16
    b_codes = (3 * i + 5 * kk + 1) % 16
    pairs = set()
    for row_a in range(16):
        for row_b in range(16):
            pairs |= set(zip(a_codes[row_a, :16].tolist(),
                             b_codes[row_b, :16].tolist()))
    assert len(pairs) == 256
    a, bt = pack(a_codes), pack(b_codes)
    sa, sb = unit_scales(m, k), unit_scales(n, k)
    ref = host_ref64(a, sa, bt, sb).float()
    c = run(attest, attest.mfma_gemm_mxfp4, a, sa, bt, sb, m, n, k)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


@pytest.mark.parametrize("patterned", ["A", "B"])
def test_scale_map_structured(attest, patterned):
    """All values 1.0, one operand's scales patterned by row and K
    block, the other's at 2^0: a wrong lane-to-row map, a wrong byte
    select or an A/B scale swap changes the sums."""
    m, n, k = 128, 128, 512
    ones = torch.full((m, k // 2), 0x22, device="cuda", dtype=torch.uint8)
    r = torch.arange(m, device="cuda")[:, None]
    kb = torch.arange(k // 32, device="cuda")[None, :]
    if patterned == "A":
        sa = (126 + (r + 2 * kb) % 3).to(torch.uint8)
        sb = unit_scales(n, k)
    else:
        sa = unit_scales(m, k)
        sb = (126 + (2 * r + kb) % 3).to(torch.uint8)
    ref = host_ref64(ones, sa, ones, sb).float()
    c = run(attest, attest.mfma_gemm_mxfp4, ones, sa, ones, sb, m, n, k)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


def test_random_exact_race_screen(attest, case_3x2):
    """3x2 blocks, nk = 3, five runs: bitwise every time."""
    (m, n, k), ops, ref = case_3x2
    for trial in range(5):
        c = run(attest, attest.mfma_gemm_mxfp4, *ops, m, n, k)
        assert torch.equal(c, ref), f"trial {trial}: {(c - ref).abs().max()}"


def test_random_exact_k2048(attest):
    """nk = 8: terms are multiples of 2^-4 below 2^8, so at K = 2048
    every partial sum still fits 24 bits in any order."""
    m, n, k = 128, 128, 2048
    ops = random_case(m, n, k, seed=11)
    ref = host_ref64(*ops).float()
    c = run(attest, attest.mfma_gemm_mxfp4, *ops, m, n, k)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


def test_wide_scales_within_accumulation_bound(attest):
    """Scale bytes in [117,137]: sums are no longer exact in fp32. With
    one truncation per add, |c - ref| <= K * 2^-23 * (|A| |Bt|^T)
    elementwise (each of at most K adds loses at most 2^-23 of a partial
    sum that the absolute product sum bounds)."""
    m, n, k = 128, 256, 512
    a, sa, bt, sb = random_case(m, n, k, seed=17, lo=117, hi=137)
    ref = host_ref64(a, sa, bt, sb)
    bound = k * 2.0 ** -23 * (dequant(a, sa, True) @ dequant(bt, sb, True).t())
    c = run(attest, attest.mfma_gemm_mxfp4, a, sa, bt, sb, m, n, k)
    assert not torch.isnan(c).any()
    excess = ((c.double() - ref).abs() - bound).max().item()
    assert excess <= 0.0, f"error exceeds the bound by {excess}"


def test_valu_reference_matches_host_reference(attest, case_3x2):
    (m, n, k), ops, ref = case_3x2
    c = run(attest, attest.ref_gemm_mxfp4_f32, *ops, m, n, k)
    assert torch.equal(c, ref), f"max diff {(c - ref).abs().max()}"


@pytest.mark.parametrize("m,n,k", [(128, 128, 128), (64, 128, 256)])
def test_shape_refusal(attest, m, n, k):
    a, sa, bt, sb = random_case(128, 128, 256, seed=1)
    c = torch.zeros(128, 128, device="cuda", dtype=torch.float32)
    with pytest.raises(attest.AttestationError, match=r"rc=-2$"):
        attest.mfma_gemm_mxfp4(0, a.data_ptr(), sa.data_ptr(), bt.data_ptr(),
                               sb.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    assert not c.any()  # nothing was launched


@pytest.mark.parametrize("dim", [256, 1024])
def test_attest_mxfp4(attest, dim):
    assert attest.attest_device(0, 256).ok
    first = attest.attest_mxfp4(0, dim)
    assert first.ok and first.mx_dim == dim
    assert first.mx_max_abs_err == 0.0
    assert first.mx_tflops > 0
    again = attest.attest_mxfp4(0, dim)
    assert again.ok
    assert again.mx_ref_ms == 0.0  # cached reference
    assert again.mx_checksum == first.mx_checksum
    assert attest.attest_device(0, 256).ok


def test_attestor_hook_runs_mxfp4_leg(attest, monkeypatch):
    """CC_ATTEST_MXFP4=1 through the real attestor hook on device 0: the
    summary carries the two MXFP4 keys; without the switch it does not."""
    from k8s_cc_manager_amd.device.shadow import ShadowBackend

    devices, _ = ShadowBackend(device_indices=[0]).find_devices()
    monkeypatch.setenv("CC_ATTEST_GEMM_DIM", "512")
    monkeypatch.delenv("CC_ATTEST_DEEP", raising=False)
    monkeypatch.delenv("CC_ATTEST_MXFP4", raising=False)
    plain = attest.attest_device_by_bdf(devices[0])
    assert "mxfp4_tflops" not in plain and "mxfp4_bitwise_ok" not in plain
    monkeypatch.setenv("CC_ATTEST_MXFP4", "1")
    summary = attest.attest_device_by_bdf(devices[0])
    assert set(summary) == set(plain) | {"mxfp4_tflops", "mxfp4_bitwise_ok"}
    assert summary["mxfp4_bitwise_ok"] is True
    assert summary["mxfp4_tflops"] > 0
