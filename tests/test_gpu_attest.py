"""GPU tests: the CDNA4 attestation probe on a real MI355X.

Numerics: the hand-written MFMA kernel is compared against a plain
PyTorch fp32 reference of the same op (and, inside the probe, against
an independent on-device VALU fp32 kernel — bitwise, on integer data).
"""

import pytest

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

pytestmark = [
    gpu,
    pytest.mark.skipif(
        not torch.cuda.is_available(), reason="needs an MI355X"
    ),
]


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a

    assert a.probe_available(), "libccattest.so must load on a GPU box"
    return a


def test_native_library_loads(attest):
    # The HIP path must be the one that runs: loudly require the .so.
    assert attest._LIB_PATH.exists()
    assert attest.device_count() >= 1


@pytest.mark.parametrize("m,n,k", [(256, 256, 256), (128, 384, 512), (512, 128, 192)])
def test_mfma_gemm_matches_torch_fp32(attest, m, n, k):
    torch.manual_seed(1234 + m + n + k)
    a = torch.randn(m, k, device="cuda", dtype=torch.float32).bfloat16()
    bt = torch.randn(n, k, device="cuda", dtype=torch.float32).bfloat16()
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
    attest.mfma_gemm_bf16(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    ref = a.float() @ bt.float().t()
    err = (c - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 2e-3 * max(scale, 1.0), f"max_abs_err={err} (scale={scale})"


def test_mfma_gemm_integer_exact(attest):
    """Small-integer bf16 inputs: MFMA (fp32 acc) must be EXACT."""
    m = n = 256
    k = 512
    a = (torch.randint(-2, 2, (m, k), device="cuda")).bfloat16()
    bt = (torch.randint(-2, 2, (n, k), device="cuda")).bfloat16()
    c = torch.empty(m, n, device="cuda", dtype=torch.float32)
    attest.mfma_gemm_bf16(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    ref = a.float() @ bt.float().t()
    assert torch.equal(c, ref)


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize(
    "m,n,k", [(256, 256, 128), (512, 256, 384), (256, 256, 512), (256, 512, 1024)]
)
def test_mfma_gemm_256_template_matches_torch(attest, m, n, k, which):
    """The deep-pipelined 256x256 8-phase variant — race-sensitive, so
    run it several times per shape (sync-structure screening)."""
    torch.manual_seed(m * 7 + n * 3 + k)
    a = torch.randn(m, k, device="cuda", dtype=torch.float32).bfloat16()
    bt = torch.randn(n, k, device="cuda", dtype=torch.float32).bfloat16()
    ref = a.float() @ bt.float().t()
    scale = ref.abs().max().item()
    for trial in range(5):
        c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
        attest.mfma_gemm_bf16_variant(
            0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, which
        )
        torch.cuda.synchronize()
        err = (c - ref).abs().max().item()
        assert err <= 2e-3 * max(scale, 1.0), f"trial {trial} which={which}: err={err}"


def test_mfma_gemm_bf16_4blk_bitwise(attest):
    """The 4-blocks/CU single-buffered bf16 variant (which=3): bitwise
    integer race screen (serial stage window discipline)."""
    m = n = 512
    k = 1024
    a = (torch.randint(-2, 2, (m, k), device="cuda")).bfloat16()
    bt = (torch.randint(-2, 2, (n, k), device="cuda")).bfloat16()
    ref = a.float() @ bt.float().t()
    for trial in range(5):
        c = torch.empty(m, n, device="cuda", dtype=torch.float32)
        attest.mfma_gemm_bf16_variant(
            0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, 3
        )
        torch.cuda.synchronize()
        assert torch.equal(c, ref), f"trial {trial} mismatch"


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_mfma_gemm_bf16_variants_nonsquare_bitwise(attest, which):
    """Every forced bf16 variant on a non-square shape (2x4 blocks for
    the 128-tile kernels, 1x2 for the 256-tile ones): a swapped M/N in
    the shared epilogue or block mapping is a bitwise mismatch."""
    m, n, k = 256, 512, 512
    torch.manual_seed(which)
    a = (torch.randint(-2, 2, (m, k), device="cuda")).bfloat16()
    bt = (torch.randint(-2, 2, (n, k), device="cuda")).bfloat16()
    ref = a.float() @ bt.float().t()
    for trial in range(5):
        c = torch.empty(m, n, device="cuda", dtype=torch.float32)
        attest.mfma_gemm_bf16_variant(
            0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, which
        )
        torch.cuda.synchronize()
        assert torch.equal(c, ref), f"which={which} trial={trial}"


@pytest.mark.parametrize("which", [4, -1])
def test_mfma_gemm_bf16_unknown_variant_refused(attest, which):
    """A number that names no kernel is refused with rc=-2 and nothing
    is launched: c stays as it was."""
    m, n, k = 256, 256, 256
    a = torch.ones(m, k, device="cuda").bfloat16()
    bt = torch.ones(n, k, device="cuda").bfloat16()
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.float32)
    with pytest.raises(attest.AttestationError, match="rc=-2"):
        attest.mfma_gemm_bf16_variant(
            0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, which
        )
    torch.cuda.synchronize()
    assert torch.isnan(c).all()


def test_mfma_gemm_256_integer_exact_race_screen(attest):
    """Integer data: any stale-LDS race shows as a bitwise mismatch."""
    m = n = 512
    k = 768
    a = (torch.randint(-2, 2, (m, k), device="cuda")).bfloat16()
    bt = (torch.randint(-2, 2, (n, k), device="cuda")).bfloat16()
    ref = a.float() @ bt.float().t()
    for trial in range(10):
        c = torch.empty(m, n, device="cuda", dtype=torch.float32)
        attest.mfma_gemm_bf16_variant(
            0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k, 1
        )
        torch.cuda.synchronize()
        assert torch.equal(c, ref), f"trial {trial} mismatch"


def test_ref_gemm_matches_torch(attest):
    m, n, k = 128, 128, 256
    a = torch.randn(m, k, device="cuda").bfloat16()
    bt = torch.randn(n, k, device="cuda").bfloat16()
    c = torch.empty(m, n, device="cuda", dtype=torch.float32)
    attest.ref_gemm_f32(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    ref = a.float() @ bt.float().t()
    assert (c - ref).abs().max().item() < 1e-3


def test_attest_device_full_probe(attest):
    rep = attest.attest_device(0, gemm_dim=1024)
    assert rep.ok
    assert "gfx950" in rep.arch or rep.cu_count > 0
    assert rep.max_abs_err == 0.0  # integer inputs: bitwise agreement
    assert rep.fp8_max_abs_err == 0.0  # fp8 MFMA path, same ground truth
    assert rep.lds_failures == 0
    assert rep.gemm_tflops > 10.0, f"MFMA path suspiciously slow: {rep.gemm_tflops}"
    assert rep.fp8_tflops > 10.0, f"fp8 MFMA path suspiciously slow: {rep.fp8_tflops}"
    assert rep.hbm_gbps > 500.0
    assert rep.checksum != 0
    # xGMI traffic leg: every ATTEMPTED link must carry data and
    # checksum-verify on the peer (vacuous 0/0 on a 1-GPU lease; on an
    # 8-GPU node this attests all 7 links per device unless
    # CC_ATTEST_XGMI_MAX_PEERS bounds the per-probe sample)
    assert rep.peers_attempted == rep.peers_accessible  # env unset here
    assert rep.peers_verified == rep.peers_attempted
    if rep.peers_accessible > 0:
        assert rep.xgmi_gbps_min > 1.0, f"dead xGMI link: {rep.xgmi_gbps_min}"
        assert rep.xgmi_ms > 0.0


def test_attest_checksum_deterministic(attest):
    r1 = attest.attest_device(0, gemm_dim=512)
    r2 = attest.attest_device(0, gemm_dim=512)
    assert r1.checksum == r2.checksum


def test_device_alive_liveness(attest):
    assert attest.device_count() >= 1
    assert attest.device_alive(0) == 0


def test_legs_keep_their_caches_across_main_dim_changes(attest):
    """A change of the main probe's dim frees only the main probe's
    buffers: the MXFP4 reference, the sweep's golden images and unit
    table and the liveness word stay."""
    mx = attest.attest_mxfp4(0, 256)
    attest.sweep_compute_units(0, rounds=1)
    units = attest.cu_sweep_units(0)
    assert units
    assert attest.device_alive(0) == 0
    assert attest.attest_device(0, 128).ok
    assert attest.attest_device(0, 256).ok
    assert attest.device_alive(0) == 0
    again = attest.attest_mxfp4(0, 256)
    assert again.mx_ref_ms == 0.0  # cached reference
    assert again.mx_checksum == mx.mx_checksum
    assert attest.cu_sweep_units(0) == units
    assert attest.sweep_compute_units(0, rounds=1).gold_ms == 0.0  # cached


def test_shutdown_frees_every_leg(attest):
    before = attest.attest_device(0, 128)
    attest.attest_mxfp4(0, 256)
    attest.sweep_compute_units(0, rounds=1)
    assert attest.device_alive(0) == 0
    attest.shutdown()
    assert attest.cu_sweep_units(0) == []
    after = attest.attest_device(0, 128)
    assert after.ok and after.ref_ms > 0.0  # reference recomputed
    assert after.checksum == before.checksum
    assert attest.attest_mxfp4(0, 256).mx_ref_ms > 0.0
    sweep = attest.sweep_compute_units(0, rounds=1)
    assert sweep.ok and sweep.units_failed == 0 and sweep.gold_ms > 0.0
    assert sweep.units_seen == sweep.units_expected
    assert attest.device_alive(0) == 0


def test_shadow_backend_transition_with_real_probe(attest):
    """A full 4-phase transition on the shadow tier with the real
    attestation probe gating verify (BASELINE config 4 analogue)."""
    from k8s_cc_manager_amd.core.transition import TransitionEngine
    from k8s_cc_manager_amd.device.shadow import ShadowBackend

    be = ShadowBackend(device_indices=[0])
    devices, n = be.find_devices()
    assert n == 1
    engine = TransitionEngine(
        attestor=lambda d: attest.attest_device(d.hip_index, gemm_dim=512)
    )
    report = engine.apply_cc_mode(devices, devices, "on")
    assert report.ok, report.error
    assert devices[0].query_cc_mode() == "on"
    assert report.phases.get("verify", 0) > 0
