"""CPU-side surface of the MXFP4 attestation leg: the CC_ATTEST_MXFP4
switch of the attestor hook (the ABI guard of its report struct is in
test_attest_abi.py)."""

from types import SimpleNamespace

import pytest

from k8s_cc_manager_amd.ops import attest

BASE_KEYS = {
    "arch", "cus", "gemm_tflops", "fp8_tflops", "hbm_gbps", "bitwise_ok", "xgmi",
}


def _main_report():
    return attest.AttestReport(
        device=0, cu_count=256, arch="gfx950:sramecc+:xnack-",
        vram_total_mb=1, gemm_dim=1024, gemm_ms=1.0, gemm_tflops=64.04,
        ref_ms=0.0, max_abs_err=0.0, checksum=1, fp8_ms=1.0,
        fp8_tflops=111.16, fp8_max_abs_err=0.0, lds_ms=1.0, lds_failures=0,
        hbm_ms=1.0, hbm_gbps=4000.0, peer_count=0, peers_accessible=0,
        peers_attempted=0, peers_verified=0, xgmi_ms=0.0, xgmi_gbps_min=0.0,
        xgmi_gbps_max=0.0, ok=True,
    )


@pytest.fixture
def hook(monkeypatch):
    """attest_device_by_bdf with the three device-touching calls stubbed;
    yields the list of attest_mxfp4 calls."""
    calls = []

    def fake_mx(idx, gemm_dim=1024):
        calls.append((idx, gemm_dim))
        return attest.MxReport(
            device=idx, mx_dim=gemm_dim, mx_ms=0.01, mx_tflops=212.26,
            mx_ref_ms=0.0, mx_max_abs_err=0.0, mx_checksum=5, ok=True,
        )

    monkeypatch.setattr(attest, "device_index_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(attest, "attest_device", lambda idx, gemm_dim=1024: _main_report())
    monkeypatch.setattr(attest, "attest_mxfp4", fake_mx)
    monkeypatch.delenv("CC_ATTEST_DEEP", raising=False)
    monkeypatch.delenv("CC_ATTEST_GEMM_DIM", raising=False)
    monkeypatch.delenv("CC_ATTEST_MXFP4", raising=False)
    return calls


DEVICE = SimpleNamespace(bdf="0000:05:00.0")


@pytest.mark.parametrize("value", [None, "0"])
def test_hook_unchanged_without_switch(hook, monkeypatch, value):
    if value is not None:
        monkeypatch.setenv("CC_ATTEST_MXFP4", value)
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS
    assert hook == []


def test_hook_adds_mxfp4_keys_with_switch(hook, monkeypatch):
    monkeypatch.setenv("CC_ATTEST_MXFP4", "1")
    monkeypatch.setenv("CC_ATTEST_GEMM_DIM", "512")
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS | {"mxfp4_tflops", "mxfp4_bitwise_ok"}
    assert summary["mxfp4_tflops"] == 212.3
    assert summary["mxfp4_bitwise_ok"] is True
    assert hook == [(3, 512)]


def test_hook_propagates_mxfp4_failure(hook, monkeypatch):
    def failing(idx, gemm_dim=1024):
        raise attest.AttestationError("mxfp4 attestation FAILED")

    monkeypatch.setattr(attest, "attest_mxfp4", failing)
    monkeypatch.setenv("CC_ATTEST_MXFP4", "1")
    with pytest.raises(attest.AttestationError, match="mxfp4"):
        attest.attest_device_by_bdf(DEVICE)
