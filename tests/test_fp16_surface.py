"""CPU-side surface of the FP16 leg: the CC_ATTEST_FP16 switch of the
attestor hook, and the frozen report struct it shares with the other
exact-GEMM legs."""

import ctypes
from types import SimpleNamespace

import pytest

from k8s_cc_manager_amd.ops import attest
from test_mxfp4_surface import BASE_KEYS, _main_report

DEVICE = SimpleNamespace(bdf="0000:05:00.0")


@pytest.fixture
def hook(monkeypatch):
    """The hook with the device-touching calls stubbed; the fp16 calls."""
    calls = []

    def fake_f16(idx, gemm_dim=1024, shape="32x32x16"):
        calls.append((idx, gemm_dim, shape))
        return attest.MxReport(
            device=idx, mx_dim=gemm_dim, mx_ms=0.01,
            mx_tflops=150.04 if shape == "32x32x16" else 131.26,
            mx_ref_ms=0.0, mx_max_abs_err=0.0, mx_checksum=5, ok=True)

    monkeypatch.setattr(attest, "device_index_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(attest, "attest_device", lambda idx, gemm_dim=1024: _main_report())
    monkeypatch.setattr(attest, "attest_fp16", fake_f16)
    for name in ("DEEP", "GEMM_DIM", "MXFP4", "MXFP6", "MXFP8", "INT8", "FP64",
                 "SPARSE", "FP16"):
        monkeypatch.delenv("CC_ATTEST_" + name, raising=False)
    return calls


@pytest.mark.parametrize("value", [None, "0"])
def test_hook_unchanged_without_switch(hook, monkeypatch, value):
    if value is not None:
        monkeypatch.setenv("CC_ATTEST_FP16", value)
    assert set(attest.attest_device_by_bdf(DEVICE)) == BASE_KEYS
    assert hook == []


def test_hook_runs_both_shapes_with_switch(hook, monkeypatch):
    monkeypatch.setenv("CC_ATTEST_FP16", "1")
    monkeypatch.setenv("CC_ATTEST_GEMM_DIM", "512")
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS | {"fp16_tflops", "fp16_bitwise_ok"}
    assert summary["fp16_tflops"] == 131.3  # the lower of the two
    assert summary["fp16_bitwise_ok"] is True
    assert hook == [(3, 512, "32x32x16"), (3, 512, "16x16x32")]
    assert attest.F16_SHAPES == ("32x32x16", "16x16x32")


def test_hook_propagates_fp16_failure(hook, monkeypatch):
    def failing(idx, gemm_dim=1024, shape="32x32x16"):
        raise attest.AttestationError("fp16 attestation FAILED")

    monkeypatch.setattr(attest, "attest_fp16", failing)
    monkeypatch.setenv("CC_ATTEST_FP16", "1")
    with pytest.raises(attest.AttestationError, match="fp16"):
        attest.attest_device_by_bdf(DEVICE)


@pytest.mark.skipif(not attest._LIB_PATH.exists(), reason="libccattest.so not built")
def test_mx_report_layout_frozen_with_fp16_entry_point():
    lib = ctypes.CDLL(str(attest._LIB_PATH))
    assert hasattr(lib, "cc_attest_fp16")
    assert lib.cc_mx_report_sizeof() == ctypes.sizeof(attest._CMxReport) == 320
