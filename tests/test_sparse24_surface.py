"""CPU-side surface of the sparse leg: the CC_ATTEST_SPARSE switch of the
attestor hook, the frozen report struct it shares with the MX legs, and
sp24_dense, the host model of the 2:4 convention."""

import ctypes
from types import SimpleNamespace

import pytest

from k8s_cc_manager_amd.ops import attest
from test_mxfp4_surface import BASE_KEYS, _main_report

DEVICE = SimpleNamespace(bdf="0000:05:00.0")


@pytest.fixture
def hook(monkeypatch):
    """The hook with the device-touching calls stubbed; the sparse calls."""
    calls = []

    def fake_sparse(idx, gemm_dim=1024, shape="32x32x32"):
        calls.append((idx, gemm_dim, shape))
        return attest.MxReport(
            device=idx, mx_dim=gemm_dim, mx_ms=0.01,
            mx_tflops=300.04 if shape == "32x32x32" else 212.26,
            mx_ref_ms=0.0, mx_max_abs_err=0.0, mx_checksum=5, ok=True)

    monkeypatch.setattr(attest, "device_index_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(attest, "attest_device", lambda idx, gemm_dim=1024: _main_report())
    monkeypatch.setattr(attest, "attest_sparse", fake_sparse)
    for name in ("DEEP", "GEMM_DIM", "MXFP4", "MXFP6", "MXFP8", "INT8", "FP64",
                 "SPARSE"):
        monkeypatch.delenv("CC_ATTEST_" + name, raising=False)
    return calls


@pytest.mark.parametrize("value", [None, "0"])
def test_hook_unchanged_without_switch(hook, monkeypatch, value):
    if value is not None:
        monkeypatch.setenv("CC_ATTEST_SPARSE", value)
    assert set(attest.attest_device_by_bdf(DEVICE)) == BASE_KEYS
    assert hook == []


def test_hook_runs_both_shapes_with_switch(hook, monkeypatch):
    monkeypatch.setenv("CC_ATTEST_SPARSE", "1")
    monkeypatch.setenv("CC_ATTEST_GEMM_DIM", "512")
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS | {"sparse_tflops", "sparse_bitwise_ok"}
    assert summary["sparse_tflops"] == 212.3  # the lower of the two
    assert summary["sparse_bitwise_ok"] is True
    assert hook == [(3, 512, "32x32x32"), (3, 512, "16x16x64")]


def test_hook_propagates_sparse_failure(hook, monkeypatch):
    def failing(idx, gemm_dim=1024, shape="32x32x32"):
        raise attest.AttestationError("sparse attestation FAILED")

    monkeypatch.setattr(attest, "attest_sparse", failing)
    monkeypatch.setenv("CC_ATTEST_SPARSE", "1")
    with pytest.raises(attest.AttestationError, match="sparse"):
        attest.attest_device_by_bdf(DEVICE)


@pytest.mark.skipif(not attest._LIB_PATH.exists(), reason="libccattest.so not built")
def test_mx_report_layout_frozen_with_sparse_entry_point():
    lib = ctypes.CDLL(str(attest._LIB_PATH))
    assert hasattr(lib, "cc_attest_sparse")
    assert lib.cc_mx_report_sizeof() == ctypes.sizeof(attest._CMxReport) == 320


def test_sp24_dense_one_row_of_two_groups():
    """One byte: low nibble 0xD = positions (1, 3) for group 0, high nibble
    0x8 = positions (0, 2) for group 1."""
    torch = pytest.importorskip("torch")
    ac = torch.tensor([[5.0, -7.0, 2.0, 3.0]], dtype=torch.bfloat16)
    am = torch.tensor([[0x8D]], dtype=torch.uint8)
    want = torch.tensor([[0, 5.0, 0, -7.0, 2.0, 0, 3.0, 0]], dtype=torch.bfloat16)
    assert torch.equal(attest.sp24_dense(ac, am), want)
