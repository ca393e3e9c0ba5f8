"""CPU-side surface of the compute-unit sweep: the unit key codec, the
report decode and the CC_ATTEST_CU_SWEEP switch of the attestor hook
(the ABI guard of its report struct is in test_attest_abi.py)."""

import itertools
from types import SimpleNamespace

import pytest

from k8s_cc_manager_amd.ops import attest

BASE_KEYS = {
    "arch", "cus", "gemm_tflops", "fp8_tflops", "hbm_gbps", "bitwise_ok", "xgmi",
}


FIELD_RANGES = (range(16), range(4), range(2), range(16), range(4))


def test_unit_key_round_trip_and_injective():
    keys = set()
    for unit in itertools.product(*FIELD_RANGES):
        key = attest.encode_unit(*unit)
        assert 0 <= key < 16384
        assert attest.decode_unit(key) == unit
        keys.add(key)
    assert len(keys) == 16 * 4 * 2 * 16 * 4


def test_unit_key_layout():
    """xcc << 10 | HW_ID[15:8] << 2 | simd with CU_ID 11:8, SH_ID 12,
    SE_ID 14:13 of HW_ID."""
    assert attest.encode_unit(0, 0, 0, 0, 3) == 3
    assert attest.encode_unit(0, 0, 0, 15, 0) == 15 << 2
    assert attest.encode_unit(0, 0, 1, 0, 0) == 1 << 6
    assert attest.encode_unit(0, 3, 0, 0, 0) == 3 << 7
    assert attest.encode_unit(7, 0, 0, 0, 0) == 7 << 10
    with pytest.raises(ValueError):
        attest.encode_unit(0, 4, 0, 0, 0)


def test_report_decodes_failed_units():
    c = attest._CSweepReport()
    c.device, c.cu_count, c.units_expected = 2, 256, 1024
    c.units_seen, c.cus_seen, c.xccs_seen = 1024, 256, 8
    c.units_failed, c.mfma_failures, c.lds_failures = 2, 5, 1
    c.launches, c.rounds, c.sweep_ms, c.gold_ms = 1, 32, 1.5, 0.0
    c.failed_keys[0] = attest.encode_unit(3, 2, 1, 9, 1)
    c.failed_keys[1] = attest.encode_unit(7, 0, 0, 4, 3)
    c.failed_keys[2] = 12345  # beyond units_failed: not reported
    c.ok = 0
    c.error = b"x"
    rep = attest.CuSweepReport.from_c(c)
    assert rep.failed_units == [(3, 2, 1, 9, 1), (7, 0, 0, 4, 3)]
    assert rep.ok is False and rep.error == "x"
    assert (rep.device, rep.units_seen, rep.mfma_failures, rep.lds_failures,
            rep.rounds, rep.sweep_ms) == (2, 1024, 5, 1, 32, 1.5)
    c.units_failed = 40  # only the first 16 keys are carried
    assert len(attest.CuSweepReport.from_c(c).failed_units) == 16


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


def _sweep_report(**over):
    base = dict(
        device=3, cu_count=256, units_expected=1024, units_seen=1024,
        cus_seen=256, xccs_seen=8, units_failed=0, mfma_failures=0,
        lds_failures=0, launches=1, rounds=32, sweep_ms=1.0, gold_ms=0.0,
        failed_units=[], ok=True,
    )
    base.update(over)
    return attest.CuSweepReport(**base)


@pytest.fixture
def hook(monkeypatch):
    """attest_device_by_bdf with the device-touching calls stubbed;
    yields the ordered list of calls."""
    calls = []

    def fake_main(idx, gemm_dim=1024):
        calls.append(("main", idx, gemm_dim))
        return _main_report()

    def fake_sweep(idx, rounds=32, _poison_key=-1):
        calls.append(("sweep", idx, rounds, _poison_key))
        return _sweep_report()

    monkeypatch.setattr(attest, "device_index_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(attest, "attest_device", fake_main)
    monkeypatch.setattr(attest, "cu_sweep_report", fake_sweep)
    for var in ("CC_ATTEST_DEEP", "CC_ATTEST_GEMM_DIM", "CC_ATTEST_MXFP4",
                "CC_ATTEST_CU_SWEEP"):
        monkeypatch.delenv(var, raising=False)
    return calls


DEVICE = SimpleNamespace(bdf="0000:05:00.0")


@pytest.mark.parametrize("value", [None, "0"])
def test_hook_unchanged_without_switch(hook, monkeypatch, value):
    if value is not None:
        monkeypatch.setenv("CC_ATTEST_CU_SWEEP", value)
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS
    assert hook == [("main", 3, 1024)]


def test_hook_adds_sweep_keys_with_switch(hook, monkeypatch):
    monkeypatch.setenv("CC_ATTEST_CU_SWEEP", "1")
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS | {"cu_sweep", "cu_sweep_ok"}
    assert summary["cu_sweep"] == "1024/1024"
    assert summary["cu_sweep_ok"] is True
    assert hook == [("main", 3, 1024), ("sweep", 3, 32, -1)]  # after the probe


def test_hook_propagates_failed_unit(hook, monkeypatch):
    bad = (5, 1, 0, 7, 2)
    monkeypatch.setattr(
        attest, "cu_sweep_report",
        lambda idx, rounds=32, _poison_key=-1: _sweep_report(
            units_failed=1, mfma_failures=3, failed_units=[bad], ok=False),
    )
    monkeypatch.setenv("CC_ATTEST_CU_SWEEP", "1")
    with pytest.raises(attest.AttestationError, match="xcc5/se1/sh0/cu7/simd2"):
        attest.attest_device_by_bdf(DEVICE)


def test_hook_propagates_coverage_shortfall(hook, monkeypatch):
    monkeypatch.setattr(
        attest, "cu_sweep_report",
        lambda idx, rounds=32, _poison_key=-1: _sweep_report(
            units_seen=1020, cus_seen=255, ok=False,
            error="coverage 1020/1024 after 4 launches"),
    )
    monkeypatch.setenv("CC_ATTEST_CU_SWEEP", "1")
    with pytest.raises(attest.AttestationError,
                       match="coverage 1020/1024 after 4 launches"):
        attest.attest_device_by_bdf(DEVICE)


def test_doctor_collect_keeps_its_positional_signature():
    import inspect

    from k8s_cc_manager_amd.doctor import collect

    params = inspect.signature(collect).parameters
    assert list(params)[:2] == ["run_attest", "gemm_dim"]
    assert params["cu_sweep"].default is False
