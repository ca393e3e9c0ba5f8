"""CPU-side surface of the HBM march: the ABI guard of its report
struct, the host model of the pattern, the report decode, the
CC_ATTEST_HBM_MIB switch of the attestor hook and doctor's signature."""

import ctypes
import random
from types import SimpleNamespace

import pytest

from k8s_cc_manager_amd.ops import attest

BASE_KEYS = {
    "arch", "cus", "gemm_tflops", "fp8_tflops", "hbm_gbps", "bitwise_ok", "xgmi",
}
HBM_KEYS = {"hbm_march_mib", "hbm_march_gbps", "hbm_march_ok", "hbm_scrubbed"}
NO_OFFSET = (1 << 64) - 1


@pytest.mark.skipif(not attest._LIB_PATH.exists(),
                    reason="libccattest.so not built")
def test_report_struct_abi_parity():
    lib = ctypes.CDLL(str(attest._LIB_PATH))  # restype defaults to c_int
    assert lib.cc_hbm_report_sizeof() == ctypes.sizeof(attest._CHbmReport)
    assert ctypes.sizeof(attest._CHbmReport) == 704


def _pattern_cases():
    rng = random.Random(0x5EED)
    ws = [0, 1, 3, 2**32 - 1, 2**32, 2**32 + 1, 2**40 + 5, 2**44 - 1]
    ws += [rng.randrange(2**44) for _ in range(300)]
    return ws


def test_pattern_closed_form():
    assert attest.hbm_pattern_word(0, 0) == 0x5EED0001
    assert attest.hbm_pattern_word(1, 0) == (2654435769 + 0x5EED0001) % 2**32
    assert attest.hbm_pattern_word(2**32, 0) == (2246822519 + 0x5EED0001) % 2**32
    assert attest.hbm_pattern_word(2**40 + 5, 0) == (
        5 * 2654435769 + 256 * 2246822519 + 0x5EED0001) % 2**32


def test_pattern_separates_single_bit_aliases():
    for w in _pattern_cases():
        for phase in (0, 1):
            here = attest.hbm_pattern_word(w, phase)
            assert 0 <= here < 2**32
            for bit in range(44):
                assert attest.hbm_pattern_word(w ^ (1 << bit), phase) != here, (
                    w, bit, phase)


def test_pattern_phases():
    for w in _pattern_cases():
        p = attest.hbm_pattern_word(w, 0)
        assert attest.hbm_pattern_word(w, 1) == p ^ 0xFFFFFFFF
        assert attest.hbm_pattern_word(w, 2) == 0
    with pytest.raises(ValueError):
        attest.hbm_pattern_word(0, 3)


def test_report_decode():
    c = attest._CHbmReport()
    c.device, c.chunks, c.passes, c.n_bad = 2, 4, 4, 2
    c.bytes_requested = c.bytes_tested = 8 << 20
    c.chunk_bytes, c.origin = 2 << 20, 16
    c.mismatch_words, c.first_bad_offset = 40, 0x1004
    c.bad_offset[0], c.bad_expected[0], c.bad_got[0], c.bad_pass[0] = (
        0x2008, 0xDEADBEEF, 0xDEADBEEE, 3)
    c.bad_offset[1], c.bad_expected[1], c.bad_got[1], c.bad_pass[1] = (
        0x1004, 7, 5, 2)
    c.bad_offset[2] = 0x9999  # beyond n_bad: not reported
    c.fill_ms, c.flip_ms, c.scrub_ms, c.zero_ms = 1.0, 2.0, 3.0, 4.0
    c.alloc_ms, c.gbps = 0.5, 1234.5
    c.beyond_cache, c.scrubbed, c.ok = 0, 0, 0
    c.error = b"x"
    rep = attest.HbmMarchReport.from_c(c)
    assert rep.bad == [(0x2008, 0xDEADBEEF, 0xDEADBEEE, 3), (0x1004, 7, 5, 2)]
    assert rep.first_bad_offset == 0x1004
    assert rep.ok is False and rep.scrubbed is False
    assert rep.beyond_cache is False and rep.error == "x"
    assert (rep.device, rep.chunks, rep.passes, rep.bytes_tested,
            rep.chunk_bytes, rep.origin, rep.mismatch_words, rep.zero_ms,
            rep.gbps) == (2, 4, 4, 8 << 20, 2 << 20, 16, 40, 4.0, 1234.5)

    c.n_bad = 40  # only 16 records are carried
    assert len(attest.HbmMarchReport.from_c(c).bad) == 16

    c.n_bad, c.mismatch_words, c.first_bad_offset = 0, 0, NO_OFFSET
    c.scrubbed = c.ok = c.beyond_cache = 1
    clean = attest.HbmMarchReport.from_c(c)
    assert clean.first_bad_offset is None and clean.bad == []
    assert clean.ok is True and clean.scrubbed is True
    assert clean.beyond_cache is True


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


def _sweep_report():
    return attest.CuSweepReport(
        device=3, cu_count=256, units_expected=1024, units_seen=1024,
        cus_seen=256, xccs_seen=8, units_failed=0, mfma_failures=0,
        lds_failures=0, launches=1, rounds=32, sweep_ms=1.0, gold_ms=0.0,
        failed_units=[], ok=True,
    )


def _march_report(mib=8, chunk_mib=1024, **over):
    chunk = min(mib, chunk_mib) << 20
    base = dict(
        device=3, bytes_requested=mib << 20, bytes_tested=mib << 20,
        chunk_bytes=chunk, origin=0, chunks=-(-(mib << 20) // chunk),
        passes=4, mismatch_words=0, first_bad_offset=None, bad=[],
        fill_ms=1.0, flip_ms=1.0, scrub_ms=1.0, zero_ms=1.0, alloc_ms=1.0,
        gbps=3456.7, beyond_cache=False, scrubbed=True, ok=True,
    )
    base.update(over)
    return attest.HbmMarchReport(**base)


@pytest.fixture
def hook(monkeypatch):
    """attest_device_by_bdf with the device-touching calls stubbed;
    yields the ordered list of calls."""
    calls = []

    def fake_main(idx, gemm_dim=1024):
        calls.append(("main", idx, gemm_dim))
        return _main_report()

    def fake_sweep(idx, rounds=32, _poison_key=-1):
        calls.append(("sweep", idx))
        return _sweep_report()

    def fake_march(idx, mib, chunk_mib=1024, _origin=0, _poison_offset=-1,
                   _poison_after=0):
        calls.append(("march", idx, mib, chunk_mib, _origin, _poison_offset))
        return _march_report(mib, chunk_mib)

    monkeypatch.setattr(attest, "device_index_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(attest, "attest_device", fake_main)
    monkeypatch.setattr(attest, "cu_sweep_report", fake_sweep)
    monkeypatch.setattr(attest, "hbm_march_report", fake_march)
    for var in ("CC_ATTEST_DEEP", "CC_ATTEST_GEMM_DIM", "CC_ATTEST_MXFP4",
                "CC_ATTEST_CU_SWEEP", "CC_ATTEST_HBM_MIB",
                "CC_ATTEST_HBM_CHUNK_MIB"):
        monkeypatch.delenv(var, raising=False)
    return calls


DEVICE = SimpleNamespace(bdf="0000:05:00.0")


@pytest.mark.parametrize("value", [None, "", "0"])
def test_hook_unchanged_without_switch(hook, monkeypatch, value):
    if value is not None:
        monkeypatch.setenv("CC_ATTEST_HBM_MIB", value)
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS
    assert hook == [("main", 3, 1024)]


def test_hook_adds_march_keys_with_switch(hook, monkeypatch):
    monkeypatch.setenv("CC_ATTEST_HBM_MIB", "8")
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS | HBM_KEYS
    assert summary["hbm_march_mib"] == 8
    assert summary["hbm_march_gbps"] == 3457
    assert summary["hbm_march_ok"] is True
    assert summary["hbm_scrubbed"] is True
    assert hook == [("main", 3, 1024), ("march", 3, 8, 1024, 0, -1)]


def test_hook_runs_march_after_sweep_with_chunk_size(hook, monkeypatch):
    monkeypatch.setenv("CC_ATTEST_CU_SWEEP", "1")
    monkeypatch.setenv("CC_ATTEST_HBM_MIB", "8")
    monkeypatch.setenv("CC_ATTEST_HBM_CHUNK_MIB", "2")
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS | HBM_KEYS | {"cu_sweep", "cu_sweep_ok"}
    assert hook == [("main", 3, 1024), ("sweep", 3),
                    ("march", 3, 8, 2, 0, -1)]


def test_hook_propagates_bad_word(hook, monkeypatch):
    monkeypatch.setattr(
        attest, "hbm_march_report",
        lambda idx, mib, chunk_mib=1024, _origin=0, _poison_offset=-1,
        _poison_after=0: _march_report(
            mib, mismatch_words=3, first_bad_offset=0x2ffffc,
            bad=[(0x2ffffc, 0x12345678, 0x12345679, 2)], scrubbed=False,
            ok=False),
    )
    monkeypatch.setenv("CC_ATTEST_HBM_MIB", "8")
    with pytest.raises(attest.AttestationError) as err:
        attest.attest_device_by_bdf(DEVICE)
    msg = str(err.value)
    assert "0x2ffffc" in msg and "3 wrong word" in msg
    assert "pass 2" in msg and "0x00000001" in msg


def test_hook_propagates_short_allocation(hook, monkeypatch):
    monkeypatch.setattr(
        attest, "hbm_march_report",
        lambda idx, mib, chunk_mib=1024, _origin=0, _poison_offset=-1,
        _poison_after=0: _march_report(
            mib, bytes_tested=0, passes=0, scrubbed=False, ok=False,
            gbps=0.0, error="allocated 4096 of 8192 MiB"),
    )
    monkeypatch.setenv("CC_ATTEST_HBM_MIB", "8192")
    with pytest.raises(attest.AttestationError,
                       match="allocated 4096 of 8192 MiB"):
        attest.attest_device_by_bdf(DEVICE)


def test_doctor_collect_keeps_its_leading_signature():
    import inspect

    from k8s_cc_manager_amd.doctor import collect

    params = inspect.signature(collect).parameters
    assert list(params)[:3] == ["run_attest", "gemm_dim", "cu_sweep"]
    assert params["cu_sweep"].default is False
    assert params["hbm_march_mib"].default == 0
