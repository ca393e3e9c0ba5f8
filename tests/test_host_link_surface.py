"""CPU-side surface of the host-link leg: the ABI guard of its report
struct, the per-pass host model of the pattern, the CPU fill and compare
(cc_host_pattern, which makes no GPU call) against a numpy model with
sentinels, the refusals, the report decode, the CC_ATTEST_HOST_MIB /
CC_ATTEST_HOST_MIN_GBPS switches of the attestor hook and doctor's new
keyword."""

import ctypes
import functools
import random
from types import SimpleNamespace

import pytest

from k8s_cc_manager_amd.ops import attest

np = pytest.importorskip("numpy")

needs_lib = pytest.mark.skipif(not attest._LIB_PATH.exists(),
                               reason="libccattest.so not built")

BASE_KEYS = {
    "arch", "cus", "gemm_tflops", "fp8_tflops", "hbm_gbps", "bitwise_ok", "xgmi",
}
HBM_KEYS = {"hbm_march_mib", "hbm_march_gbps", "hbm_march_ok", "hbm_scrubbed"}
HOST_KEYS = {"host_link_mib", "host_link_gbps", "host_link_ok"}
NO_OFFSET = (1 << 64) - 1

MIB = 1 << 20
SIZES = [16, 4096 + 16, 3 * MIB + 48]
# with the second origin w crosses 2^32 one MiB into the buffer
ORIGINS = [0, 2**34 - 2**20]
SHAPES = [(n, o) for n in SIZES for o in ORIGINS]
GUARD = 16  # uint32 words of sentinel on each side: 64 bytes
SENTINEL = 0x5A17E4E1


@needs_lib
def test_report_struct_abi_parity():
    lib = ctypes.CDLL(str(attest._LIB_PATH))  # restype defaults to c_int
    assert lib.cc_host_report_sizeof() == ctypes.sizeof(attest._CHostReport)
    assert ctypes.sizeof(attest._CHostReport) == 744


def test_pass_pattern_is_the_march_pattern_at_the_pass_origin():
    rng = random.Random(0x11F0)
    offsets = [0, 4, 2**20 - 4, 2**30 - 4] + [
        4 * rng.randrange(2**28) for _ in range(300)]
    for origin in (0, 16, 2**34 - 2**20, 2**47):
        for off in offsets:
            words = []
            for k in range(1, 6):
                phase = 0 if k in (1, 3, 5) else 1
                want = attest.hbm_pattern_word(
                    (origin + (k << 40) + off) // 4, phase)
                assert attest.host_link_word(off, k, origin) == want
                words.append(want)
            # no two passes expect the same word at the same offset
            assert len(set(words)) == 5, (origin, off)
    # 2^40 bytes are 2^38 words: the high half of w moves by 64 per pass
    assert attest.host_link_word(0, 1) == (64 * 2246822519 + 0x5EED0001) % 2**32
    for bad in (0, 6):
        with pytest.raises(ValueError):
            attest.host_link_word(0, bad)


@functools.lru_cache(maxsize=None)
def model(nbytes, origin, phase):
    """uint32 words of the window in `phase`, read-only."""
    w = np.uint64(origin // 4) + np.arange(nbytes // 4, dtype=np.uint64)
    lo = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (w >> np.uint64(32)).astype(np.uint32)
    p = lo * np.uint32(2654435769) + hi * np.uint32(2246822519)
    p = p + np.uint32(0x5EED0001)
    out = {0: p, 1: ~p, 2: np.zeros_like(p)}[phase]
    out.setflags(write=False)
    return out


class Guarded:
    """nbytes of uint32 in host memory between two sentinel runs, the
    buffer 64-byte aligned."""

    def __init__(self, nbytes):
        self.n = nbytes // 4
        raw = np.full(self.n + 2 * GUARD + 16, SENTINEL, dtype=np.uint32)
        skip = (-raw.ctypes.data % 64) // 4
        self.whole = raw[skip:skip + self.n + 2 * GUARD]
        self.buf = self.whole[GUARD:GUARD + self.n]
        self.ptr = self.buf.ctypes.data
        assert self.ptr % 16 == 0

    def assert_guards_intact(self):
        assert (self.whole[:GUARD] == SENTINEL).all()
        assert (self.whole[GUARD + self.n:] == SENTINEL).all()


def corrupt(g, origin):
    """XOR chosen words of a phase-0 buffer: the first, the last, one in
    the middle and the two around the 2^32 crossing; returns {(byte
    offset, expected, got)}."""
    n = g.n
    picks = {0: 0x00000001, n - 1: 0x80000000, n // 2: 0xFFFFFFFF}
    edge = 2**32 - 1 - origin // 4  # the word at w = 2^32 - 1
    if 0 <= edge and edge + 1 < n:
        picks[edge] = 0x00000004
        picks[edge + 1] = 0x5A5A5A5A
    p = model(4 * n, origin, 0)
    for i, mask in picks.items():
        g.buf[i] ^= np.uint32(mask)
    return {(4 * i, int(p[i]), int(p[i]) ^ m) for i, m in picks.items()}


@needs_lib
@pytest.mark.parametrize("nbytes,origin", SHAPES)
def test_cpu_fill_equals_numpy_model(nbytes, origin):
    g = Guarded(nbytes)
    for phase in (0, 1, 2):
        rep = attest.host_pattern(g.ptr, nbytes, origin, write=phase)
        assert rep.ok and rep.device == -1 and rep.passes == 1
        assert rep.bytes_tested == nbytes and rep.origin == origin
        assert rep.mismatch_words == 0 and rep.bad == []
        assert rep.first_bad_offset is None
        assert np.array_equal(g.buf, model(nbytes, origin, phase)), phase
        assert attest.host_pattern(g.ptr, nbytes, origin, check=phase).ok
    g.assert_guards_intact()


@needs_lib
@pytest.mark.parametrize("nbytes,origin", SHAPES)
def test_cpu_compare_finds_exactly_what_was_broken(nbytes, origin):
    g = Guarded(nbytes)
    g.buf[:] = model(nbytes, origin, 0)
    broken = corrupt(g, origin)
    before = g.buf.copy()
    rep = attest.host_pattern(g.ptr, nbytes, origin, check=0)
    assert not rep.ok
    assert rep.mismatch_words == len(broken) == len(rep.bad)
    assert rep.first_bad_offset == 0
    assert {b[:3] for b in rep.bad} == broken
    assert all(b[3] == 0 for b in rep.bad)
    assert np.array_equal(g.buf, before)  # compare writes nothing
    g.assert_guards_intact()


@needs_lib
def test_cpu_compare_counts_past_sixteen_records():
    nbytes = 4096
    g = Guarded(nbytes)
    g.buf[:] = model(nbytes, 0, 1)
    g.buf[100:140] ^= np.uint32(2)
    rep = attest.host_pattern(g.ptr, nbytes, 0, check=1)
    assert rep.mismatch_words == 40 and len(rep.bad) == 16
    assert rep.first_bad_offset == 400
    assert [b[0] for b in rep.bad] == [400 + 4 * i for i in range(16)]


@needs_lib
def test_cpu_pattern_refusals():
    g = Guarded(64)
    refused = pytest.raises(attest.AttestationError, match=r"rc=-2$")
    for kwargs in (
        dict(ptr=g.ptr + 4, nbytes=32, write=0),   # misaligned pointer
        dict(ptr=g.ptr, nbytes=0, write=0),
        dict(ptr=g.ptr, nbytes=24, write=0),       # not a multiple of 16
        dict(ptr=g.ptr, nbytes=32, check=0, write=0),  # both
        dict(ptr=g.ptr, nbytes=32),                # neither
        dict(ptr=g.ptr, nbytes=32, write=3),
        dict(ptr=g.ptr, nbytes=32, write=0, origin=8),
    ):
        with refused:
            attest.host_pattern(**kwargs)
    assert (g.whole == SENTINEL).all()  # nothing was written


def test_report_decode():
    c = attest._CHostReport()
    c.device, c.engine, c.passes, c.n_bad = 2, 1, 5, 2
    c.bytes_requested = c.bytes_tested = 8 << 20
    c.origin, c.mismatch_words, c.first_bad_offset = 16, 40, 0x1004
    c.bad_offset[0], c.bad_expected[0], c.bad_got[0], c.bad_pass[0] = (
        0x2008, 0xDEADBEEF, 0xDEADBEEE, 5)
    c.bad_offset[1], c.bad_expected[1], c.bad_got[1], c.bad_pass[1] = (
        0x1004, 7, 5, 2)
    c.bad_offset[2] = 0x9999  # beyond n_bad: not reported
    c.pull_ms, c.push_ms, c.h2d_ms, c.d2h_ms, c.duplex_ms = 1., 2., 3., 4., 5.
    c.pull_gbps, c.push_gbps, c.h2d_gbps, c.d2h_gbps = 11., 12., 13., 14.
    c.duplex_pull_gbps, c.duplex_push_gbps = 15., 16.
    c.host_ms, c.alloc_ms, c.ok = 6.0, 0.5, 0
    c.error = b"x"
    rep = attest.HostLinkReport.from_c(c)
    assert rep.bad == [(0x2008, 0xDEADBEEF, 0xDEADBEEE, 5), (0x1004, 7, 5, 2)]
    assert rep.first_bad_offset == 0x1004
    assert rep.ok is False and rep.error == "x"
    assert (rep.device, rep.engine, rep.passes, rep.bytes_requested,
            rep.bytes_tested, rep.origin, rep.mismatch_words) == (
                2, 1, 5, 8 << 20, 8 << 20, 16, 40)
    assert (rep.pull_ms, rep.push_ms, rep.h2d_ms, rep.d2h_ms, rep.duplex_ms,
            rep.host_ms, rep.alloc_ms) == (1., 2., 3., 4., 5., 6., 0.5)
    assert (rep.pull_gbps, rep.push_gbps, rep.h2d_gbps, rep.d2h_gbps,
            rep.duplex_pull_gbps, rep.duplex_push_gbps) == (
                11., 12., 13., 14., 15., 16.)

    c.n_bad = 40  # only 16 records are carried
    assert len(attest.HostLinkReport.from_c(c).bad) == 16

    c.n_bad, c.mismatch_words, c.first_bad_offset, c.ok = 0, 0, NO_OFFSET, 1
    clean = attest.HostLinkReport.from_c(c)
    assert clean.first_bad_offset is None and clean.bad == []
    assert clean.ok is True

    c.bytes_tested, c.passes, c.ok = 0, 0, 0
    c.error = b"allocated 0 of 8 MiB pinned host, 0 of 8 MiB device"
    failed = attest.HostLinkReport.from_c(c)
    assert failed.ok is False and failed.bytes_tested == 0
    assert failed.error.startswith("allocated 0 of 8 MiB")


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


def _march_report(mib=8):
    return attest.HbmMarchReport(
        device=3, bytes_requested=mib << 20, bytes_tested=mib << 20,
        chunk_bytes=mib << 20, origin=0, chunks=1, passes=4,
        mismatch_words=0, first_bad_offset=None, bad=[], fill_ms=1.0,
        flip_ms=1.0, scrub_ms=1.0, zero_ms=1.0, alloc_ms=1.0, gbps=3456.7,
        beyond_cache=False, scrubbed=True, ok=True,
    )


def _link_report(mib=64, **over):
    base = dict(
        device=3, engine=0, bytes_requested=mib << 20, bytes_tested=mib << 20,
        origin=0, passes=5, mismatch_words=0, first_bad_offset=None, bad=[],
        pull_ms=1.0, push_ms=1.0, h2d_ms=1.0, d2h_ms=1.0, duplex_ms=1.0,
        pull_gbps=41.4, push_gbps=47.6, h2d_gbps=55.5, d2h_gbps=52.4,
        duplex_pull_gbps=30.0, duplex_push_gbps=30.0, host_ms=9.0,
        alloc_ms=1.0, ok=True,
    )
    base.update(over)
    return attest.HostLinkReport(**base)


@pytest.fixture
def hook(monkeypatch):
    """attest_device_by_bdf with the device-touching calls stubbed;
    yields the ordered list of calls."""
    calls = []

    def fake_main(idx, gemm_dim=1024):
        calls.append(("main", idx, gemm_dim))
        return _main_report()

    def fake_march(idx, mib, chunk_mib=1024, _origin=0, _poison_offset=-1,
                   _poison_after=0):
        calls.append(("march", idx, mib))
        return _march_report(mib)

    def fake_link(idx, mib, _origin=0, _poison_offset=-1, _poison_pass=0):
        calls.append(("link", idx, mib, _origin, _poison_offset))
        return _link_report(mib)

    monkeypatch.setattr(attest, "device_index_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(attest, "attest_device", fake_main)
    monkeypatch.setattr(attest, "hbm_march_report", fake_march)
    monkeypatch.setattr(attest, "host_link_report", fake_link)
    for var in ("CC_ATTEST_DEEP", "CC_ATTEST_GEMM_DIM", "CC_ATTEST_MXFP4",
                "CC_ATTEST_CU_SWEEP", "CC_ATTEST_HBM_MIB",
                "CC_ATTEST_HBM_CHUNK_MIB", "CC_ATTEST_HOST_MIB",
                "CC_ATTEST_HOST_MIN_GBPS"):
        monkeypatch.delenv(var, raising=False)
    return calls


DEVICE = SimpleNamespace(bdf="0000:05:00.0")


@pytest.mark.parametrize("value", [None, "", "0"])
def test_hook_unchanged_without_switch(hook, monkeypatch, value):
    if value is not None:
        monkeypatch.setenv("CC_ATTEST_HOST_MIB", value)
    monkeypatch.setenv("CC_ATTEST_HOST_MIN_GBPS", "1000")  # inert without it
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS
    assert hook == [("main", 3, 1024)]


def test_hook_adds_host_link_keys_after_the_march(hook, monkeypatch):
    monkeypatch.setenv("CC_ATTEST_HBM_MIB", "8")
    monkeypatch.setenv("CC_ATTEST_HOST_MIB", "64")
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS | HBM_KEYS | HOST_KEYS
    assert summary["host_link_mib"] == 64
    assert summary["host_link_gbps"] == [41, 48, 56, 52]
    assert summary["host_link_ok"] is True
    assert hook == [("main", 3, 1024), ("march", 3, 8), ("link", 3, 64, 0, -1)]


def test_hook_host_link_alone(hook, monkeypatch):
    monkeypatch.setenv("CC_ATTEST_HOST_MIB", "8")
    summary = attest.attest_device_by_bdf(DEVICE)
    assert set(summary) == BASE_KEYS | HOST_KEYS
    assert hook == [("main", 3, 1024), ("link", 3, 8, 0, -1)]


def test_hook_propagates_bad_word(hook, monkeypatch):
    monkeypatch.setattr(
        attest, "host_link_report",
        lambda idx, mib, _origin=0, _poison_offset=-1, _poison_pass=0:
        _link_report(mib, mismatch_words=3, first_bad_offset=0x2ffffc,
                     bad=[(0x2ffffc, 0x12345678, 0x12345679, 4)], ok=False),
    )
    monkeypatch.setenv("CC_ATTEST_HOST_MIB", "8")
    with pytest.raises(attest.AttestationError) as err:
        attest.attest_device_by_bdf(DEVICE)
    msg = str(err.value)
    assert "0x2ffffc" in msg and "3 wrong word" in msg
    assert "pass 4 (d2h)" in msg and "0x00000001" in msg


def test_hook_propagates_short_allocation(hook, monkeypatch):
    text = "allocated 0 of 1024 MiB pinned host, 0 of 1024 MiB device"
    monkeypatch.setattr(
        attest, "host_link_report",
        lambda idx, mib, _origin=0, _poison_offset=-1, _poison_pass=0:
        _link_report(mib, bytes_tested=0, passes=0, ok=False, error=text),
    )
    monkeypatch.setenv("CC_ATTEST_HOST_MIB", "1024")
    with pytest.raises(attest.AttestationError, match=text):
        attest.attest_device_by_bdf(DEVICE)


@pytest.mark.parametrize("slow", ["h2d_gbps", "d2h_gbps"])
def test_hook_min_gbps_refuses_a_slow_copy_path(hook, monkeypatch, slow):
    monkeypatch.setattr(
        attest, "host_link_report",
        lambda idx, mib, _origin=0, _poison_offset=-1, _poison_pass=0:
        _link_report(mib, **{slow: 3.9}),
    )
    monkeypatch.setenv("CC_ATTEST_HOST_MIB", "64")
    assert attest.attest_device_by_bdf(DEVICE)["host_link_ok"] is True
    monkeypatch.setenv("CC_ATTEST_HOST_MIN_GBPS", "3.5")
    assert attest.attest_device_by_bdf(DEVICE)["host_link_ok"] is True
    monkeypatch.setenv("CC_ATTEST_HOST_MIN_GBPS", "20")
    with pytest.raises(attest.AttestationError,
                       match="CC_ATTEST_HOST_MIN_GBPS=20"):
        attest.attest_device_by_bdf(DEVICE)


def test_doctor_collect_gains_a_trailing_keyword():
    import inspect

    from k8s_cc_manager_amd.doctor import collect

    params = inspect.signature(collect).parameters
    assert list(params)[:4] == ["run_attest", "gemm_dim", "cu_sweep",
                                "hbm_march_mib"]
    assert params["host_link_mib"].default == 0
