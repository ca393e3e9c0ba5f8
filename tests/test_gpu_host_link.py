"""Host-link leg on a real MI355X: one direction at a time on numpy
buffers against a numpy model of the pattern (both engines, sentinels on
each side), the five-pass leg clean and with a word poisoned in every
pass, the refusals, the neighbouring legs and the registration that must
not leak.

Pattern (docs/KERNELS.md, "Host link"): the HBM march's word at logical
byte address origin + k * 2^40 + offset for pass k, phase 0 in passes 1,
3, 5 and its complement in passes 2, 4."""

import functools

import pytest

np = pytest.importorskip("numpy")
torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X"),
]

MIB = 1 << 20
# The grid strides 1 MiB (64 blocks x 4 vectors x 256 lanes x 16 B), so
# the last size is three strides and three vectors: the stride loop and
# the tail both run.
SIZES = [16, 4096 + 16, 3 * MIB + 48]
# with the second origin w crosses 2^32 one MiB into the buffer
ORIGINS = [0, 2**34 - 2**20]
SHAPES = [(n, o) for n in SIZES for o in ORIGINS]
ENGINES = [0, 1]
GUARD = 16  # uint32 words of sentinel on each side: 64 bytes
SENTINEL = 0x5A17E4E1
W = 2 * MIB  # the leg's window in these tests


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a

    assert a.probe_available()
    return a


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
    """nbytes of uint32 in ordinary host memory between two sentinel
    runs, the buffer 64-byte aligned."""

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


def rate_and_ms(rep, check, engine):
    name = [["push", "pull"], ["d2h", "h2d"]][engine][check]
    return getattr(rep, name + "_gbps"), getattr(rep, name + "_ms")


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("nbytes,origin", SHAPES)
def test_write_direction_equals_host_model(attest, nbytes, origin, engine):
    g = Guarded(nbytes)
    for phase in (0, 1, 2):
        rep = attest.host_step(0, g.ptr, nbytes, origin, write=phase,
                               engine=engine)
        assert rep.ok and rep.mismatch_words == 0 and rep.bad == []
        assert rep.first_bad_offset is None and rep.engine == engine
        assert rep.bytes_tested == nbytes and rep.origin == origin
        gbps, ms = rate_and_ms(rep, False, engine)
        assert gbps > 0 and ms > 0
        assert np.array_equal(g.buf, model(nbytes, origin, phase)), phase
    g.assert_guards_intact()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("nbytes,origin", SHAPES)
def test_check_direction_finds_exactly_what_numpy_broke(attest, nbytes, origin,
                                                        engine):
    g = Guarded(nbytes)
    g.buf[:] = model(nbytes, origin, 0)
    rep = attest.host_step(0, g.ptr, nbytes, origin, check=0, engine=engine)
    assert rep.ok and rep.mismatch_words == 0 and rep.bad == []
    gbps, ms = rate_and_ms(rep, True, engine)
    assert gbps > 0 and ms > 0

    broken = corrupt(g, origin)
    before = g.buf.copy()
    rep = attest.host_step(0, g.ptr, nbytes, origin, check=0, engine=engine)
    assert not rep.ok
    assert rep.mismatch_words == len(broken) == len(rep.bad)
    assert rep.first_bad_offset == 0
    assert {b[:3] for b in rep.bad} == broken
    assert all(b[3] == 0 for b in rep.bad)  # bad_pass is the leg's
    assert np.array_equal(g.buf, before)  # the check direction writes nothing
    g.assert_guards_intact()


@pytest.mark.parametrize("engine", ENGINES)
def test_check_other_phases(attest, engine):
    nbytes, origin = SHAPES[3]
    g = Guarded(nbytes)
    for phase in (1, 2):
        g.buf[:] = model(nbytes, origin, phase)
        assert attest.host_step(0, g.ptr, nbytes, origin, check=phase,
                                engine=engine).ok
        rep = attest.host_step(0, g.ptr, nbytes, origin, check=0,
                               engine=engine)
        differ = np.count_nonzero(g.buf != model(nbytes, origin, 0))
        assert differ >= nbytes // 4 - 1
        assert rep.mismatch_words == differ and len(rep.bad) == 16


def assert_clean_leg(rep, mib, origin=0):
    assert rep.ok, rep
    assert rep.passes == 5
    assert rep.bytes_tested == rep.bytes_requested == mib * MIB
    assert rep.origin == origin
    assert rep.mismatch_words == 0 and rep.bad == []
    assert rep.first_bad_offset is None
    assert rep.error == ""
    assert min(rep.pull_ms, rep.push_ms, rep.h2d_ms, rep.d2h_ms,
               rep.duplex_ms, rep.host_ms) > 0
    assert min(rep.pull_gbps, rep.push_gbps, rep.h2d_gbps, rep.d2h_gbps,
               rep.duplex_pull_gbps, rep.duplex_push_gbps) > 0


@pytest.mark.parametrize("origin", ORIGINS)
def test_leg_clean(attest, origin):
    rep = attest.attest_host_link(0, W // MIB, _origin=origin)
    print(f"{W // MIB} MiB @ {origin:#x}: pull {rep.pull_gbps:.1f} push "
          f"{rep.push_gbps:.1f} h2d {rep.h2d_gbps:.1f} d2h {rep.d2h_gbps:.1f} "
          f"duplex {rep.duplex_pull_gbps:.1f}+{rep.duplex_push_gbps:.1f} GB/s, "
          f"host {rep.host_ms:.3f} alloc {rep.alloc_ms:.3f} ms")
    assert_clean_leg(rep, W // MIB, origin)


@pytest.mark.parametrize("poison_pass", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("offset", [0, W - 4, W // 2 - 4, W // 2])
def test_leg_poisoned(attest, poison_pass, offset):
    """One flipped bit in any pass, at the window's ends and on both
    sides of the middle (in pass 5 the lower half is pulled and checked
    by the kernel, the upper half pushed and checked by the CPU)."""
    rep = attest.host_link_report(0, W // MIB, _poison_offset=offset,
                                  _poison_pass=poison_pass)
    e = attest.host_link_word(offset, poison_pass)
    assert not rep.ok
    assert rep.passes == 5 and rep.bytes_tested == W
    assert rep.mismatch_words == 1
    assert rep.first_bad_offset == offset
    assert rep.bad == [(offset, e, e ^ 1, poison_pass)]

    with pytest.raises(attest.AttestationError) as err:
        attest.attest_host_link(0, W // MIB, _poison_offset=offset,
                                _poison_pass=poison_pass)
    assert f"offset {offset:#x} " in str(err.value)
    assert f"pass {poison_pass} " in str(err.value)


def test_leg_poisoned_at_the_other_origin(attest):
    origin = ORIGINS[1]
    for poison_pass in (1, 5):
        rep = attest.host_link_report(0, W // MIB, _origin=origin,
                                      _poison_offset=W // 2,
                                      _poison_pass=poison_pass)
        e = attest.host_link_word(W // 2, poison_pass, origin)
        assert rep.bad == [(W // 2, e, e ^ 1, poison_pass)]
    assert_clean_leg(attest.attest_host_link(0, W // MIB), W // MIB)


def test_refusals(attest):
    refused = pytest.raises(attest.AttestationError, match=r"rc=-2$")
    for kwargs in (
        dict(mib=0),
        dict(mib=1025),
        dict(mib=2, _origin=8),
        dict(mib=2, _origin=2**48 - 6 * 2**40 + 16),
        dict(mib=2, _poison_offset=2 * MIB, _poison_pass=1),
        dict(mib=2, _poison_offset=6, _poison_pass=1),
        dict(mib=2, _poison_offset=0, _poison_pass=0),
        dict(mib=2, _poison_offset=0, _poison_pass=6),
    ):
        with refused:
            attest.host_link_report(0, **kwargs)
    g = Guarded(64)
    for kwargs in (
        dict(nbytes=24, write=0),
        dict(nbytes=0, write=0),
        dict(nbytes=32),
        dict(nbytes=32, check=0, write=0),
        dict(nbytes=32, check=3),
        dict(nbytes=32, write=0, engine=2),
        dict(nbytes=32, write=0, origin=8),
    ):
        with refused:
            attest.host_step(0, g.ptr, **kwargs)
    with refused:
        attest.host_step(0, g.ptr + 4, 32, write=0)
    assert (g.whole == SENTINEL).all()  # nothing was launched
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    with refused:  # device memory is not host memory
        attest.host_step(0, t.data_ptr(), 64, write=0)
    assert not t.any()
    assert_clean_leg(attest.attest_host_link(0, 1), 1)


def test_neighbouring_legs_unaffected(attest):
    assert attest.attest_device(0, 256).ok
    assert_clean_leg(attest.attest_host_link(0, 2), 2)
    main = attest.attest_device(0, 256)
    assert main.ok and main.ref_ms == 0.0  # its cached reference survived
    assert attest.march_hbm(0, 8).ok
    attest.shutdown()
    assert_clean_leg(attest.attest_host_link(0, 2), 2)
    assert attest.attest_device(0, 256).ok


def test_registration_does_not_leak(attest):
    """host_step page-locks ordinary memory for the call only: the same
    buffer registers again, in either engine and after a mismatch."""
    nbytes = 4096 + 16
    g = Guarded(nbytes)
    for engine in (0, 1, 0):
        assert attest.host_step(0, g.ptr, nbytes, write=0, engine=engine).ok
        assert attest.host_step(0, g.ptr, nbytes, check=0, engine=engine).ok
        assert not attest.host_step(0, g.ptr, nbytes, check=1,
                                    engine=engine).ok
    g.assert_guards_intact()


def test_pinned_memory_is_used_as_it_is(attest):
    """A buffer that is already page-locked (torch's pinned allocator) is
    not registered again and stays pinned afterwards."""
    t = torch.empty(MIB // 4, dtype=torch.int32).pin_memory()
    for engine in ENGINES:
        assert attest.host_step(0, t.data_ptr(), MIB, write=1,
                                engine=engine).ok
        assert np.array_equal(t.numpy().view(np.uint32), model(MIB, 0, 1))
        assert attest.host_step(0, t.data_ptr(), MIB, check=1,
                                engine=engine).ok
    assert t.is_pinned()


def test_attestor_hook_runs_host_link(attest, monkeypatch):
    """CC_ATTEST_HOST_MIB through the real attestor hook on device 0."""
    from k8s_cc_manager_amd.device.shadow import ShadowBackend

    devices, _ = ShadowBackend(device_indices=[0]).find_devices()
    monkeypatch.setenv("CC_ATTEST_GEMM_DIM", "512")
    for var in ("CC_ATTEST_DEEP", "CC_ATTEST_MXFP4", "CC_ATTEST_CU_SWEEP",
                "CC_ATTEST_HBM_MIB", "CC_ATTEST_HBM_CHUNK_MIB",
                "CC_ATTEST_HOST_MIB", "CC_ATTEST_HOST_MIN_GBPS"):
        monkeypatch.delenv(var, raising=False)
    keys = {"host_link_mib", "host_link_gbps", "host_link_ok"}
    plain = attest.attest_device_by_bdf(devices[0])
    assert not keys & set(plain)
    monkeypatch.setenv("CC_ATTEST_HOST_MIB", "2")
    summary = attest.attest_device_by_bdf(devices[0])
    assert set(summary) == set(plain) | keys
    assert summary["host_link_mib"] == 2
    assert len(summary["host_link_gbps"]) == 4
    assert summary["host_link_ok"] is True
