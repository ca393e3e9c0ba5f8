"""HBM march on a real MI355X: the step kernels on torch-owned buffers
against a numpy model of the pattern (fill, verify against corruption
made with torch, check-and-write), the four-pass leg clean and with a
poisoned word, the refusals, one window past the Infinity Cache, the
neighbouring legs and the opt-in attestor hook.

Pattern (docs/KERNELS.md, "HBM march"): logical word index
w = (origin + byte offset) / 4, lo = w mod 2^32, hi = w >> 32,
p = lo * 2654435769 + hi * 2246822519 + 0x5EED0001 mod 2^32; phase 0
holds p, phase 1 ~p, phase 2 zero. Every buffer under test is a slice of
a larger tensor with 64 sentinel bytes on each side."""

import functools

import pytest

np = pytest.importorskip("numpy")
torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X"),
]

MIB = 1 << 20
SIZES = [16, 4096 + 16, 3 * MIB + 48]
# with the second origin w crosses 2^32 one MiB into the buffer
ORIGINS = [0, 2**34 - 2**20]
SHAPES = [(n, o) for n in SIZES for o in ORIGINS]
GUARD = 16  # int32 words of sentinel on each side: 64 bytes
SENTINEL = 0x5A17E4E1


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
    """nbytes of int32 on the device between two sentinel runs."""

    def __init__(self, nbytes):
        self.n = nbytes // 4
        self.whole = torch.full((self.n + 2 * GUARD,), SENTINEL,
                                dtype=torch.int32, device="cuda")
        self.buf = self.whole[GUARD:GUARD + self.n]
        self.ptr = self.buf.data_ptr()
        assert self.ptr % 16 == 0

    def words(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def assert_guards_intact(self):
        whole = self.whole.cpu()
        assert (whole[:GUARD] == SENTINEL).all()
        assert (whole[GUARD + self.n:] == SENTINEL).all()


def corrupt(g, origin):
    """XOR up to 16 chosen words of a filled buffer with chosen masks;
    returns {(byte offset, expected, got)} for phase 0."""
    n = g.n
    picks = {0: 0x00000001, n - 1: 0x80000000,
             n // 3: 0x00010000, n // 2: 0xFFFFFFFF}
    edge = 2**32 - 1 - origin // 4  # the word at w = 2^32 - 1
    if 0 <= edge and edge + 1 < n:
        picks[edge] = 0x00000004
        picks[edge + 1] = 0x5A5A5A5A
    idx = sorted(picks)
    assert len(idx) <= 16
    masks = np.array([picks[i] for i in idx], dtype=np.uint32)
    g.buf[torch.tensor(idx, device="cuda")] ^= torch.from_numpy(
        masks.view(np.int32)).cuda()
    p = model(4 * n, origin, 0)
    return {(4 * i, int(p[i]), int(p[i] ^ m)) for i, m in zip(idx, masks)}


@pytest.mark.parametrize("nbytes,origin", SHAPES)
def test_fill_equals_host_model(attest, nbytes, origin):
    g = Guarded(nbytes)
    for phase in (0, 1, 2):
        rep = attest.hbm_step(0, g.ptr, nbytes, origin, check=-1, write=phase)
        assert rep.ok and rep.mismatch_words == 0
        assert rep.first_bad_offset is None and rep.bad == []
        assert rep.bytes_tested == nbytes and rep.origin == origin
        assert np.array_equal(g.words(), model(nbytes, origin, phase)), phase
    g.assert_guards_intact()


@pytest.mark.parametrize("nbytes,origin", SHAPES)
def test_verify_finds_exactly_what_torch_broke(attest, nbytes, origin):
    g = Guarded(nbytes)
    attest.hbm_step(0, g.ptr, nbytes, origin, write=0)
    assert attest.hbm_step(0, g.ptr, nbytes, origin, check=0).ok
    broken = corrupt(g, origin)
    before = g.words().copy()

    rep = attest.hbm_step(0, g.ptr, nbytes, origin, check=0)
    assert not rep.ok
    assert rep.mismatch_words == len(broken)
    assert rep.first_bad_offset == min(off for off, _, _ in broken) == 0
    assert {b[:3] for b in rep.bad} == broken
    assert len(rep.bad) == len(broken)
    assert all(b[3] == 0 for b in rep.bad)  # bad_pass is the leg's
    assert np.array_equal(g.words(), before)  # check-only writes nothing
    g.assert_guards_intact()


@pytest.mark.parametrize("nbytes,origin", SHAPES)
def test_wrong_origin_reports_every_word(attest, nbytes, origin):
    g = Guarded(nbytes)
    attest.hbm_step(0, g.ptr, nbytes, origin, write=0)
    rep = attest.hbm_step(0, g.ptr, nbytes, origin + 16, check=0)
    assert not rep.ok
    assert rep.mismatch_words == nbytes // 4
    assert rep.first_bad_offset == 0
    assert len(rep.bad) == min(16, nbytes // 4)
    p_here, p_there = model(nbytes, origin, 0), model(nbytes, origin + 16, 0)
    for off, expected, got, _ in rep.bad:
        assert expected == p_there[off // 4] and got == p_here[off // 4]
    g.assert_guards_intact()


@pytest.mark.parametrize("nbytes,origin", SHAPES)
def test_check_and_write(attest, nbytes, origin):
    g = Guarded(nbytes)
    attest.hbm_step(0, g.ptr, nbytes, origin, write=0)
    broken = corrupt(g, origin)

    rep = attest.hbm_step(0, g.ptr, nbytes, origin, check=0, write=1)
    assert rep.mismatch_words == len(broken)
    assert rep.first_bad_offset == 0
    assert {b[:3] for b in rep.bad} == broken
    # the write happens whether or not the compare matched
    assert np.array_equal(g.words(), model(nbytes, origin, 1))

    rep = attest.hbm_step(0, g.ptr, nbytes, origin, check=1, write=2)
    assert rep.ok and rep.mismatch_words == 0 and rep.bad == []
    assert not g.words().any()

    rep = attest.hbm_step(0, g.ptr, nbytes, origin, check=2)
    assert rep.ok and rep.first_bad_offset is None
    g.assert_guards_intact()


def assert_clean_leg(rep, mib, chunk_mib):
    assert rep.ok, rep
    assert rep.passes == 4
    assert rep.bytes_tested == rep.bytes_requested == mib * MIB
    assert rep.chunk_bytes == chunk_mib * MIB
    assert rep.chunks == -(-mib // chunk_mib)
    assert rep.mismatch_words == 0 and rep.bad == []
    assert rep.first_bad_offset is None
    assert rep.scrubbed
    assert rep.error == ""
    assert min(rep.fill_ms, rep.flip_ms, rep.scrub_ms, rep.zero_ms) > 0


@pytest.mark.parametrize("mib,chunks", [(8, 4), (5, 3)])
def test_leg_clean(attest, mib, chunks):
    rep = attest.march_hbm(0, mib, chunk_mib=2)
    print(f"{mib} MiB: fill {rep.fill_ms:.3f} flip {rep.flip_ms:.3f} scrub "
          f"{rep.scrub_ms:.3f} zero {rep.zero_ms:.3f} alloc {rep.alloc_ms:.3f} "
          f"ms, {rep.gbps:.0f} GB/s")
    assert_clean_leg(rep, mib, 2)
    assert rep.chunks == chunks
    assert not rep.beyond_cache


@pytest.mark.parametrize("poison_after", [1, 2, 3])
@pytest.mark.parametrize("offset", [0, 2 * MIB, 8 * MIB - 4])
def test_leg_poisoned(attest, poison_after, offset):
    rep = attest.hbm_march_report(0, 8, chunk_mib=2, _poison_offset=offset,
                                  _poison_after=poison_after)
    e = attest.hbm_pattern_word(offset // 4, poison_after - 1)
    assert not rep.ok
    assert rep.passes == 4 and rep.bytes_tested == 8 * MIB
    assert rep.mismatch_words == 1
    assert rep.first_bad_offset == offset
    assert rep.bad == [(offset, e, e ^ 1, poison_after + 1)]
    assert not rep.scrubbed

    with pytest.raises(attest.AttestationError) as err:
        attest.march_hbm(0, 8, chunk_mib=2, _poison_offset=offset,
                         _poison_after=poison_after)
    assert f"offset {offset:#x} " in str(err.value)
    assert f"pass {poison_after + 1}" in str(err.value)

    assert_clean_leg(attest.march_hbm(0, 8, chunk_mib=2), 8, 2)  # nothing sticks


def test_refusals(attest):
    refused = pytest.raises(attest.AttestationError, match=r"rc=-2$")
    for kwargs in (
        dict(mib=0),
        dict(mib=8, chunk_mib=0),
        dict(mib=8, chunk_mib=1025),
        dict(mib=8, _origin=8),
        dict(mib=8, _poison_offset=8 * MIB, _poison_after=1),
        dict(mib=8, _poison_offset=6, _poison_after=1),
        dict(mib=8, _poison_offset=0, _poison_after=4),
    ):
        with refused:
            attest.hbm_march_report(0, **kwargs)
    g = Guarded(64)
    with refused:
        attest.hbm_step(0, g.ptr, 24, write=0)
    with refused:
        attest.hbm_step(0, g.ptr, 32)
    with refused:
        attest.hbm_step(0, g.ptr, 32, check=3)
    with refused:
        attest.hbm_step(0, g.ptr + 4, 32, write=0)
    assert (g.whole.cpu() == SENTINEL).all()  # nothing was launched
    assert_clean_leg(attest.march_hbm(0, 8, chunk_mib=2), 8, 2)


def test_beyond_the_cache_once(attest):
    """512 MiB, twice the Infinity Cache: the smallest window at which
    beyond_cache flips."""
    rep = attest.march_hbm(0, 512)
    print(f"512 MiB: fill {rep.fill_ms:.3f} flip {rep.flip_ms:.3f} scrub "
          f"{rep.scrub_ms:.3f} zero {rep.zero_ms:.3f} alloc {rep.alloc_ms:.3f} "
          f"ms, {rep.gbps:.0f} GB/s")
    assert_clean_leg(rep, 512, 1024)
    assert rep.chunks == 1
    assert rep.beyond_cache


def test_neighbouring_legs_unaffected(attest):
    assert attest.attest_device(0, 256).ok
    assert attest.attest_mxfp4(0, 256).ok
    assert attest.sweep_compute_units(0).ok
    assert_clean_leg(attest.march_hbm(0, 8), 8, 1024)
    assert attest.attest_device(0, 256).ok
    assert attest.attest_mxfp4(0, 256).ok
    sweep = attest.sweep_compute_units(0)
    assert sweep.ok and sweep.gold_ms == 0.0  # its cache survived the march


def test_attestor_hook_runs_march(attest, monkeypatch):
    """CC_ATTEST_HBM_MIB through the real attestor hook on device 0."""
    from k8s_cc_manager_amd.device.shadow import ShadowBackend

    devices, _ = ShadowBackend(device_indices=[0]).find_devices()
    monkeypatch.setenv("CC_ATTEST_GEMM_DIM", "512")
    for var in ("CC_ATTEST_DEEP", "CC_ATTEST_MXFP4", "CC_ATTEST_CU_SWEEP",
                "CC_ATTEST_HBM_MIB", "CC_ATTEST_HBM_CHUNK_MIB"):
        monkeypatch.delenv(var, raising=False)
    keys = {"hbm_march_mib", "hbm_march_gbps", "hbm_march_ok", "hbm_scrubbed"}
    plain = attest.attest_device_by_bdf(devices[0])
    assert not keys & set(plain)
    monkeypatch.setenv("CC_ATTEST_HBM_MIB", "8")
    monkeypatch.setenv("CC_ATTEST_HBM_CHUNK_MIB", "2")
    summary = attest.attest_device_by_bdf(devices[0])
    assert set(summary) == set(plain) | keys
    assert summary["hbm_march_mib"] == 8
    assert summary["hbm_march_ok"] is True
    assert summary["hbm_scrubbed"] is True
