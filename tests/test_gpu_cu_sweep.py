"""Compute-unit sweep on a real MI355X: the VALU golden images against
a host evaluation of the generator, full and repeatable coverage of
every SIMD of every CU, detection and localisation of a poisoned unit,
refusal of out-of-range rounds, and the opt-in attestor hook.

Generator (docs/KERNELS.md, "Compute-unit sweep"): element (op, which,
round r, row, k) has index (b + k s) % 11 into VALUES, with
b = (3 row + 5 r + 2 op + 4 which) % 11 and s = 1 + ((row >> 2) + r) % 10;
scale byte (op, which, r, row, kb) is 126 + (x + (x >> 3)) % 3 with
x = (row + 1)(2 r + 3) + 5 kb + 7 which + op."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X"),
]

VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, -0.5, -1.0, -1.5, -2.0, -3.0]
# op -> (rows of A and of B, K, scaled)
SHAPES = {0: (32, 16, False), 1: (16, 32, False), 2: (32, 64, True),
          3: (32, 64, True)}


@pytest.fixture(scope="module")
def attest():
    from k8s_cc_manager_amd.ops import attest as a

    assert a.probe_available()
    return a


def host_operand(op, which, r):
    """Dequantised operand of one round, float64 [rows, K]."""
    rows, k_dim, scaled = SHAPES[op]
    row = torch.arange(rows)[:, None]
    k = torch.arange(k_dim)[None, :]
    b = (3 * row + 5 * r + 2 * op + 4 * which) % 11
    s = 1 + ((row >> 2) + r) % 10
    vals = torch.tensor(VALUES, dtype=torch.float64)[(b + k * s) % 11]
    if scaled:
        kb = torch.arange(k_dim // 32)[None, :]
        x = (row + 1) * (2 * r + 3) + 5 * kb + 7 * which + op
        byte = 126 + (x + (x >> 3)) % 3
        scale = 2.0 ** (byte.to(torch.float64) - 127.0)
        vals = vals * scale.repeat_interleave(32, dim=1)
    return vals


def host_gold64(rounds):
    """The four C images, row-major and concatenated, float64."""
    images = []
    for op in range(4):
        c = sum(host_operand(op, 0, r) @ host_operand(op, 1, r).t()
                for r in range(rounds))
        images.append(c.reshape(-1))
    return torch.cat(images)


def assert_clean(attest, rep):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert rep.ok, rep
    assert rep.units_seen == rep.units_expected == 4 * rep.cu_count
    assert rep.cus_seen == rep.cu_count == cus
    assert rep.units_failed == 0 and rep.failed_units == []
    assert rep.mfma_failures == 0 and rep.lds_failures == 0
    assert 1 <= rep.launches <= 4
    assert len(attest.cu_sweep_units(0)) == rep.units_seen


@pytest.mark.parametrize("rounds", [1, 4, 32])
def test_gold_matches_host_generator(attest, rounds):
    gold = torch.tensor(attest.cu_sweep_gold(0, rounds), dtype=torch.float32)
    ref = host_gold64(rounds)
    assert gold.shape == ref.shape == (3328,)
    assert ref.abs().max() > 0
    for op, lo, hi in ((0, 0, 1024), (1, 1024, 1280), (2, 1280, 2304),
                       (3, 2304, 3328)):
        diff = (gold[lo:hi].double() - ref[lo:hi]).abs().max().item()
        print(f"rounds {rounds} op {op}: max |gold - host| = {diff}")
    assert torch.equal(gold, ref.float())


def test_exact_at_the_rounds_cap(attest):
    """At CU_SWEEP_MAX_ROUNDS the partial sums are the largest the
    exactness argument allows (multiples of 2^-4 below 2^20): the golden
    images still equal the host's and every unit still agrees bitwise."""
    cap = attest.CU_SWEEP_MAX_ROUNDS
    gold = torch.tensor(attest.cu_sweep_gold(0, cap), dtype=torch.float32)
    ref = host_gold64(cap)
    assert ref.abs().max() < 2.0 ** 20
    assert torch.equal(gold, ref.float())
    rep = attest.sweep_compute_units(0, rounds=cap)
    assert rep.rounds == cap
    assert_clean(attest, rep)


def test_full_coverage_clean(attest):
    rep = attest.sweep_compute_units(0)
    print(f"launches {rep.launches}, sweep_ms {rep.sweep_ms:.3f}, "
          f"units {rep.units_seen}/{rep.units_expected}, cus {rep.cus_seen}, "
          f"xccs {rep.xccs_seen}")
    assert rep.rounds == 32
    assert_clean(attest, rep)
    hits = attest.cu_sweep_hits(0)
    # 4 blocks of 16 waves per CU and launch, wherever they landed
    assert sum(hits.values()) == 64 * rep.cu_count * rep.launches


def test_repeatable(attest):
    attest.sweep_compute_units(0)
    seen = []
    for _ in range(5):
        rep = attest.sweep_compute_units(0)
        assert_clean(attest, rep)
        assert rep.gold_ms == 0.0  # cached golden images
        seen.append(tuple(attest.cu_sweep_units(0)))
    assert len(set(seen)) == 1


def test_poisoned_unit_is_detected_and_localised(attest):
    assert_clean(attest, attest.sweep_compute_units(0))
    units = attest.cu_sweep_units(0)  # ascending
    key = units[len(units) // 2]
    unit = attest.decode_unit(key)

    rep = attest.cu_sweep_report(0, _poison_key=key)
    assert not rep.ok
    assert rep.units_failed == 1
    assert rep.failed_units == [unit]
    assert rep.mfma_failures > 0 and rep.lds_failures == 0
    assert rep.units_seen == rep.units_expected  # coverage itself is whole

    with pytest.raises(attest.AttestationError) as err:
        attest.sweep_compute_units(0, _poison_key=key)
    assert attest.unit_name(unit) in str(err.value)

    assert_clean(attest, attest.sweep_compute_units(0))  # nothing sticks

    unseen = max(set(range(16384)) - set(units))
    assert_clean(attest, attest.sweep_compute_units(0, _poison_key=unseen))


def test_rounds_refusal_launches_nothing(attest):
    assert_clean(attest, attest.sweep_compute_units(0))
    before = attest.cu_sweep_hits(0)
    assert before
    for rounds in (0, attest.CU_SWEEP_MAX_ROUNDS + 1):
        with pytest.raises(attest.AttestationError, match=r"rc=-2$"):
            attest.sweep_compute_units(0, rounds=rounds)
        with pytest.raises(attest.AttestationError, match=r"rc=-2$"):
            attest.cu_sweep_gold(0, rounds)
    assert attest.cu_sweep_hits(0) == before


def test_neighbouring_legs_unaffected(attest):
    assert attest.attest_device(0, 256).ok
    assert attest.attest_mxfp4(0, 256).ok
    assert_clean(attest, attest.sweep_compute_units(0))
    assert attest.attest_device(0, 256).ok
    assert attest.attest_mxfp4(0, 256).ok


def test_attestor_hook_runs_sweep(attest, monkeypatch):
    """CC_ATTEST_CU_SWEEP=1 through the real attestor hook on device 0."""
    from k8s_cc_manager_amd.device.shadow import ShadowBackend

    devices, _ = ShadowBackend(device_indices=[0]).find_devices()
    monkeypatch.setenv("CC_ATTEST_GEMM_DIM", "512")
    for var in ("CC_ATTEST_DEEP", "CC_ATTEST_MXFP4", "CC_ATTEST_CU_SWEEP"):
        monkeypatch.delenv(var, raising=False)
    plain = attest.attest_device_by_bdf(devices[0])
    assert "cu_sweep" not in plain and "cu_sweep_ok" not in plain
    monkeypatch.setenv("CC_ATTEST_CU_SWEEP", "1")
    summary = attest.attest_device_by_bdf(devices[0])
    assert set(summary) == set(plain) | {"cu_sweep", "cu_sweep_ok"}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert summary["cu_sweep"] == f"{4 * cus}/{4 * cus}"
    assert summary["cu_sweep_ok"] is True
