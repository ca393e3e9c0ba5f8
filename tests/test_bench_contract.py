"""bench.py contract: runs on CPU (mock tier) and emits the JSON line."""

import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_bench_cpu_mock(tmp_path):
    out = tmp_path / "bench.json"
    proc = subprocess.run(
        [
            sys.executable,
            str(REPO / "bench.py"),
            "--mock",
            "--gpus",
            "2",
            "--steps",
            "3",
            "--warmup",
            "1",
            "--json-out",
            str(out),
        ],
        capture_output=True,
        text=True,
        timeout=240,
        cwd=REPO,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    line = out.read_text().strip()
    result = json.loads(line)
    assert result["metric"] == "reconcile_gpus_per_sec"
    assert result["n_gpus"] == 2
    assert result["steps"] == 3
    assert result["warmup"] == 1
    assert result["value"] > 0
    assert result["higher_is_better"] is True
    assert result["scaling"] == "weak"
    assert result["data"] == "synthetic"
    assert result["config"]["model"] == "cc-mode-transition"
    assert result["config"]["eviction"] is True
    # the stdout JSON line is parseable too
    json_lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert json_lines and json.loads(json_lines[-1])["value"] > 0
    # a plain run reports the headline only: no per-phase breakdown
    assert result["ms_per_step"] > 0
    assert "phase_ms_mean" not in proc.stderr


def _run_inprocess(argv, capsys):
    import bench  # the repository root is on sys.path (conftest.py)

    assert bench.main(argv) == 0
    return capsys.readouterr()


def test_dump_outputs_mock(tmp_path, capsys):
    """--dump-outputs writes the last timed step's results as float64
    .npy files, identical from run to run."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        _run_inprocess(
            ["--mock", "--gpus", "2", "--steps", "2", "--warmup", "1",
             "--dump-outputs", str(d)],
            capsys,
        )
        files = sorted(p.name for p in d.iterdir())
        assert files == ["device_modes.npy", "node_labels.npy"]
        dumps.append({f: np.load(d / f) for f in files})
    a, b = dumps
    for f in a:
        assert a[f].dtype == np.float64
        assert np.array_equal(a[f], b[f])
    # steps 0..2 alternate on/off/on: the last timed step left CC on,
    # fabric off, labels on/true, node uncordoned
    assert a["device_modes.npy"].tolist() == [[1.0, 0.0], [1.0, 0.0]]
    assert a["node_labels.npy"].tolist() == [1.0, 2.0, 0.0]

    # one step fewer ends on "off": --steps really sets the step count
    d = tmp_path / "c"
    _run_inprocess(
        ["--mock", "--gpus", "1", "--steps", "1", "--warmup", "1",
         "--dump-outputs", str(d)],
        capsys,
    )
    assert np.load(d / "device_modes.npy").tolist() == [[0.0, 0.0]]
    assert np.load(d / "node_labels.npy").tolist() == [0.0, 1.0, 0.0]


def test_full_adds_phase_breakdown(capsys):
    """--full carries everything beyond the headline figure."""
    cap = _run_inprocess(
        ["--mock", "--steps", "2", "--warmup", "1", "--full"], capsys
    )
    result = json.loads(
        [l for l in cap.out.splitlines() if l.startswith("{")][-1]
    )
    assert result["metric"] == "reconcile_gpus_per_sec"
    assert result["steps"] == 2 and result["ms_per_step"] > 0
    phase = json.loads(
        [l for l in cap.err.splitlines() if l.startswith('{"phase_ms_mean"')][-1]
    )
    assert phase["phase_ms_mean"] and phase["step_ms"] > 0
