"""bench.py's plain run and --dump-outputs: a plain run times the headline steps and nothing else (the rest is --full), and
--dump-outputs DIR writes what the last timed step computed, the same from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
DUMPED = ("stats", "histogram", "sample_keys", "sample_counts")


def test_bench_options_are_checked_before_any_work():
    """--full and --dump-outputs are offered; a run that could not honour --steps or --dump-outputs is refused by the argument
    parser (exit 2), before torch or the library is loaded."""
    h = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    for bad in (["--steps", "0"], ["--group", "2", "--dump-outputs", "x"], ["--hg", "--dump-outputs", "x"]):
        p = subprocess.run([sys.executable, BENCH] + bad, capture_output=True, text=True, timeout=60, cwd=ROOT)
        assert p.returncode == 2 and "error:" in p.stderr, (bad, p.stderr[-500:])


def _plain_run(tmp_path, tag):
    out_dir = tmp_path / tag
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", "2000000",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, BENCH_FULL_PATH=str(tmp_path / f"{tag}_full.json")))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {n: np.load(out_dir / f"{n}.npy") for n in DUMPED}, out_dir


@pytest.mark.gpu
def test_plain_bench_run_times_the_headline_alone_and_dumps_its_outputs(tmp_path):
    d, got, out_dir = _plain_run(tmp_path, "a")
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(d)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert not {"verify", "cpu_baseline", "end_to_end", "configs", "cli", "unhinted"} & set(d), sorted(d)
    assert sum(f.stat().st_size for f in out_dir.iterdir()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    kmers, distinct = got["stats"]
    assert kmers == d["config"]["kmers_per_step_per_gpu"] and distinct == d["config"]["distinct_per_gpu"]
    hist = got["histogram"]
    assert hist.ndim == 2 and hist.shape[1] == 2 and (hist[:, 0] * hist[:, 1]).sum() == kmers and hist[:, 1].sum() == distinct
    keys, counts = got["sample_keys"], got["sample_counts"]
    assert keys.shape == (counts.size, 2) and counts.size > 1000
    assert (counts >= 1).all()     # every sampled key was read from the counted reads
    # the same arguments give the same inputs, so a second run writes the same outputs
    _, again, _ = _plain_run(tmp_path, "b")
    for n in DUMPED:
        assert np.array_equal(got[n], again[n]), n
