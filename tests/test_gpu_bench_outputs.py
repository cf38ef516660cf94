"""bench.py's plain run and --dump-outputs: the plain line carries the headline and nothing that needs runs of its own (those
are --full's), --steps sets the timed steps, and the last timed step's results are written as .npy files that are the same
from run to run with the same arguments (seeded inputs), so two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS, STEPS, B, K = 200_000, 4, 64, 100
ARGV = ["--docs", str(DOCS), "--vocab", "4096", "--steps", str(STEPS), "--warmup", "1"]


def _run_plain(dump_dir):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGV + ["--dump-outputs", str(dump_dir)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(dump_dir, n + ".npy")) for n in ("scores", "docs", "counts")}


@pytest.mark.gpu
@pytest.mark.timeout(700)
def test_plain_bench_line_and_dumped_outputs_are_reproducible(tmp_path):
    line, out = _run_plain(tmp_path / "a")
    assert line["steps"] == STEPS and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - B * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    assert line["unit"] == "queries/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("queries/sec")
    for side in ("p50_ms", "latency", "exact_scorer", "f32_stream_scorer", "pipelined_native", "other_kernels_ms_per_step",
                 "cpu_baseline", "lexicon_path", "headline_path", "other_configs"):
        assert side not in line, side
    assert out["scores"].dtype == np.float32 and out["scores"].shape == (B, K)
    assert out["docs"].dtype == np.float64 and out["docs"].shape == (B, K)
    assert out["counts"].dtype == np.float64 and out["counts"].shape == (B,)
    assert np.all(out["counts"] == K)
    d = out["docs"]
    assert np.all(d == np.floor(d)) and d.min() >= 0 and d.max() < DOCS
    assert all(len(set(row.tolist())) == K for row in d)          # a fused list names each document once
    assert np.all(np.isfinite(out["scores"])) and np.all(out["scores"] > 0)
    _, again = _run_plain(tmp_path / "b")
    for n in out:
        assert np.array_equal(out[n], again[n]), n
