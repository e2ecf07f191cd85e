"""bench.py's plain run: the headline line only (the other legs are behind
--full), --steps honoured, and --dump-outputs writing the last timed step's
rows as .npy files that agree with each other and with the line."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("selfcheck", "parity_sample_ok", "fresh_publishes_per_s", "dense_csr", "two_in_flight", "latency_sweep",
             "p99_batch_ms", "coalesce", "e2e", "cpu_baseline", "c1", "c5")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    n, out = 20_000, tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--topics", str(n), "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "publishes/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u32" and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(n / (1e-3 * d["ms_per_step"]), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in d]

    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(files) == {"totals", "row_counts", "sample_rows", "sample_row_offsets", "sample_filter_ids"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64_000_000
    cnt, rows, offs = files["row_counts"], files["sample_rows"].astype(np.int64), files["sample_row_offsets"]
    assert files["totals"].tolist() == [n, d["matches_per_step"]]
    assert cnt.shape == (n,) and cnt.sum(dtype=np.float64) == d["matches_per_step"]
    assert len(rows) == n and (np.diff(rows) > 0).all()             # n < the sample size: every row
    assert np.array_equal(np.diff(offs), cnt[rows]) and offs[0] == 0
    assert len(files["sample_filter_ids"]) == offs[-1]
