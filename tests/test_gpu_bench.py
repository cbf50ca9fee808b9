"""bench.py end to end on one GPU at a small size: a plain run reports the headline alone and can dump the
last timed step's outputs; `--full` adds the sections that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_em", "hbm_headline_contract", "cpu_baseline", "string_rates", "em_at_scale",
             "cfg5_columns", "exact_cells_per_column")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--records", "20000"] + args,
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_outputs(tmp_path):
    d = str(tmp_path / "out")
    line = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", d])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"] == "fp64"
    pairs = line["config"]["candidate_pairs"]
    assert pairs > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(pairs / (line["ms_per_step"] / 1e3), rel=1e-12)
    assert not [k for k in FULL_ONLY if k in line] and "score" not in line["breakdown_ms"]
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert set(got) == {"em_stats", "lambda", "m_probabilities", "u_probabilities", "gammas_sample",
                        "gammas_sample_rows"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    K = line["config"]["comparison_columns"]
    assert got["gammas_sample"].shape == (min(pairs, 1 << 20), K)
    assert got["em_stats"][1] == pairs  # the E+M iteration saw every pair
    assert 0 < got["lambda"][0] < 1
    g = got["gammas_sample"]
    assert (g >= -1).all() and (g <= 2).all() and (g == np.round(g)).all()


def test_full_run_adds_its_sections():
    line = _bench(["--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "0.3", "--em-scale", "2",
                   "--cfg5-steps", "1"])
    assert line["full"] is True and line["steps"] == 2 and line["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k not in line]
    assert line["breakdown_ms"]["score"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["em_at_scale"]["pairs"] == 2 * line["config"]["candidate_pairs"]
    assert line["cfg5_columns"]["steps"] == 1 and line["cfg5_columns"]["ms_per_step"] > 0
