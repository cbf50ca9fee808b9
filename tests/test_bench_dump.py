"""bench.dump_outputs on a stub job (host logic only, no GPU): the arrays `--dump-outputs DIR` writes, their
dtypes, the 64 MB cap, and the fixed sample of comparison vectors (in range, the same from call to call)."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

K = 6


def _vectors(start, count):
    rows = np.arange(start, start + count, dtype=np.int64)
    return ((rows[:, None] * 7 + np.arange(K)[None, :]) % 5 - 1).astype(np.int8)


class _StubCtx:
    def __init__(self, n_pairs):
        self.n_pairs = n_pairs

    def gammas_copy(self, k, start, count):
        assert k == K and 0 <= start and count >= 0 and start + count <= self.n_pairs
        return _vectors(start, count)


class _StubParams:
    params = {"λ": 0.25}

    def _level_probabilities(self):
        return [([0.1, 0.9], [0.8, 0.2])] * K


def _run(n_pairs):
    job = argparse.Namespace(ctx=_StubCtx(n_pairs), n_pairs=n_pairs)
    return argparse.Namespace(job=job, params=_StubParams(), names=[f"gamma_c{i}" for i in range(K)],
                              last_stats=np.arange(8, dtype=np.float64))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("n_pairs", [1000, bench.DUMP_RUNS * bench.DUMP_RUN_ROWS, 46_000_003])
def test_dump_outputs_arrays(tmp_path, n_pairs):
    d = str(tmp_path / "a" / "out")  # the directory is created
    bench.dump_outputs(d, _run(n_pairs))
    got = _load(d)
    assert set(got) == {"em_stats", "lambda", "m_probabilities", "u_probabilities", "gammas_sample",
                        "gammas_sample_rows"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 1000 * 1000
    assert np.array_equal(got["em_stats"], np.arange(8.0)) and got["lambda"].tolist() == [0.25]
    assert got["m_probabilities"].tolist() == [0.1, 0.9] * K and got["u_probabilities"].tolist() == [0.8, 0.2] * K
    rows = got["gammas_sample_rows"].astype(np.int64)
    n = min(n_pairs, bench.DUMP_RUNS * bench.DUMP_RUN_ROWS)
    assert rows.shape == (n,) and got["gammas_sample"].shape == (n, K)
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < n_pairs
    if n == n_pairs:
        assert np.array_equal(rows, np.arange(n_pairs))
    want = ((rows[:, None] * 7 + np.arange(K)[None, :]) % 5 - 1).astype(np.float32)
    assert np.array_equal(got["gammas_sample"], want)
    # the sample is fixed: a second dump of the same job holds the same arrays
    d2 = str(tmp_path / "b")
    bench.dump_outputs(d2, _run(n_pairs))
    again = _load(d2)
    assert all(np.array_equal(got[k], again[k]) for k in got)
