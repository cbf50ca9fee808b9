"""The comparison of a scored frame and an EM history with a reference golden, shared by
tests/test_gpu_parity.py and tests/test_gpu_residual.py."""
import math

import pandas as pd


def frame(d):
    return pd.DataFrame(d) if d else None


def rel_close(a, b, tol=1e-9):
    """Relative closeness; NULL (None) and NaN are the same missing value."""
    a = None if (isinstance(a, float) and math.isnan(a)) else a
    b = None if (isinstance(b, float) and math.isnan(b)) else b
    if a is None or b is None:
        return a is None and b is None
    return abs(a - b) <= tol * max(abs(a), abs(b), 1e-300)


def sort_like_golden(df):
    keys = [k for k in ("_source_table_l", "unique_id_l", "_source_table_r", "unique_id_r") if k in df.columns]
    rest = [c for c in df.columns if c.startswith("gamma_")]
    return df.sort_values(keys + rest, kind="mergesort").reset_index(drop=True)


def compare_frames(got: pd.DataFrame, exp: dict, columns):
    assert list(got.columns) == list(columns)
    got = sort_like_golden(got)
    for c in columns:
        gv, ev = got[c].tolist(), exp[c]
        assert len(gv) == len(ev), c
        for a, b in zip(gv, ev):
            if isinstance(b, float) or (isinstance(a, float) and not isinstance(b, str)):
                a = None if a is None else float(a)
                assert rel_close(a, b), (c, a, b)
            else:
                if isinstance(a, float) and math.isnan(a):
                    a = None
                assert a == b, (c, a, b)


def check_history(params, g):
    if not g["iterations"]:  # max_iterations = 0: the initial parameters, untouched
        assert params.param_history == []
        assert rel_close(params.params["λ"], g["initial"]["lambda"])
        return
    hist = params.param_history[1:] + [params.params]
    assert len(hist) == len(g["iterations"])
    for p, it in zip(hist, g["iterations"]):
        assert rel_close(p["λ"], it["lambda"])
        for gname, d in it["pi"].items():
            for i, (m, u) in enumerate(zip(d["m"], d["u"])):
                assert rel_close(p["π"][gname]["prob_dist_match"][f"level_{i}"]["probability"], m), (gname, i)
                assert rel_close(p["π"][gname]["prob_dist_non_match"][f"level_{i}"]["probability"], u), (gname, i)
