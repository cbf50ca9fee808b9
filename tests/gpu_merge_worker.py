"""One rank of tests/test_gpu_components_merge.py's two-rank cases (run as a child process), and, imported, the same
frames from one process.

Every rank uses cuda:0 with the gloo backend, as tests/gpu_dist_worker.py does: the public API shards the pairs by
rank, and the cluster frames gather the ranks' labels (staged through the host under gloo) and merge them on the
device."""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

THRESHOLDS = [0.5, 0.99, 0.9]
COLS = ["unique_id", "first_name", "surname", "dob", "city", "email", "cluster"]


def _linker(mode):
    from splink_amd import Splink
    from splink_amd.session import AmdSession
    if mode == "link_tf":
        from conftest import load_golden
        g = load_golden("link_tf")
        return Splink(copy.deepcopy(g["settings_in"]), AmdSession(0), df_l=pd.DataFrame(g["df_l"]),
                      df_r=pd.DataFrame(g["df_r"]))
    from splink_amd.synthetic import cfg_settings, make_records
    df = make_records(2000, seed=3, surname_vocab=120, first_vocab=80, city_vocab=20)[COLS]
    rng = np.random.Generator(np.random.PCG64(3))
    df["cluster"] = df["cluster"].astype(np.float64)
    df.loc[rng.random(len(df)) < 0.05, "cluster"] = np.nan
    return Splink(cfg_settings(2, max_iterations=3), AmdSession(0), df=df)


def _plain(d):
    return {c: [None if (isinstance(v, float) and v != v) else (v.item() if hasattr(v, "item") else v)
                for v in d[c].tolist()] for c in d.columns}


def run(mode):
    """The cluster frames of one job through the public API, as plain lists; `sharded` tells whether this process
    held a shard (then metrics() and summary() must have been refused)."""
    df_e = _linker(mode).get_scored_comparisons()
    job = df_e.job
    one = df_e.clusters(0.9)
    sweep = df_e.clusters_at_thresholds(THRESHOLDS)
    out = {"sharded": bool(job.reduces_across_ranks()), "n_pairs": int(job.n_pairs),
           "clusters": _plain(one.toPandas()), "n_clusters": int(one.n_clusters),
           "sweep": _plain(sweep.toPandas()), "sweep_columns": list(sweep.toPandas().columns),
           "sweep_n_clusters": [int(sweep.at(t).n_clusters) for t in THRESHOLDS],
           "sweep_n_edges": [int(sweep._info[1][sweep._level_of(t)]) for t in THRESHOLDS],
           "truth_sweep": _plain(sweep.truth_table("cluster")), "truth_one": _plain(one.truth_table("cluster")),
           "truth_at": _plain(sweep.at(0.9).truth_table("cluster"))}
    refused = []
    for name, call in (("one.metrics", one.metrics), ("sweep.metrics", lambda: sweep.metrics(0.9)),
                       ("sweep.summary", sweep.summary), ("at.metrics", lambda: sweep.at(0.9).metrics())):
        try:
            call()
        except ValueError as e:
            assert "sharded job" in str(e), str(e)
            refused.append(name)
    out["refused"] = refused
    return out


def main():
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    out = run(sys.argv[2])
    with open(f"{sys.argv[1]}.{rank}", "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
