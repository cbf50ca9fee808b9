"""Merging the shards' clusters on the device against the host recipe it replaces, at cfg2 (1 M records, ~46 M pairs).

The pairs are scored with the initial parameters and kept when match_probability > 0.9.  The pair set is cut into 8
ordinal shards, held by 8 jobs in this one process (shard=(s, 8)); every shard's components are labelled on its own.
Then, into shard 0's components:

(a) spk_components_merge with the other 7 shards' labels as a [7, n] device tensor (what an RCCL all-gather leaves),
    and the same with a host array (what a gloo all-gather leaves: the upload is inside the call);
(b) the recipe DESIGN.md gave before: spk_components_copy of the labels, the non-trivial (v, label[v]) pairs in numpy,
    (all-gather of the ragged lists: not timed, the other shards' lists are made outside the clock), then
    spk_components_edges over the concatenated list;
(c) for scale, spk_components of the unsharded job.

Wall times around the calls, medians of `reps` runs after one warm-up, the forms alternating inside every repetition;
device milliseconds from the *_info calls (HIP events) where there is one.  The all-gather itself is in neither form:
its 8-rank RCCL time is not measured here (one GPU).

    python tools/ab_cluster_merge.py [reps]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.frames import ExpectationFrame, GammaFrame  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
SHARDS = 8
cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols]
params = Params(cfg_settings(2), AmdSession(0))
st = params.settings
lam, probs = params.params["λ"], params._level_probabilities()
cond = "match_probability > 0.9"
print(f"cfg2: {len(df)} records, condition {cond}, {SHARDS} ordinal shards, {reps} runs after a warm-up", flush=True)


def selected_job(shard):
    job = Job("dedupe_only", [df], "unique_id", 0, shard=shard)
    job.ctx.enable_timing(True)
    job.block(st["blocking_rules"])
    f = ExpectationFrame(GammaFrame(job, st), st, lam, probs).filter(cond)
    return job, f, f._select()


def med(xs):
    return float(np.median(xs))


# (c) the unsharded job
job, f, kept = selected_job((0, 1))
n = sum(len(t) for t in job.inputs)
wall, dev = [], []
for i in range(reps + 1):
    t0 = time.perf_counter()
    _, whole_clusters, whole_rounds = job.ctx.components()
    t1 = time.perf_counter()
    if i:
        wall.append((t1 - t0) * 1e3)
        dev.append(job.ctx.components_info()[3])
want = job.ctx.components_copy(0, n)
print(f"unsharded: {job.n_pairs} pairs, {kept} kept, {whole_clusters} clusters, rounds {whole_rounds}; spk_components "
      f"wall {med(wall):.3f} ms, device {med(dev):.3f} ms", flush=True)
del job, f

# the shards
labels, jobs = [], []
for s in range(SHARDS):
    job, f, kept = selected_job((s, SHARDS))
    _, n_clusters, rounds = job.ctx.components()
    labels.append(job.ctx.components_copy(0, n))
    print(f"shard {s}: {job.n_pairs} pairs, {kept} kept, {n_clusters} clusters, rounds {rounds}", flush=True)
    if s == 0:
        jobs.append((job, f))  # shard 0 stays: the merges go into its components
    del job, f
ctx = jobs[0][0].ctx
peers_host = np.stack(labels[1:])
peers_dev = torch.from_numpy(peers_host.view(np.int32)).to("cuda:0")
torch.cuda.synchronize()
print(f"peer labels: {peers_host.shape[0]} x {peers_host.shape[1]} uint32 = {peers_host.nbytes / 1e6:.1f} MB", flush=True)


def nontrivial(lab):
    v = np.flatnonzero(lab != np.arange(len(lab), dtype=np.uint32)).astype(np.uint32)
    return v, lab[v]


others = [nontrivial(lab) for lab in labels[1:]]  # made by the other ranks, outside this rank's clock
t = {k: [] for k in ("merge_device", "merge_device_ms", "merge_host", "merge_host_ms", "recipe", "recipe_copy",
                     "recipe_numpy", "recipe_edges", "recipe_edges_ms")}
rounds = {}
results = {}
for i in range(reps + 1):
    order = ("merge_device", "recipe", "merge_host") if i % 2 else ("recipe", "merge_host", "merge_device")
    for form in order:
        ctx.components()  # shard 0's own components again: every form starts from them
        base_ms = ctx.components_info()[3]
        t0 = time.perf_counter()
        if form == "recipe":
            lab0 = ctx.components_copy(0, n)
            t1 = time.perf_counter()
            mine = nontrivial(lab0)
            u = np.concatenate([mine[0]] + [o[0] for o in others])
            v = np.concatenate([mine[1]] + [o[1] for o in others])
            t2 = time.perf_counter()
            n_clusters, r = ctx.components_edges(n, u, v)
            t3 = time.perf_counter()
            if i:
                t["recipe"].append((t3 - t0) * 1e3)
                t["recipe_copy"].append((t1 - t0) * 1e3)
                t["recipe_numpy"].append((t2 - t1) * 1e3)
                t["recipe_edges"].append((t3 - t2) * 1e3)
                t["recipe_edges_ms"].append(ctx.components_info()[3])
            rounds["recipe"] = (r, len(u))
        else:
            n_clusters, r = ctx.components_merge(peers_dev if form == "merge_device" else peers_host)
            t1 = time.perf_counter()
            if i:
                t[form].append((t1 - t0) * 1e3)
                t[form + "_ms"].append(ctx.components_info()[3] - base_ms)
            rounds[form] = r
        results[form] = (int(n_clusters), ctx.components_copy(0, n))

for form, (n_clusters, got) in results.items():
    print(f"{form}: {n_clusters} clusters, labels {'equal to' if np.array_equal(got, want) else 'DIFFER from'} the "
          f"unsharded job's", flush=True)
print(f"(a) spk_components_merge, 7 peers on the device: wall {med(t['merge_device']):.3f} ms, device "
      f"{med(t['merge_device_ms']):.3f} ms, rounds {rounds['merge_device']}")
print(f"(a) spk_components_merge, 7 peers from the host (upload inside): wall {med(t['merge_host']):.3f} ms, device "
      f"{med(t['merge_host_ms']):.3f} ms, rounds {rounds['merge_host']}")
print(f"(b) recipe: wall {med(t['recipe']):.3f} ms = spk_components_copy {med(t['recipe_copy']):.3f} + numpy "
      f"{med(t['recipe_numpy']):.3f} + spk_components_edges {med(t['recipe_edges']):.3f} (device "
      f"{med(t['recipe_edges_ms']):.3f} ms, rounds {rounds['recipe'][0]}, {rounds['recipe'][1]} edges); the ragged "
      f"all-gather is not in it")
print(f"recipe / merge on the device, wall: {med(t['recipe']) / med(t['merge_device']):.2f}; recipe / merge from the "
      f"host: {med(t['recipe']) / med(t['merge_host']):.2f}")
print("not measured: the all-gather (8-rank RCCL wall time needs 8 GPUs), and the 100 M-record case")
