"""The clusters of a sharded job on the device (spk_components_merge, spk_components_sweep_merge): each part of a graph
is labelled on its own, the parts' labels are merged, and the result must be the union-find labels of all edges, bit
for bit.  Then the pipeline over three explicit shards in one process, and the public API on two gloo ranks."""
import ctypes
import json
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

import merge_common as M

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

PAD = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


@pytest.fixture(scope="module")
def ctx(amd):
    from splink_amd import _native as N
    return N.Context(0)


def part_labels(ctx, n, parts):
    """components_edges on every part: its labels, copied."""
    out = []
    for u, v in parts:
        ctx.components_edges(n, u, v)
        out.append(ctx.components_copy(0, n))
    return out


def peer_rows(labels, stride):
    """[P, stride] uint32: row p is labels[p], the padding 0xFFFFFFFF (never read: as an entry it would be invalid)."""
    rows = np.full((len(labels), stride), PAD, dtype=np.uint32)
    for p, lab in enumerate(labels):
        rows[p, :len(lab)] = lab
    return rows


def on_device(rows):
    import torch
    return torch.from_numpy(rows.view(np.int32)).to("cuda:0")


def merge_into_first(ctx, n, first, rows, want, device):
    """components_edges of the first part, then the merge of `rows`; every label against `want`."""
    u, v = first
    _, own_rounds = ctx.components_edges(n, u, v)
    n_clusters, rounds = ctx.components_merge(on_device(rows) if device else rows)
    got = ctx.components_copy(0, n)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert n_clusters == int(np.count_nonzero(want == np.arange(n, dtype=np.uint32)))
    assert 1 <= rounds <= M.ROUND_CAP
    assert ctx.components_info()[:3] == (n, len(u), own_rounds + rounds)
    return got, rounds


# ---- 1. the three graphs, dealt over 2, 3 and 8 parts ------------------------------------------------------------------
@pytest.mark.parametrize("how", M.DEALINGS)
@pytest.mark.parametrize("parts", M.PARTS)
@pytest.mark.parametrize("name", M.GRAPH_NAMES)
def test_merged_parts_equal_the_union_find(name, parts, how, ctx):
    n, _, _, want = M.graph(name)
    dealt = M.dealt(name, parts, how)
    labels = part_labels(ctx, n, dealt)
    assert any(not np.array_equal(lab, want) for lab in labels)  # no part alone has the answer
    rows = peer_rows(labels[1:], n)
    a, ra = merge_into_first(ctx, n, dealt[0], rows, want, device=False)
    b, rb = merge_into_first(ctx, n, dealt[0], rows, want, device=True)
    c, _ = merge_into_first(ctx, n, dealt[0], rows, want, device=False)  # a second run: the same bytes
    assert a.tobytes() == b.tobytes() == c.tobytes()
    print(f"{name} {parts} parts {how}: merge rounds {ra} (host peers), {rb} (device peers)")


# ---- 2. lane, wave and workgroup edges; every row alignment ------------------------------------------------------------
def _node_counts():
    return [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, "grid"]


@pytest.mark.parametrize("n_peers", [1, 3])
@pytest.mark.parametrize("n", _node_counts())
def test_lane_wave_and_workgroup_edges(n, n_peers, ctx):
    if n == "grid":  # one node past what the capped grid covers in one trip of a lane's loop
        import torch
        n = 8 * int(torch.cuda.get_device_properties(0).multi_processor_count) * 256 + 1
    rng = np.random.Generator(np.random.PCG64(n + n_peers))
    m = n // 2 if n < 5000 else 4096  # the big case: few edges, so that the host reference stays quick
    u = rng.integers(0, n, m).astype(np.uint32)
    v = rng.integers(0, n, m).astype(np.uint32)
    if n > 5000:
        u[:8], v[:8] = n - 1, rng.integers(0, n, 8)  # the last node, the one past the grid, is in a cluster
    want = M.union_find(n, u, v)
    part = np.arange(m) % (n_peers + 1)
    dealt = [(u[part == p], v[part == p]) for p in range(n_peers + 1)]
    labels = part_labels(ctx, n, dealt)
    for stride in (n, n + 1, n + 3, (n + 63) // 64 * 64):  # rows 1.. then start at every 4-byte alignment
        rows = peer_rows(labels[1:], stride)
        for device in (False, True):
            merge_into_first(ctx, n, dealt[0], rows, want, device)


# ---- 3. one call or many; a graph merged into itself ----------------------------------------------------------------
def test_one_call_equals_one_call_per_peer_and_self_merge_changes_nothing(ctx):
    n, _, _, want = M.graph("random")
    dealt = M.dealt("random", 3, "round_robin")
    labels = part_labels(ctx, n, dealt)
    both, _ = merge_into_first(ctx, n, dealt[0], peer_rows(labels[1:], n), want, device=False)
    ctx.components_edges(n, *dealt[0])
    first_clusters, _ = ctx.components_merge(labels[1])
    after_a = ctx.components_copy(0, n)
    assert not np.array_equal(after_a, want) and (after_a <= labels[0]).all() and (after_a <= labels[1]).all()
    n_clusters, _ = ctx.components_merge(on_device(labels[2].reshape(1, -1)))
    assert n_clusters < first_clusters
    assert ctx.components_copy(0, n).tobytes() == both.tobytes()
    # the merged labels into themselves, and this graph's own labels again: nothing changes, one quiet round
    for again in (both, labels[0], peer_rows([both, labels[1], labels[2]], n + 1)):
        assert ctx.components_merge(again) == (n_clusters, 1)
        assert ctx.components_copy(0, n).tobytes() == both.tobytes()


# ---- 4. invalid peers -------------------------------------------------------------------------------------------------
def test_invalid_peers_leave_no_components(ctx):
    n = 3000
    u = np.arange(0, n - 1, 2, dtype=np.uint32)
    good = np.arange(n, dtype=np.uint32)
    cases = []
    above = good.copy()
    above[5] = 6                      # greater than its own index
    cases.append(above.reshape(1, -1))
    beyond = good.copy()
    beyond[n - 1] = n                 # >= n_nodes
    cases.append(beyond.reshape(1, -1))
    huge = np.stack([good, good, good])
    huge[2, 2999] = 0xFFFFFFFF
    cases.append(huge)
    first = good.copy()
    first[0] = 1
    cases.append(first.reshape(1, -1))
    for rows in cases:
        for device in (False, True):
            ctx.components_edges(n, u, u + 1)
            with pytest.raises(ValueError, match="peer label"):
                ctx.components_merge(on_device(rows) if device else rows)
            assert ctx.components_info() == (-1, -1, -1, -1.0)
            with pytest.raises(RuntimeError, match="no components"):
                ctx.components_copy(0, 1)
    # a following valid call works
    want = M.union_find(n, u, u + 1)
    ctx.components_edges(n, u, u + 1)
    assert np.array_equal(ctx.components_copy(0, n), want)
    assert ctx.components_merge(good)[0] == int(np.count_nonzero(want == good))


# ---- 5. state ---------------------------------------------------------------------------------------------------------
def raw_merge(c, n_peers, rows, stride, level=None):
    N = sys.modules["splink_amd._native"]
    out_c, out_r = ctypes.c_int64(0), ctypes.c_int(0)
    args = [ctypes.c_int(n_peers), N._ptr(rows), ctypes.c_int64(stride), ctypes.c_int(0), ctypes.byref(out_c),
            ctypes.byref(out_r)]
    if level is None:
        return c._lib.spk_components_merge(c._h, *args)
    return c._lib.spk_components_sweep_merge(c._h, ctypes.c_int(level), *args)


def test_abi_states(amd):
    from splink_amd import _native as N
    from sweep_common import scores_for, thresholds_for
    c = N.Context(0)
    n, u, v, _ = M.graph("hub")
    rows = peer_rows([np.arange(n, dtype=np.uint32)] * 2, n)
    # nothing to merge into
    assert raw_merge(c, 1, rows, n) == N.SPK_E_STATE
    assert raw_merge(c, 1, rows, n, level=0) == N.SPK_E_STATE
    with pytest.raises(RuntimeError, match="no components"):
        c.components_merge(rows)
    with pytest.raises(RuntimeError, match="no components"):
        c.components_copy_device(on_device(rows[0]))
    # argument errors leave the components as they are
    c.components_edges(n, u, v)
    before = c.components_copy(0, n)
    big = np.zeros((N.COMPONENTS_MAX_PEERS + 1, 4), dtype=np.uint32)
    assert raw_merge(c, 0, rows, n) == N.SPK_E_INVALID
    assert raw_merge(c, N.COMPONENTS_MAX_PEERS + 1, big, n) == N.SPK_E_INVALID
    assert raw_merge(c, -1, rows, n) == N.SPK_E_INVALID
    assert raw_merge(c, 1, None, n) == N.SPK_E_INVALID
    assert raw_merge(c, 2, rows, n - 1) == N.SPK_E_INVALID  # stride < n_nodes
    with pytest.raises(ValueError, match="stride"):
        c.components_merge(rows[:, :n - 1])
    assert np.array_equal(c.components_copy(0, n), before)
    # the device copy, at odd offsets
    import torch
    out = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    c.components_copy_device(out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), before)
    c.components_copy_device(out[3:260], start=65)
    assert np.array_equal(out[3:260].cpu().numpy().view(np.uint32), before[65:65 + 257])
    with pytest.raises(ValueError):
        c.components_copy_device(out, start=1)
    with pytest.raises(ValueError):
        c.components_copy_device(out.cpu())
    # a sweep over two parts of the hub graph's scored edges: levels merged one by one
    L = 4
    level = M.emulation().random_levels(len(u), L, seed=L)
    thr, score = thresholds_for(L), scores_for(level, L)
    half = np.arange(len(u)) % 2 == 0
    want = M.emulation().union_find_levels(n, u, v, level, L)
    ids = (np.arange(n, dtype=np.int64) % 97) - 3
    c.components_sweep_edges(n, u, v, score, thr)
    whole_agreement = c.cluster_agreement(ids)
    whole_metrics = c.cluster_metrics(L - 1)
    c.components_sweep_edges(n, u[~half], v[~half], score[~half], thr)
    other = [c.components_sweep_copy(k, 0, n) for k in range(L)]
    e, clusters, rounds = c.components_sweep_edges(n, u[half], v[half], score[half], thr)
    assert c.cluster_metrics(0)[2] >= 1  # unmerged: the metrics work
    unmerged = [c.components_sweep_copy(k, 0, n) for k in range(L)]
    # spk_components_merge does not reach the sweep (nor the other way round)
    mine = half & (level < L)  # this half's edges of the last level (an edge of no level is in no sweep level)
    c.components_edges(n, u[mine], v[mine])
    c.components_merge(other[L - 1])
    assert np.array_equal(c.components_copy(0, n), want[L - 1])
    assert all(np.array_equal(c.components_sweep_copy(k, 0, n), unmerged[k]) for k in range(L))
    assert c.cluster_metrics(0)[2] >= 1
    for bad in (-1, L, L + 7):
        assert raw_merge(c, 1, other[0], n, level=bad) == N.SPK_E_INVALID
        with pytest.raises(ValueError, match="level"):
            c.components_sweep_merge(bad, other[0])
    assert raw_merge(c, 0, other[0], n, level=0) == N.SPK_E_INVALID
    assert raw_merge(c, 1, other[0], n - 1, level=0) == N.SPK_E_INVALID
    assert c.cluster_metrics(0)[2] >= 1  # refused merges do not mark the sweep
    for k in (2, 0, 3, 1):  # any order: the levels are independent
        n_clusters, r = c.components_sweep_merge(k, on_device(other[k].reshape(1, -1)) if k % 2 else other[k])
        assert np.array_equal(c.components_sweep_copy(k, 0, n), want[k])
        assert n_clusters == int(np.count_nonzero(want[k] == np.arange(n))) and 1 <= r <= M.ROUND_CAP
        with pytest.raises(RuntimeError, match="merged"):
            c.cluster_metrics(0)
    with pytest.raises(RuntimeError):
        c.cluster_metrics_copy(0, 1)
    assert np.array_equal(c.cluster_agreement(ids), whole_agreement)
    assert np.array_equal(c.components_copy(0, n), want[L - 1])  # the sweep's merges did not reach spk_components' labels
    dev = torch.empty(n, dtype=torch.int32, device="cuda:0")
    c.components_sweep_copy_device(1, dev)
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), want[1])
    with pytest.raises(ValueError, match="level"):
        c.components_sweep_copy_device(L, dev)
    # an invalid peer leaves no sweep; a new sweep is unmarked
    bad = other[0].copy()
    bad[7] = 8
    with pytest.raises(ValueError, match="peer label"):
        c.components_sweep_merge(0, bad)
    assert c.components_sweep_info()[0] == -1
    c.components_sweep_edges(n, u, v, score, thr)
    assert c.cluster_metrics(L - 1) == whole_metrics
    c.close()


def test_merge_leaves_selection_scores_and_sweep_alone(amd):
    df_e = scored_job(amd, "dedupe_only", [records(1500, seed=12)])
    job, ctx = df_e.job, df_e.job.ctx
    f = df_e.filter("match_probability > 0.5")
    k = f._select()
    assert k > 0
    n_nodes = ctx.components()[0]
    from splink_amd import _native as N
    ctx.components_sweep(N.SEL_MP, [0.9, 0.5])

    def state():
        sel = ctx.select_copy(0, k, len(df_e.gammas.meta[0]))
        sweep = [ctx.components_sweep_copy(j, 0, n_nodes) for j in range(2)]
        return list(sel) + sweep + [np.array(ctx.cluster_metrics(1)), job.score(df_e.lam, df_e.level_probs).copy(),
                                    job.em_stats(df_e.lam, df_e.level_probs).copy()]
    before = state()
    chain = np.maximum(np.arange(n_nodes, dtype=np.int64) - 1, 0).astype(np.uint32)  # one path through every record
    assert ctx.components_merge(chain)[0] == 1
    assert (ctx.components_copy(0, n_nodes) == 0).all()
    for a, b in zip(before, state()):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 6. the pipeline over three explicit shards in one process --------------------------------------------------------
def records(n, seed):
    from splink_amd.synthetic import make_records
    return make_records(n, seed=seed, surname_vocab=120, first_vocab=80, city_vocab=20)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]


def scored_job(amd, link_type, tables, shard=(0, 1)):
    from splink_amd.engine import Job
    from splink_amd.frames import ExpectationFrame, GammaFrame
    from splink_amd.params import Params
    from splink_amd.synthetic import cfg_settings
    s = cfg_settings(2)
    s["link_type"] = link_type
    params = Params(s, amd)
    st = params.settings
    job = Job(link_type, tables, "unique_id", 0, shard=shard)
    job.block(st["blocking_rules"])
    return ExpectationFrame(GammaFrame(job, st), st, params.params["λ"], params._level_probabilities())


def tables_for(link_type):
    df = records(3000, seed=11)
    if link_type == "dedupe_only":
        return [df]
    rng = np.random.Generator(np.random.PCG64(10))
    side = rng.random(len(df)) < 0.5  # copies of one entity fall on both sides
    return [df[side].sample(frac=1.0, random_state=1).reset_index(drop=True),
            df[~side].sample(frac=1.0, random_state=2).reset_index(drop=True)]


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only"])
def test_three_shards_merge_to_the_unsharded_clusters(link_type, amd):
    from splink_amd import _native as N
    tables = tables_for(link_type)
    whole = scored_job(amd, link_type, tables)
    mp = whole.toPandas()["match_probability"]
    qs = (0.9, 0.8, 0.6) if link_type == "dedupe_only" else (0.95, 0.9, 0.8)
    ts = [float(np.quantile(mp, q)) for q in qs]
    assert ts[0] > ts[1] > ts[2]
    t = ts[1]
    want = whole.clusters(t).toPandas()["cluster_id"].to_numpy()
    want_sweep = whole.clusters_at_thresholds(ts).toPandas()
    n = len(want)
    assert np.bincount(want).max() >= 3
    shards = [scored_job(amd, link_type, tables, shard=(s, 3)) for s in range(3)]
    assert sum(s.job.n_pairs for s in shards) == whole.job.n_pairs and all(s.job.n_pairs > 0 for s in shards)
    for s in shards:  # a shard alone is still refused, and told where to go
        with pytest.raises(ValueError, match="shards") as e:
            s.clusters(t)
        assert "components_merge" in str(e.value)
    # clusters(t)
    own = []
    for s in shards:
        assert s.filter(f"match_probability > {t!r}")._select() > 0
        assert s.job.ctx.components()[0] == n
        own.append(s.job.ctx.components_copy(0, n))
    assert any(not np.array_equal(lab.astype(np.int64), want) for lab in own)
    for target in (0, 2):  # into the first shard's context with host peers, into the last with device peers
        ctx = shards[target].job.ctx
        rows = peer_rows([own[p] for p in range(3) if p != target], n + 1)
        n_clusters, rounds = ctx.components_merge(on_device(rows) if target else rows)
        got = ctx.components_copy(0, n)
        assert np.array_equal(got.astype(np.int64), want)
        assert n_clusters == len(np.unique(want)) and rounds >= 1
    # the same per level of a three-threshold sweep
    levels = []
    for s in shards:
        s.filter(f"match_probability > {ts[2]!r}")._select()
        s.job.ctx.components_sweep(N.SEL_MP, ts)
        levels.append([s.job.ctx.components_sweep_copy(k, 0, n) for k in range(3)])
    ctx = shards[1].job.ctx
    differs = False
    for k, tk in enumerate(ts):
        col = want_sweep[f"cluster_id_{tk!r}"].to_numpy()
        differs |= not np.array_equal(levels[1][k].astype(np.int64), col)
        n_clusters, _ = ctx.components_sweep_merge(k, peer_rows([levels[0][k], levels[2][k]], n))
        assert np.array_equal(ctx.components_sweep_copy(k, 0, n).astype(np.int64), col)
        assert n_clusters == len(np.unique(col))
    assert differs
    assert np.array_equal(want_sweep[f"cluster_id_{t!r}"].to_numpy(), want)


def test_forced_merge_at_one_rank_gives_the_same_frames(amd):
    """force_reduce, as tests/test_gpu_dist.py sets it for the EM histogram: the frames gather (one row: this rank's)
    and merge, and must equal the plain ones; metrics() and summary() are refused on that path."""
    a = scored_job(amd, "dedupe_only", [records(1500, seed=12)])
    b = scored_job(amd, "dedupe_only", [records(1500, seed=12)])
    b.job.force_reduce = True
    ts = [0.5, 0.9]
    plain, forced = a.clusters(0.9), b.clusters(0.9)
    pd.testing.assert_frame_equal(forced.toPandas(), plain.toPandas(), check_exact=True)
    assert forced.n_clusters == plain.n_clusters < plain.count()
    assert plain.rounds >= 1 and forced.rounds >= 2  # its own rounds, and the merge's quiet one
    sa, sb = a.clusters_at_thresholds(ts), b.clusters_at_thresholds(ts)
    pd.testing.assert_frame_equal(sb.toPandas(), sa.toPandas(), check_exact=True)
    assert [sb.at(t).n_clusters for t in ts] == [sa.at(t).n_clusters for t in ts]
    assert list(sb._info[1]) == list(sa._info[1])
    for call in (forced.metrics, sb.summary, lambda: sb.metrics(0.9), lambda: sb.at(0.5).metrics()):
        with pytest.raises(ValueError, match="sharded job"):
            call()
    assert len(sa.summary()) == 2 and plain.metrics().largest_cluster >= 2


@pytest.fixture
def nccl_group(amd):
    """A world-size-1 `nccl` group, as tests/test_gpu_dist.py opens one (RCCL refuses two ranks on one device)."""
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda:0"))
    yield dist
    dist.destroy_process_group()


def test_forced_merge_through_rccl_keeps_the_labels_on_the_device(nccl_group, amd):
    """The nccl branch of the frames at one rank: labels copied device to device, all-gathered by RCCL as a device
    tensor, merged from a device pointer."""
    import torch
    from splink_amd import distributed as D
    assert D.stream_ordered_reduce(0)
    t = torch.arange(1000, dtype=torch.int32, device="cuda:0")
    got = D.allgather_labels(t, force=True)
    assert got.is_cuda and tuple(got.shape) == (1, 1000) and torch.equal(got[0], t)
    with pytest.raises(ValueError, match="device tensors"):
        D.allgather_labels(t.cpu(), force=True)
    a = scored_job(amd, "dedupe_only", [records(1500, seed=12)])
    b = scored_job(amd, "dedupe_only", [records(1500, seed=12)])
    b.job.force_reduce = True
    pd.testing.assert_frame_equal(b.clusters(0.9).toPandas(), a.clusters(0.9).toPandas(), check_exact=True)
    ts = [0.5, 0.9]
    sa, sb = a.clusters_at_thresholds(ts), b.clusters_at_thresholds(ts)
    pd.testing.assert_frame_equal(sb.toPandas(), sa.toPandas(), check_exact=True)
    assert list(sb._info[1]) == list(sa._info[1]) and list(sb._info[2]) == list(sa._info[2])


# ---- 7. two gloo ranks on cuda:0 through the public API ---------------------------------------------------------------
def _two_ranks(tmp_path, mode):
    """Run tests/gpu_merge_worker.py as two gloo ranks on cuda:0; returns their JSON outputs."""
    here = os.path.dirname(os.path.abspath(__file__))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "rank")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   LOCAL_RANK="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(here, "gpu_merge_worker.py"), out, mode], env=env))
    for p in procs:
        assert p.wait(timeout=170) == 0
    return [json.load(open(f"{out}.{r}")) for r in range(2)]


@pytest.mark.parametrize("mode", ["dedupe", "link_tf"])
def test_two_ranks_give_the_single_process_frames(mode, amd, tmp_path):
    import gpu_merge_worker as W
    single = W.run(mode)
    assert not single["sharded"] and single["refused"] == []
    n = len(single["clusters"]["cluster_id"])
    assert single["n_clusters"] < n and single["sweep_n_clusters"][0] <= single["sweep_n_clusters"][2]
    ranks = _two_ranks(tmp_path, mode)
    assert ranks[0]["n_pairs"] > 0 and ranks[1]["n_pairs"] > 0
    assert ranks[0]["n_pairs"] + ranks[1]["n_pairs"] == single["n_pairs"]
    for rk in ranks:
        assert rk["sharded"]
        assert rk["refused"] == ["one.metrics", "sweep.metrics", "sweep.summary", "at.metrics"]
        for key in ("clusters", "n_clusters", "sweep", "sweep_columns", "sweep_n_clusters", "sweep_n_edges",
                    "truth_sweep", "truth_one", "truth_at"):
            assert rk[key] == single[key], key
