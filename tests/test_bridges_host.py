"""clusters(t).bridges(): the entry points, the header, the oracle against the definition, the host emulation of the
device's launches against the oracle, and the frame helpers (no GPU)."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
import bridges_common as B

from splink_amd import _native as N

SYMBOLS = ["spk_cluster_bridges", "spk_cluster_bridges_copy", "spk_cluster_bridges_cores_copy",
           "spk_cluster_bridges_info"]


def test_native_and_frame_methods_exist():
    from splink_amd import ClusterBridges, ClusterFrame, ClusterSweepFrame
    for name in ("cluster_bridges", "cluster_bridges_copy", "cluster_bridges_cores_copy", "cluster_bridges_info"):
        assert callable(getattr(N.Context, name)), name
    assert callable(ClusterFrame.bridges) and callable(ClusterSweepFrame.bridges)
    assert callable(ClusterBridges.edges) and callable(ClusterBridges.cores)
    assert set(SYMBOLS) <= set(N.EXPORTS)


def test_header_declares_the_symbols_and_the_library_has_them():
    raw = open(os.path.join(ROOT, "include", "splink_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*spk_ctx \*ctx" % name, text), name
    lib = N.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    src = open(os.path.join(ROOT, "splink_amd", "csrc", "spk_bridges.hip")).read()
    assert re.search(r"constexpr int BR_MAX_ROUNDS = %d;" % N.BRIDGES_MAX_ROUNDS, src)
    assert B.emulation().MAX_ROUNDS == N.BRIDGES_MAX_ROUNDS


def rows_of(res):
    return sorted(zip(*(res[k].tolist() for k in ("u", "v", "side_u", "side_v"))))


def check(n, u, v, seeds=(0, 1)):
    """The oracle agrees with the definition (small graphs), and the emulation with the oracle under every seed."""
    want = B.oracle(n, u, v)
    if len(u) <= 64:
        assert rows_of(want) == B.brute_force(n, u, v)
    emu = B.emulation()
    for seed in seeds:
        got = emu.bridges(n, u, v, seed=seed)
        B.same(got, want)
        assert got["rounds"] == (want["out4"][3] + 1 if len(u) else 0)
    return want


def test_the_oracle_on_graphs_with_known_answers():
    g = B.degenerate_graphs()
    expect = {"no_edges": [], "self_loops": [], "one_edge": [(2, 1, 1, 1)], "edge_twice": [], "edge_twice_reversed": [],
              "triangle": [], "triangle_pendant": [(3, 4, 3, 1)], "triangles_one_edge": [(3, 5, 3, 3)],
              "triangles_two_edges": [], "triangles_shared_node": [], "idle_nodes": [(5, 6, 1, 2), (6, 7, 2, 1)]}
    assert set(expect) == set(g)
    for name, (n, u, v) in g.items():
        want = B.oracle(n, u, v)
        assert rows_of(want) == expect[name], name
        assert want["out4"][0] == len(expect[name])
    n, u, v = g["triangles_shared_node"]
    want = B.oracle(n, u, v)
    assert want["core"].tolist() == [0, 1, 1, 1, 4, 1, 1, 7] and want["out4"] == (0, 4, 5, 2)
    n, u, v = g["idle_nodes"]
    want = B.oracle(n, u, v)
    assert want["core"].tolist() == [0, 1, 1, 1, 4, 5, 6, 7, 8, 9] and want["out4"] == (2, 8, 3, 2)


@pytest.mark.parametrize("name", sorted(B.degenerate_graphs()))
def test_emulation_equals_the_oracle_on_the_degenerate_graphs(name):
    n, u, v = B.degenerate_graphs()[name]
    check(n, u, v, seeds=range(4))


def test_emulation_equals_the_oracle_on_random_multigraphs():
    rng = np.random.default_rng(23)
    bridges = 0
    for i in range(400):
        n, u, v = B.random_multigraph(rng)
        bridges += check(n, u, v, seeds=(i,))["out4"][0]
    assert bridges >= 100  # the sample holds bridges at all: it is not all cycles and repeats


@pytest.mark.parametrize("m", [63, 64, 65, 255, 256, 257])
def test_emulation_equals_the_oracle_on_chains_with_chords(m):
    n, u, v = B.chain_of_edges(m)
    want = check(n, u, v)
    assert 0 < want["out4"][0] < n - 1


def test_path_cycle_and_barbell():
    n, u, v, order = B.permuted_path(300)
    want = check(n, u, v)
    at = int(np.flatnonzero(order == 0)[0])  # the root is node 0: its eccentricity is the longer arm
    assert want["out4"] == (n - 1, n, 1, max(at, n - 1 - at))
    assert (want["side_u"].astype(int) + want["side_v"] == n).all()
    n, u, v = B.permuted_cycle(257)
    assert check(n, u, v)["out4"][:3] == (0, 1, 257)
    n, u, v = B.permuted_cycle(257, tail=10)
    want = check(n, u, v)
    assert want["out4"][:3] == (10, 11, 257)
    assert sorted(np.minimum(want["side_u"], want["side_v"]).tolist()) == list(range(1, 11))
    n, u, v = B.barbell(12)
    want = check(n, u, v)
    assert rows_of(want) == [(11, 12, 12, 12)] and want["out4"][:3] == (1, 2, 12)


@pytest.mark.parametrize("name,rounds", [("hub", 3), ("random", 78)])
def test_emulation_equals_the_oracle_on_the_large_test_graphs(name, rounds):
    n, u, v = B.emulation()._CC.GRAPHS[name]()
    want = check(n, u, v, seeds=(5,))
    assert want["out4"][3] + 1 == rounds  # the rounds DESIGN.md reports for the device


def test_the_emulations_limit():
    emu = B.emulation()
    n, u, v = B.id_order_path(12)
    assert emu.bridges(n, u, v, max_rounds=12)["rounds"] == 12
    with pytest.raises(RuntimeError, match="deeper"):
        emu.bridges(n, u, v, max_rounds=11)


# ---- the frame helpers ----------------------------------------------------------------------------------------------
class _Job:
    passthrough = None
    n_shards = 1
    force_reduce = False

    def __init__(self, link_type, inputs):
        self.link_type, self.inputs = link_type, inputs

    def reduces_across_ranks(self):
        return False


class _Ctx:
    """The four calls ClusterBridges makes, answered from an oracle result."""

    def __init__(self, res):
        self.res = res

    def cluster_bridges(self, level):
        return self.res["out4"]

    def cluster_bridges_info(self):
        return 0, self.res["out4"][3] + 1, -1.0

    def cluster_bridges_copy(self, start, count):
        return tuple(self.res[k][start:start + count] for k in ("u", "v", "side_u", "side_v"))

    def cluster_bridges_cores_copy(self, start, count):
        return self.res["core"][start:start + count]


def _bridges_of(link_type, inputs, n, u, v):
    from splink_amd.frames import ClusterBridges, ClusterFrame
    frame = ClusterFrame.__new__(ClusterFrame)
    frame.job = _Job(link_type, inputs)
    frame.settings = {"unique_id_column_name": "uid"}
    res = B.oracle(n, u, v)
    lab = np.array(B._union_find(n, u.tolist(), v.tolist()), dtype=np.uint32)
    frame._labels, frame._info = lab, (n, 0, 0)
    return ClusterBridges(frame, lab, _Ctx(res), 0), res


def test_edges_and_cores_columns_and_min_side():
    n, u, v = B.degenerate_graphs()["triangles_one_edge"]
    u, v = np.append(u, [7, 8]).astype(np.uint32), np.append(v, [8, 0]).astype(np.uint32)  # 7 - 8 - 0 hang off triangle B
    ids = pd.DataFrame({"uid": ["r%d" % i for i in range(n)]})
    br, res = _bridges_of("dedupe_only", [ids], n, u, v)
    assert (br.n_bridges, br.n_cores, br.largest_core, br.depth, br.rounds) == res["out4"] + (res["out4"][3] + 1,)
    e = br.edges()
    assert list(e.columns) == ["cluster_id", "uid_l", "uid_r", "nodes_l", "nodes_r", "n_nodes"]
    assert e.values.tolist() == [[0, "r3", "r5", 3, 5, 8], [0, "r7", "r8", 6, 2, 8], [0, "r8", "r0", 7, 1, 8]]
    assert br.edges(min_side=2).values.tolist() == e.values.tolist()[:2]
    assert br.edges(min_side=3).values.tolist() == e.values.tolist()[:1] and len(br.edges(min_side=4)) == 0
    for bad in (0, -1, 1.5, "a", None):
        with pytest.raises(ValueError, match="min_side"):
            br.edges(min_side=bad)
    c = br.cores()
    assert list(c.columns) == ["cluster_id", "uid", "core_id"]
    assert c["core_id"].tolist() == [0, 1, 1, 1, 4, 5, 5, 5, 8] and (c["cluster_id"] == [0, 0, 0, 0, 4, 0, 0, 0, 0]).all()


def test_edges_of_the_two_table_link_types():
    n, u, v = 6, np.array([0, 1], dtype=np.uint32), np.array([3, 3], dtype=np.uint32)
    left = pd.DataFrame({"uid": [10, 11, 12]})
    right = pd.DataFrame({"uid": [20, 21, 22]})
    br, _ = _bridges_of("link_only", [left, right], n, u, v)
    e = br.edges()
    assert list(e.columns) == ["cluster_id", "uid_l", "uid_r", "nodes_l", "nodes_r", "n_nodes"]
    assert e.values.tolist() == [[0, 10, 20, 1, 2, 3], [0, 11, 20, 1, 2, 3]]
    assert list(br.cores().columns) == ["cluster_id", "uid", "_source_table", "core_id"]
    both = pd.concat([left.assign(_source_table="left"), right.assign(_source_table="right")], ignore_index=True)
    br, _ = _bridges_of("link_and_dedupe", [both], n, u, v)
    e = br.edges()
    assert list(e.columns) == ["cluster_id", "uid_l", "uid_r", "_source_table_l", "_source_table_r", "nodes_l", "nodes_r",
                               "n_nodes"]
    assert e.values.tolist() == [[0, 10, 20, "left", "right", 1, 2, 3], [0, 11, 20, "left", "right", 1, 2, 3]]


def test_refusals():
    from splink_amd.frames import ClusterBridges, ClusterFrame, ClusterSweepFrame, reject_filtered
    with pytest.raises(ValueError, match="cluster frame"):
        reject_filtered(ClusterBridges.__new__(ClusterBridges), "run_maximisation_step")
    frame = ClusterFrame.__new__(ClusterFrame)
    frame.job = _Job("dedupe_only", [])
    frame.job.force_reduce = True
    with pytest.raises(ValueError, match=r"bridges\(\) on a sharded job"):
        frame.bridges()
    sweep = ClusterSweepFrame.__new__(ClusterSweepFrame)
    sweep.job, sweep.thresholds, sweep._level = frame.job, [0.5], [0]
    with pytest.raises(ValueError, match=r"bridges\(\) on a sharded job"):
        sweep.bridges(0.5)
    with pytest.raises(ValueError, match="not one of this frame's thresholds"):
        sweep.bridges(0.7)
