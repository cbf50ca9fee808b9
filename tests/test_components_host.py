"""frame.clusters(): the entry points, the header, and the host emulation of the kernel's rounds (no GPU)."""
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from splink_amd import _native as N

SYMBOLS = ["spk_components", "spk_components_edges", "spk_components_copy", "spk_components_info",
           "spk_components_release"]
ROUND_CAP = 256  # test_gpu_components.py's bound on the long path: 16 log2(65536)


def emulation():
    spec = importlib.util.spec_from_file_location("emulate_components", os.path.join(ROOT, "tools", "emulate_components.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def union_find(n_nodes, u, v):
    """label[x] = the smallest id of x's component: find with path halving, link to the smaller id."""
    parent = list(range(n_nodes))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n_nodes)], dtype=np.uint32)


def test_native_and_frame_methods_exist():
    from splink_amd import ClusterFrame, FilteredFrame
    from splink_amd.frames import ExpectationFrame
    for name in ("components", "components_edges", "components_copy", "components_info", "components_release"):
        assert callable(getattr(N.Context, name)), name
    assert callable(FilteredFrame.clusters) and callable(ExpectationFrame.clusters)
    for name in ("toPandas", "count"):
        assert callable(getattr(ClusterFrame, name)), name
    assert isinstance(ClusterFrame.n_clusters, property) and isinstance(ClusterFrame.rounds, property)
    assert set(SYMBOLS) <= set(N.EXPORTS)


def test_no_device_means_native_unavailable():
    """Every entry point sits behind a Context, and making one without a library or a device raises."""
    if N.device_count() > 0:
        return
    with pytest.raises(N.NativeUnavailable):
        N.Context(0).components_edges(2, [0], [1])
    with pytest.raises(N.NativeUnavailable):
        N.Context(0).components()


def test_header_declares_the_five_symbols():
    text = open(os.path.join(ROOT, "include", "splink_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*spk_ctx \*ctx" % name, text), name
    lib = N.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_constants_mirror_the_kernel_file():
    text = open(os.path.join(ROOT, "splink_amd", "csrc", "spk_components.hip")).read()
    threads = int(re.search(r"CC_THREADS = (\d+);", text).group(1))
    vec = int(re.search(r"CC_VEC = (\d+);", text).group(1))
    assert "CC_CHUNK = (int64_t)CC_THREADS * CC_VEC;" in text and threads * vec == N.COMPONENTS_CHUNK
    emu = emulation()
    assert int(re.search(r"CC_CLIMB = (\d+);", text).group(1)) == emu.CLIMB
    assert int(re.search(r"CC_MAX_ROUNDS = (\d+);", text).group(1)) == emu.ROUND_CAP == ROUND_CAP


def test_cluster_frame_is_refused_by_the_stage_functions():
    from splink_amd.frames import ClusterFrame, reject_filtered
    c = ClusterFrame.__new__(ClusterFrame)
    with pytest.raises(ValueError, match="cluster frame"):
        reject_filtered(c, "run_maximisation_step")


@pytest.mark.parametrize("name", ["path", "hub", "random"])
def test_emulated_rounds_reach_the_union_find_labels(name):
    emu = emulation()
    n, u, v = emu.GRAPHS[name]()
    want = union_find(n, u, v)
    got, rounds = emu.components(n, u, v)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(emu.union_find(n, u, v), want)
    if name == "path":
        assert n == 65536 and len(u) == n - 1 and (want == 0).all()
        assert rounds <= ROUND_CAP // 4, rounds  # a quarter of the device test's cap, on this very graph
    if name == "hub":
        assert len(u) == 20000 + 32640 and np.count_nonzero(want == np.arange(n)) == 1000 + 2
    if name == "random":
        assert n == 200000 and len(u) == 150000
