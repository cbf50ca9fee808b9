"""Clusters of a sharded job, without a GPU: the host emulation of spk_components_merge's rounds against a union-find,
the label all-gather under two gloo ranks, and the argument checks of the new _native wrappers."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

import merge_common as M
from splink_amd import _native as N

SYMBOLS = ["spk_components_merge", "spk_components_sweep_merge", "spk_components_copy_device",
           "spk_components_sweep_copy_device"]


# ---- the emulated merge -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", M.DEALINGS)
@pytest.mark.parametrize("parts", M.PARTS)
@pytest.mark.parametrize("name", M.GRAPH_NAMES)
def test_emulated_merge_reaches_the_union_find_labels(name, parts, how):
    """Every part labelled on its own (the emulated spk_components), then parts 1.. merged into part 0 under the least
    favourable staleness model: the labels are the union-find's of all edges, within a quarter of the device's round
    cap (the margin tests/test_components_host.py gives the emulation)."""
    emu = M.emulation()
    n, u, v, want = M.graph(name)
    own = [emu.components(n, pu, pv)[0] for pu, pv in M.dealt(name, parts, how)]
    got, rounds = emu.components_merge(own[0], np.stack(own[1:]))
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert 1 <= rounds <= M.ROUND_CAP // 4, rounds
    if name == "path":
        assert (want == 0).all() and any((lab != 0).any() for lab in own)  # the long path forms only in the union
    # one call with every peer = one call per peer, and a graph merged into itself does not change
    step = own[0]
    for lab in own[1:]:
        step, _ = emu.components_merge(step, lab[None, :])
    assert np.array_equal(step, want)
    again, r = emu.components_merge(got, got[None, :])
    assert np.array_equal(again, got) and r == 1


def test_emulated_merge_refuses_an_entry_above_its_index():
    emu = M.emulation()
    with pytest.raises(ValueError):
        emu.components_merge(np.arange(4), np.array([[0, 2, 2, 3]]))


def test_dealings_partition_the_edges():
    emu = M.emulation()
    for how in M.DEALINGS:
        part = emu.deal_edges(10, 3, how)
        assert sorted(set(part.tolist())) == [0, 1, 2] and len(part) == 10
    assert emu.deal_edges(10, 3, "round_robin").tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]
    assert (np.diff(emu.deal_edges(10, 3, "blocks")) >= 0).all()


# ---- the all-gather of the labels, two gloo ranks on the CPU -----------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_labels(rank, n=1000):
    return (np.arange(n, dtype=np.uint32) // np.uint32(rank + 2)) * np.uint32(rank + 2)


def _gather_rank_main(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from splink_amd import distributed as D
    mine = _rank_labels(rank)
    mine[-1] = 0xFFFFFFF0 + rank  # the top bit survives the int32 wire format
    got = D.allgather_labels(torch.from_numpy(mine.view(np.int32)))
    assert got.dtype == torch.int32 and tuple(got.shape) == (world, len(mine)) and not got.is_cuda
    np.save(os.path.join(out_dir, f"labels{rank}.npy"), got.numpy().view(np.uint32))
    dist.destroy_process_group()


def test_two_rank_gloo_allgather_labels(tmp_path):
    world = 2
    mp.start_processes(_gather_rank_main, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    want = np.stack([_rank_labels(r) for r in range(world)])
    for r in range(world):
        want[r, -1] = 0xFFFFFFF0 + r
    for r in range(world):
        assert np.array_equal(np.load(tmp_path / f"labels{r}.npy"), want)


def test_allgather_labels_without_a_group_is_one_row():
    from splink_amd import distributed as D
    t = torch.arange(5, dtype=torch.int32)
    got = D.allgather_labels(t)
    assert tuple(got.shape) == (1, 5) and got.tolist() == [[0, 1, 2, 3, 4]]
    with pytest.raises(ValueError):
        D.allgather_labels(torch.arange(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        D.allgather_labels(torch.zeros((2, 3), dtype=torch.int32))


# ---- the entry points and the wrappers' own checks ---------------------------------------------------------------------
def test_symbols_header_and_constants():
    assert set(SYMBOLS) <= set(N.EXPORTS)
    lib = N.load_library()
    text = open(os.path.join(ROOT, "include", "splink_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(\s*spk_ctx \*ctx" % name, code), name
    cap = int(re.search(r"#define SPK_COMPONENTS_MAX_PEERS (\d+)", text).group(1))
    assert cap == N.COMPONENTS_MAX_PEERS == 64
    kernel = open(os.path.join(ROOT, "splink_amd", "csrc", "spk_components.hip")).read()
    assert "CC_MAX_PEERS = SPK_COMPONENTS_MAX_PEERS;" in kernel and "k_cc_jump_stars" in kernel
    for name in ("components_merge", "components_sweep_merge", "components_copy_device", "components_sweep_copy_device"):
        assert callable(getattr(N.Context, name)), name


def test_peer_argument_checks_need_no_device():
    peers = N.Context._peer_labels
    a = np.arange(12, dtype=np.uint32).reshape(3, 4)
    n_peers, addr, stride, on_device, keep = peers(a)
    assert (n_peers, stride, on_device) == (3, 4, False) and addr == keep.ctypes.data and keep.dtype == np.uint32
    assert peers(np.arange(4, dtype=np.int32))[:1] + peers(np.arange(4, dtype=np.int32))[2:4] == (1, 4, False)
    assert peers(a[:, ::2])[2] == 2  # made contiguous
    assert peers(torch.arange(8, dtype=torch.int32).reshape(2, 4))[:1] == (2,)
    assert peers(np.zeros((2, 0), dtype=np.uint32))[2] == 0
    for bad in (np.zeros((0, 4), np.uint32), np.zeros((N.COMPONENTS_MAX_PEERS + 1, 4), np.uint32),
                np.zeros((2, 2, 2), np.uint32), np.zeros((2, 4), np.int64), np.zeros((2, 4), np.float32),
                torch.zeros((2, 4), dtype=torch.int64), torch.zeros((0, 4), dtype=torch.int32)):
        with pytest.raises(ValueError, match="components_merge"):
            peers(bad)
    with pytest.raises(ValueError, match="components_sweep_merge"):
        peers(np.zeros((0, 4), np.uint32), "components_sweep_merge")


def test_no_device_means_native_unavailable():
    if N.device_count() > 0:
        return
    with pytest.raises(N.NativeUnavailable):
        N.Context(0).components_merge(np.zeros((1, 2), np.uint32))


def test_explicit_shard_message_points_at_the_merge():
    """A job with an explicit shard and no process group keeps its refusal ("shards"), which now names the merge."""
    from splink_amd import frames as F

    class OneShard:
        n_shards, shard, force_reduce, passthrough = 2, 0, False, None

        def reduces_across_ranks(self):
            return False

    for what in ("clusters()", "clusters_at_thresholds()"):
        with pytest.raises(ValueError, match="shards") as e:
            F._refuse_unreachable_shards(OneShard(), what)
        assert "Context.components_merge" in str(e.value) and what in str(e.value)
    whole = OneShard()
    whole.n_shards = 1
    F._refuse_unreachable_shards(whole, "clusters()")
    F._refuse_sharded_metrics(whole, "metrics()")
    whole.force_reduce = True
    with pytest.raises(ValueError, match="sharded job"):
        F._refuse_sharded_metrics(whole, "summary()")
