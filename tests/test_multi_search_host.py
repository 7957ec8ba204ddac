"""CPU tests of the sharded key, tempo and scored searches: the C surface of
include/hpfw_gpu_multi_search.h and of the two device entry points behind it, the argument checks that come before any
device is used, the C++ facade, the arithmetic of the group-level scored bound, and hpfw_amd.dist.allgather_topk_scored
under gloo.  The libraries load without a device; nothing here touches one."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, multi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


def _declared(header, pattern):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(pattern, text))


def test_search_entry_points_are_declared_and_exported():
    assert _declared("hpfw_gpu_multi_search.h", r"\b(hpfw_gpu_(?:group|shard)_\w+)\s*\(") == set(multi.SEARCH_EXPORTS)
    assert len(multi.SEARCH_EXPORTS) == 4 and not set(multi.SEARCH_EXPORTS) & (set(multi.EXPORTS) | set(multi.RESAMPLE_EXPORTS))
    M = multi.lib()
    assert all(hasattr(M, s) for s in multi.SEARCH_EXPORTS)
    single = _declared("hpfw_gpu.h", r"\b(hpfw_gpu_\w+)\s*\(")
    for sym in ("hpfw_gpu_merge_topk_device", "hpfw_gpu_sum_stats_device", "hpfw_gpu_get_filters"):
        assert sym in single and sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym), sym


def _message():
    return hpfw_amd.lib().hpfw_gpu_last_error().decode()


def test_bad_arguments_are_refused_before_any_device_is_used():
    """there is no device here and no group: a bad k (the plain search included), a bad n_shifts and null stats are named by the
    messages of the one-handle functions although the group is NULL, so they are checked before the group (and through it a device) is looked at; a NULL
    group with good arguments is refused too"""
    M = multi.lib()
    q = np.zeros(8, np.uint64)
    off = np.arange(0, 9, 2, dtype=np.int64)                       # four sets of two hashprints
    hits = np.zeros((4, 64), _lib.HIT_DTYPE)
    stats = np.zeros(4, _lib.STATS_DTYPE)
    P = _lib._hp
    scored = lambda k, st: M.hpfw_gpu_group_search_topk_scored(None, P(q), P(off), 4, k, P(hits), st)
    transposed = lambda ns, k: M.hpfw_gpu_group_search_topk_transposed(None, P(q), P(off), 2, ns, k, P(hits))
    both = lambda ns, k, st: M.hpfw_gpu_group_search_topk_transposed_scored(None, P(q), P(off), 2, ns, k, P(hits), st)
    plain = lambda k: M.hpfw_gpu_group_search_topk(None, P(q), P(off), 4, k, P(hits))
    for k in (0, 65, -1):
        for rc in (scored(k, P(stats)), transposed(2, k), both(2, k, P(stats))):
            assert rc == E_INVALID and _message() == "k must be in 1..64", (k, _message())
    for k in (0, 65):                                              # the plain search goes through the same checks
        assert plain(k) == E_INVALID and _message() == "k must be in 1..64", (k, _message())
    for ns in (0, 65, -3):
        for rc in (transposed(ns, 3), both(ns, 3, P(stats))):
            assert rc == E_INVALID and _message() == "bad argument", (ns, _message())
    for rc in (scored(3, None), both(2, 3, None)):
        assert rc == E_INVALID and _message() == "null stats"
    for rc in (plain(3), scored(3, P(stats)), transposed(2, 3), both(2, 3, P(stats))):   # nothing wrong but the group
        assert rc == E_INVALID and _message() == "bad argument"
    assert M.hpfw_gpu_group_extract_windows_pcm16(None, P(np.zeros(4, np.int16)), 4, 220500, 110250, None, 0, None, 0, P(q)) == E_INVALID
    # the two device entry points: the checks of the host merge, before the handle is used
    L = hpfw_amd.lib()
    for n_shards, k in ((0, 3), (65, 3), (2, 0), (2, 65)):
        assert L.hpfw_gpu_merge_topk_device(None, 16, n_shards, 4, k, 32, None) == E_INVALID
    assert L.hpfw_gpu_merge_topk_device(None, 16, 2, 4, 3, 32, None) == E_INVALID           # null handle
    for n_shards in (0, 65):
        assert L.hpfw_gpu_sum_stats_device(None, 16, n_shards, 4, 32, None) == E_INVALID
    assert L.hpfw_gpu_get_filters(None, None) == E_INVALID


def test_group_scored_bound_arithmetic():
    """n_clips * k_max^2 * 4096 < 2^64 with the group's clip count: at the longest query (16 000 hashprints) the first refused
    index has 17 592 187 clips, and each of two shards of it, seeing its own 8 796 094 or 8 796 093, would pass alone --
    tests/test_gpu_multi_search.py runs exactly that case on the device"""
    bound = lambda n_clips, k_max: n_clips * k_max * k_max * 4096 < 2 ** 64
    first = -(-2 ** 64 // (16000 * 16000 * 4096))
    assert first == 17_592_187 and not bound(first, 16000) and bound(first - 1, 16000)
    halves = [b - a for a, b in (multi.shard_range(first, s, 2) for s in range(2))]
    assert halves == [8_796_094, 8_796_093] and all(bound(n, 16000) for n in halves)
    assert first < 0xfffffff0                                       # within the group's limit on the number of clips
    # the moments themselves: d <= 64 k_max per counted clip
    assert (first - 1) * (64 * 16000) ** 2 < 2 ** 64 <= first * (64 * 16000) ** 2


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/sharded_storage.h>
#include <hpfw/gpu/tempo.h>
#include <hpfw/gpu/timeline.h>
#include <hpfw/gpu/transposed.h>
int main(int argc, char **argv)
{
    if (argc < 3) { // no argument: no device touched
        if (hpfw_gpu_group_search_topk_transposed(nullptr, nullptr, nullptr, 1, 3, 0, nullptr) != HPFW_E_INVALID) return 1;
        return hpfw_gpu_group_search_topk_scored(nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr) == HPFW_E_INVALID ? 2 : 1;
    }
    using Storage = hpfw::db::ShardedGpuStorage<hpfw::GpuCollector>;
    hpfw_gpu *h = nullptr; // the extractor's handle: it holds the index's filters
    if (hpfw_gpu_create(0, &h) != 0) return 1;
    Storage s(std::vector<int>{0, 0});
    const auto keyed = s.find_topk_transposed(hpfw::transposed_hashprints(h, argv[1], {-2, 0, 2}), 3);
    const auto paced = s.find_topk_transposed(hpfw::tempo_hashprints(h, argv[1], {0.96f, 1.0f, 1.04f}, {-2, 0, 2}), 3);
    const Storage::ShiftResult *first = keyed.empty() ? nullptr : &keyed[0];
    hpfw::TimelineOptions opt;
    opt.min_score = 10;
    const hpfw::Timeline t = hpfw::timeline(s, h, argv[2], opt);
    return (int)(t.segments.size() + paced.size() + s.index_offsets().size() + s.names().size()) + (first ? first->shift_index : 0)
           + (s.group() ? 0 : 1) + (hpfw_gpu_device(h) ? 1 : 0);
}
"""


def test_facade_with_the_sharded_finds_compiles_and_links(tmp_path):
    src = tmp_path / "facade.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "facade"), "-L", lib_dir, "-lhpfw_gpu_multi", "-lhpfw_gpu", "-Wl,-rpath," + lib_dir,
           "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "facade")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2


# ---- hpfw_amd.dist.allgather_topk_scored under gloo -------------------------------------------------------------------------
N_Q, K, SETS = 23, 5, 3


def _rank_lists(rank, world):
    """seeded per-rank results as a shard's transposed scored search leaves them: SHIFT_HIT_DTYPE [N_Q][K] ascending by
    (dist, clip) with globally distinct clips, fewer than K hits on some rows (padding: dist = clip = 0xffffffff, offset 0,
    shift_index -1), equal distances across ranks; STATS_DTYPE [N_Q][SETS] with moments near 2^63, so that their sum wraps in
    int64 and not in uint64"""
    rng = np.random.default_rng(900 + rank)
    hits = np.zeros((N_Q, K), _lib.SHIFT_HIT_DTYPE)
    for q in range(N_Q):
        n = int(rng.integers(0, K + 1)) if (q + rank) % 4 else K
        d = np.sort(rng.integers(0, 6, n)).astype(np.uint32) * 100            # few distinct distances: the clip decides
        clips = rng.choice(1000, n, replace=False).astype(np.uint32) * 8 + rank
        rows = sorted(zip(d.tolist(), clips.tolist()))
        for t in range(K):
            hits[q, t] = (rows[t][0], rows[t][1], int(rng.integers(-50, 5000)), int(rng.integers(0, SETS))) if t < n else \
                (0xFFFFFFFF, 0xFFFFFFFF, 0, -1)
    stats = np.zeros((N_Q, SETS), _lib.STATS_DTYPE)
    stats["sum"] = rng.integers(0, 2 ** 63 // world, (N_Q, SETS), dtype=np.uint64) * 2
    stats["sum_sq"] = rng.integers(0, 2 ** 64 // world, (N_Q, SETS), dtype=np.uint64)
    stats["sum_sq"][0, 0] = 2 ** 63 - 1 if rank == 0 else 1                  # crosses 2^63 exactly
    stats["n"] = rng.integers(0, 2 ** 32 // world, (N_Q, SETS), dtype=np.uint32)
    return hits, stats


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from hpfw_amd import dist as hdist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    hits, stats = _rank_lists(rank, world)
    merged, total = hdist.allgather_topk_scored(hits, stats, K)
    q.put((rank, merged.dtype == _lib.SHIFT_HIT_DTYPE, merged.tobytes(), total.tobytes()))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allgather_topk_scored_equals_single_rank(world):
    """every rank ends with the single-rank answer: the lists of all ranks merged by the host hpfw_gpu_merge_topk (shift hits
    keep their fourth word) and the moments summed as Python integers modulo 2^64 (n modulo 2^32)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    parts = [_rank_lists(r, world) for r in range(world)]
    want_hits = _lib.merge_topk(np.stack([h.view(_lib.HIT_DTYPE) for h, _ in parts]), K).view(_lib.SHIFT_HIT_DTYPE)
    # (the merge is what a sort of all ranks' records by (dist, clip) gives, padding last)
    for qi in range(N_Q):
        recs = sorted((int(r["dist"]), int(r["clip"]), int(r["offset"]), int(r["shift_index"])) for h, _ in parts for r in h[qi])
        assert [tuple(int(x) for x in r) for r in want_hits[qi]] == recs[:K]
    want = np.zeros((N_Q, SETS), _lib.STATS_DTYPE)
    for i in range(N_Q):
        for j in range(SETS):
            want[i, j] = (sum(int(s[i, j]["sum"]) for _, s in parts) % 2 ** 64, sum(int(s[i, j]["sum_sq"]) for _, s in parts) % 2 ** 64,
                          sum(int(s[i, j]["n"]) for _, s in parts) % 2 ** 32, 0)
    assert sum(int(s[0, 0]["sum_sq"]) for _, s in parts) >= 2 ** 63       # the int64 all-reduce wrapped on the way
    for _, is_shift, raw_hits, raw_stats in got:
        assert is_shift
        assert raw_hits == want_hits.tobytes()
        assert raw_stats == want.tobytes()
