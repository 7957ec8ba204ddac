"""Removal from a sharded index (include/hpfw_gpu_multi_index.h): every group search after
hpfw_gpu_group_index_remove equals its one-handle namesake after the same removal, field for field, at every placement."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hpfw_amd  # noqa: E402
from hpfw_amd import _lib, multi  # noqa: E402

import index_ref as ref  # noqa: E402
from test_gpu_multi_search import V, _placements, _workload  # noqa: E402

N_CLIPS = 206
_one = {}


def _removal(n_shards):
    """the first and last id of every shard's range, one whole shard's clips, a scattering of other ids -- unsorted, with
    repeats"""
    ids = []
    for s in range(n_shards):
        lo, hi = multi.shard_range(N_CLIPS, s, n_shards)
        ids += [lo, hi - 1]
    lo, hi = multi.shard_range(N_CLIPS, n_shards // 2, n_shards)
    whole = list(range(lo, hi)) if n_shards > 1 else []            # (one shard: its whole range would be the whole index)
    scatter = [3, 200, 17, 51, 51, 85, 119, 153, 187, 203, 204]
    return ids + whole[::-1] + scatter


def _one_handle(ids, k):
    """what one handle gives after the same removal: computed once per removal set"""
    key = (tuple(sorted(set(ids))), k)
    if key not in _one:
        db, db_off, _, q_hp, q_off = _workload()
        g = hpfw_amd.Gpu(0)
        try:
            g.index_add(db, db_off)
            g.index_remove(ids)
            hp, off = g.index_get()
            want = ref.remove(db, db_off, ids)
            assert hp.tobytes() == want[0].tobytes() and np.array_equal(off, want[1])
            _one[key] = (g.search_topk(q_hp, q_off, k), g.search_topk_scored(q_hp, q_off, k), g.search_topk_transposed(q_hp, q_off, V, k),
                         g.search_topk_transposed_scored(q_hp, q_off, V, k), g.search_votes(q_hp, q_off))
        finally:
            g.close()
    return _one[key]


@pytest.mark.parametrize("devices", _placements())
def test_group_searches_after_removal_equal_one_handle(torch_cuda, devices):
    db, db_off, sets, q_hp, q_off = _workload()
    assert db_off.size - 1 == N_CLIPS
    ids = _removal(len(devices))
    k = 10
    g = multi.GpuGroup(devices)
    try:
        g.index_build(db, db_off)
        before = g.search_topk(q_hp, q_off, k)
        # an id outside the index is refused with every shard untouched
        for bad in ([0, N_CLIPS], [5, -1]):
            with pytest.raises(hpfw_amd.HpfwError) as e:
                g.index_remove(bad)
            assert e.value.status == _lib.E_INVALID
        assert np.array_equal(g.index_offsets(), db_off)
        assert g.search_topk(q_hp, q_off, k).tobytes() == before.tobytes()
        for s in range(len(devices)):
            lo, hi = multi.shard_range(N_CLIPS, s, len(devices))
            hp, off = hpfw_amd.Gpu.from_handle(g.handle(s)).index_get()
            assert hp.tobytes() == db[db_off[lo]:db_off[hi]].tobytes() and np.array_equal(off, db_off[lo:hi + 1] - db_off[lo])
        g.index_remove(ids)
        want_hp, want_off = ref.remove(db, db_off, ids)
        assert np.array_equal(g.index_offsets(), want_off)
        for s in range(len(devices)):                              # every shard keeps its range; its clips closed up
            lo, hi = multi.shard_range(N_CLIPS, s, len(devices))
            hp, off = hpfw_amd.Gpu.from_handle(g.handle(s)).index_get()
            assert hp.tobytes() == want_hp[want_off[lo]:want_off[hi]].tobytes() and np.array_equal(off, want_off[lo:hi + 1] - want_off[lo])
        topk, (hits, stats), t, (ts, tstats), votes = _one_handle(ids, k)
        assert g.search_topk(q_hp, q_off, k).tobytes() == topk.tobytes() != before.tobytes()
        got_hits, got_stats = g.search_topk_scored(q_hp, q_off, k)
        assert got_hits.tobytes() == hits.tobytes() and got_stats.tobytes() == stats.tobytes()
        assert g.search_topk_transposed(q_hp, q_off, V, k).tobytes() == t.tobytes()
        got_ts, got_tstats = g.search_topk_transposed_scored(q_hp, q_off, V, k)
        assert got_ts.tobytes() == ts.tobytes() and got_tstats.tobytes() == tstats.tobytes()
        got_votes = g.search_votes(q_hp, q_off)
        assert got_votes.tobytes() == votes.tobytes()
        gone = np.array(sorted(set(ids)))
        assert not np.isin(got_hits["clip"], gone).any() and not np.isin(got_votes["clip"], gone).any()
        assert (got_votes["clip"] != 0xFFFFFFFF).sum() > 10
        # a second removal, ids already empty among them
        g.index_remove([0, 1, 2, 100])
        assert np.array_equal(g.index_offsets(), ref.remove(want_hp, want_off, [0, 1, 2, 100])[1])
        assert g.search_topk(q_hp, q_off, k).tobytes() == _one_handle(ids + [0, 1, 2, 100], k)[0].tobytes()
    finally:
        g.close()
