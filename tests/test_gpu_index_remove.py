"""Removal from the index in place on the GPU against the rule of tests/index_ref.py: index_get byte for
byte at the shapes where the kernels change path, and every search against a fresh handle built with the removed clips empty."""
import ctypes
import os

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib

import index_ref as ref

pytestmark = pytest.mark.gpu

N_CLIPS = 40
STAGE_KB = 96                                             # three tiles of 4096 hashprints to a chunk


def _geometry():
    tile, chunk = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(hpfw_amd.lib().hpfw_gpu_index_remove_geometry(ctypes.byref(tile), ctypes.byref(chunk)))
    return tile.value, chunk.value


@pytest.fixture(scope="module")
def ix(torch_cuda):
    """a handle of this file's own: the session's handle keeps its index"""
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


@pytest.fixture
def small_chunks():
    os.environ["HPFW_INDEX_STAGE_KB"] = str(STAGE_KB)
    yield STAGE_KB * 1024 // 8
    os.environ.pop("HPFW_INDEX_STAGE_KB", None)


def _build(g, lengths, seed=0):
    off = np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)]).astype(np.int64)
    hp = ref.mixed(int(off[-1]), seed)
    g.index_clear()
    g.index_add(hp, off)
    return hp, off


def _check(g, want, what):
    hp, off = g.index_get()
    assert np.array_equal(off, want[1]), what
    assert hp.size == want[0].size, what
    if hp.tobytes() != want[0].tobytes():
        bad = int(np.flatnonzero(hp != want[0])[0])
        raise AssertionError(f"{what}: first difference at hashprint {bad} of {hp.size}")


def _base_lengths(seed):
    return [int(n) for n in np.random.default_rng([0x69647872, seed]).integers(1200, 2400, N_CLIPS)]


def _shapes(tile, chunk):
    """name -> (lengths, the removals made one after the other)"""
    base = _base_lengths(1)
    assert len(base) == N_CLIPS and sum(base) >= 5 * chunk
    first = lambda n: [n] + base[1:]
    long_at_3 = base[:3] + [3 * chunk + 5] + base[4:]
    edges = [e + d for e in (tile, chunk) for d in range(-2, 3)]
    with_empty = base[:5] + [0] + base[6:]
    return {
        "nothing": (base, [[]]),
        "first clip of 1 hashprint (odd shift)": (first(1), [[0]]),
        "first clip of 2 hashprints (even shift)": (first(2), [[0]]),
        "last clip": (base, [[N_CLIPS - 1]]),
        "all clips": (base, [list(range(N_CLIPS))]),
        "two adjacent clips": (base, [[7, 8]]),
        "every other clip of lengths 1 to 3": ([1 + i % 3 for i in range(30001)], [list(range(0, 30001, 2))]),
        "every other clip of lengths 1 to 3, from the second": ([1 + (i * 7) % 3 for i in range(30001)], [list(range(1, 30001, 2))]),
        "the clip in front of one longer than three chunks": (long_at_3, [[2]]),
        "the clip behind one longer than three chunks": (long_at_3, [[4]]),
        "a shift larger than a chunk, then a small one": (long_at_3, [[3], [1]]),
        "a shift larger than a chunk and a small one in one call": (long_at_3, [[1, 3]]),
        "widths within 2 of the tile and the chunk": ([3] + edges + [5] + edges, [list(range(0, 2 * len(edges) + 2, 2)), [1, 3]]),
        "an empty clip, a repeated id, an unsorted list": (with_empty, [[9, 3, 9, 5, 3], [5, 9]]),
    }


SHAPES = list(_shapes(4096, STAGE_KB * 128))


def test_geometry(ix, small_chunks):
    tile, chunk = _geometry()
    assert tile == 4096 and chunk >= tile, "SHAPES above is listed for this tile"
    assert small_chunks == 3 * tile


@pytest.mark.parametrize("name", SHAPES)
def test_shapes(ix, small_chunks, name):
    tile, _ = _geometry()
    lengths, removals = _shapes(tile, small_chunks)[name]
    want = _build(ix, lengths, seed=len(name))
    cap = ix.index_capacity()
    for ids in removals:
        ix.index_remove(ids)
        want = ref.remove(want[0], want[1], ids)
        _check(ix, want, (name, ids[:8]))
        assert ix.index_size() == len(lengths) and ix.index_capacity() == cap


def test_out_of_range_id_changes_nothing(ix, small_chunks):
    want = _build(ix, _base_lengths(2))
    for ids in ([3, N_CLIPS], [-1], [0, 1, 2, 1 << 40]):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            ix.index_remove(ids)
        assert e.value.status == _lib.E_INVALID
        _check(ix, want, ids)


def test_default_staging_large(ix):
    """2^23 hashprints in 4096 clips, clip 0 of one hashprint removed: every hashprint moves left by one, so every tile's
    sources overlap the next tile's destination -- the shape at which an in-place copy without the plan's order goes wrong"""
    assert "HPFW_INDEX_STAGE_KB" not in os.environ and "HPFW_INDEX_STAGE_MB" not in os.environ
    _, chunk = _geometry()
    lengths = [1] + [2048] * 4094 + [2048 + 2047]
    assert len(lengths) == 4096 and sum(lengths) == 1 << 23 and chunk >= 4096
    want = _build(ix, lengths, seed=23)
    ix.index_remove([0])
    _check(ix, ref.remove(want[0], want[1], [0]), "2^23")
    ix.index_clear()


def test_add_and_reserve(small_chunks, torch_cuda):
    g = hpfw_amd.Gpu(0)
    try:
        lengths = _base_lengths(3)
        want = _build(g, lengths)
        cap = g.index_capacity()
        assert cap >= want[0].size
        g.index_remove([0, 10, 11])
        want = ref.remove(want[0], want[1], [0, 10, 11])
        freed = lengths[0] + lengths[10] + lengths[11]
        # the freed room suffices: ids continue at C, nothing is allocated
        extra = ref.mixed(freed, seed=77)
        g.index_add(extra, np.array([0, 5, freed], np.int64))
        want = (np.concatenate([want[0], extra]), np.concatenate([want[1], want[1][-1] + np.array([5, freed], np.int64)]))
        _check(g, want, "remove, then add")
        assert g.index_size() == N_CLIPS + 2 and g.index_capacity() == cap
        q = extra[5:5 + 300]
        hit = g.search_topk(q, np.array([0, q.size]), 1)[0, 0]
        assert (int(hit["clip"]), int(hit["offset"]), int(hit["dist"])) == (N_CLIPS + 1, 0, 0)
        # reserve: appends up to the reserved size leave the capacity alone; it never shrinks
        g.index_reserve(3 * cap + 1)
        cap3 = g.index_capacity()
        assert cap3 >= 3 * cap + 1
        _check(g, want, "reserve keeps the index")
        g.index_reserve(10)
        assert g.index_capacity() == cap3
        while want[0].size + 5000 <= 3 * cap + 1:
            more = ref.mixed(5000, seed=want[0].size)
            g.index_add(more, np.array([0, 5000], np.int64))
            want = (np.concatenate([want[0], more]), np.concatenate([want[1], [want[1][-1] + 5000]]))
        assert g.index_capacity() == cap3
        g.index_remove([N_CLIPS + 2])
        _check(g, ref.remove(want[0], want[1], [N_CLIPS + 2]), "appends after reserve, one removed")
        assert g.index_capacity() == cap3
    finally:
        g.close()


def _rand(n, seed):
    return np.random.default_rng([0x69786464, seed]).integers(0, 2 ** 64, n, dtype=np.uint64)


def _flip(hp, fraction, seed):
    rng = np.random.default_rng([0x666C6970, seed])
    mask = np.zeros(hp.size, np.uint64)
    for b in range(64):
        mask |= (rng.random(hp.size) < fraction).astype(np.uint64) << np.uint64(b)
    return hp ^ mask


RAGGED = [0, 1, 5, 31, 32, 33, 36, 63, 64, 71, 72, 73, 100, 143, 152, 153, 154, 200, 250, 304, 305, 306, 320, 400, 64, 143, 305, 72,
          511, 512, 513, 600, 1027, 10, 20, 153, 80, 90, 8, 16]
GONE = [31, 1, 4, 7, 10, 13, 16, 19, 22, 25, 28, 34, 37]          # a third of the clips, clip 31 among them


def _planted_case():
    """a ragged index of 40 clips; most queries are cut from clip 31, one from clip 32, one from a clip that is removed too;
    clip 36 holds a part of clip 31 (the second candidate that becomes the first)"""
    clips = [_rand(n, 700 + i) for i, n in enumerate(RAGGED)]
    clips[36][:] = clips[31][90:170]
    queries = [_flip(clips[31][100:164], 0.1, 1), _flip(clips[32][500:643], 0.1, 2), _flip(clips[31][2:307], 0.1, 3),
               _flip(clips[31][120:200:1], 0.05, 4), _flip(clips[22][3:300], 0.1, 5), _flip(clips[31][300:500], 0.1, 6),
               _flip(clips[31][:95], 0.1, 7), _flip(clips[23][10:210], 0.1, 8)]
    return clips, queries


def _all_searches(g, q_hp, q_off, gone):
    """name -> bytes of every search of the handle"""
    n_q = q_off.size - 1
    out = {}
    for var in ("HPFW_SEARCH_MFMA", "HPFW_SEARCH_SHIFT", "HPFW_SEARCH_POPC"):
        os.environ[var] = "1"
        try:
            out["topk " + var] = g.search_topk(q_hp, q_off, 5).tobytes()
        finally:
            os.environ.pop(var, None)
    hits, stats = g.search_topk_scored(q_hp, q_off, 5)
    out["scored hits"], out["scored moments"] = hits.tobytes(), stats.tobytes()
    # the transposed search: two variants of every query, the second a few bits off
    sets = []
    for i in range(n_q):
        q = q_hp[q_off[i]:q_off[i + 1]]
        sets += [q, _flip(q, 0.02, 50 + i)]
    t_hp, t_off = _lib._ragged(sets, np.uint64)
    out["transposed"] = g.search_topk_transposed(t_hp, t_off, 2, 3).tobytes()
    hits, stats = g.search_topk_transposed_scored(t_hp, t_off, 2, 3)
    out["transposed scored hits"], out["transposed scored moments"] = hits.tobytes(), stats.tobytes()
    exclude = [36, -1, 32, -1, 5, -1, 0, 23][:n_q]
    out["overlap"] = g.search_overlap(q_hp, q_off, 4, 40).tobytes()
    out["overlap exclude"] = g.search_overlap(q_hp, q_off, 4, 40, exclude=exclude).tobytes()
    hits, stats = g.search_overlap_scored(q_hp, q_off, 4, 40, exclude=exclude)
    out["overlap scored hits"], out["overlap scored moments"] = hits.tobytes(), stats.tobytes()
    out["votes"] = g.search_votes(q_hp, q_off).tobytes()
    for k, cand in ((3, 0), (3, 3), (5, 8)):
        out[f"dtw {k} {cand}"] = g.search_dtw(q_hp, q_off, k, cand).tobytes()
    for c in (gone[0], 36):
        hit, path = g.dtw_path(q_hp[q_off[0]:q_off[1]], c)
        out[f"dtw_path {c}"] = hit.tobytes() + path.tobytes()
    return out


def test_every_search_after_removal(ix, small_chunks):
    clips, queries = _planted_case()
    assert len(clips) == N_CLIPS and len(GONE) == N_CLIPS // 3
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    fresh = hpfw_amd.Gpu(0)
    try:
        for base in (0, 1000):
            ix.index_clear()
            ix.index_set_clip_base(base)
            ix.index_add(db_hp, db_off)
            before = ix.search_dtw(q_hp, q_off, 1, 0)             # (the plain search prefers the shortest clips)
            assert [int(c) - base for c in before["clip"][:, 0]] == [31, 32, 31, 31, 22, 31, 31, 23]
            ix.index_remove(GONE)
            e_hp, e_off = _lib._ragged([c[:0] if i in GONE else c for i, c in enumerate(clips)], np.uint64)
            fresh.index_clear()
            fresh.index_set_clip_base(base)
            fresh.index_add(e_hp, e_off)
            got, want = _all_searches(ix, q_hp, q_off, GONE), _all_searches(fresh, q_hp, q_off, GONE)
            assert list(got) == list(want) and len(got) >= 17
            for name in want:
                assert got[name] == want[name], (name, base)
            after = ix.search_dtw(q_hp, q_off, 1, 0)
            assert not np.isin(after["clip"].astype(np.int64) - base, GONE).any()
            assert int(after["clip"][0, 0]) - base == 36 and int(after["clip"][7, 0]) - base == 23
            # a removed clip has no path: the padding record and -1 throughout
            hit, path = ix.dtw_path(queries[0], 31)
            assert (int(hit["dist"]), int(hit["clip"]), int(hit["start"]), int(hit["end"])) == (0xFFFFFFFF, 0xFFFFFFFF, 0, 0)
            assert path.size == queries[0].size and (path == -1).all()
    finally:
        fresh.close()
        ix.index_set_clip_base(0)


def test_ordering_without_synchronisation(ix, small_chunks, torch_cuda):
    """search on stream 1, removal on stream 2, search on stream 3, nothing waited for until the end: the first search answers
    on the old index, the second on the rebuilt one"""
    torch = torch_cuda
    clips, queries = _planted_case()
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    ix.index_clear()
    ix.index_add(db_hp, db_off)
    want_old = ix.search_topk(q_hp, q_off, 5)
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    d_q = torch.from_numpy(q_hp.view(np.int64)).cuda()
    n = (q_off.size - 1) * 5 * _lib.HIT_DTYPE.itemsize
    out_old = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out_new = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ix.search_topk_dev(d_q.data_ptr(), q_off, 5, out_old.data_ptr(), s1.cuda_stream)
    ix.index_remove(GONE, s2.cuda_stream)
    ix.search_topk_dev(d_q.data_ptr(), q_off, 5, out_new.data_ptr(), s3.cuda_stream)
    torch.cuda.synchronize()
    assert out_old.cpu().numpy().tobytes() == want_old.tobytes()
    want = ref.remove(db_hp, db_off, GONE)
    _check(ix, want, "ordering")
    fresh = hpfw_amd.Gpu(0)
    try:
        fresh.index_add(*want)
        want_new = fresh.search_topk(q_hp, q_off, 5)
    finally:
        fresh.close()
    assert out_new.cpu().numpy().tobytes() == want_new.tobytes() and want_new.tobytes() != want_old.tobytes()


# ---- LiveSongIdentification on synthetic recordings ---------------------------------------------------------------------------
N_SONGS = 10


def _identifier(filters, pairs, **kw):
    """an identifier whose collector holds the filter fixture, built (not indexed: nothing is learned) from (array, name) pairs"""
    lsi = hpfw_amd.LiveSongIdentification(**kw)
    lsi.collector.gpu().set_filters(filters)
    lsi.build(pairs)
    return lsi


def _cache(tmp_path, filters):
    """a cache directory that holds the filter fixture and nothing else: what calc_hashprints needs to have been loaded"""
    cache = str(tmp_path / "cache") + "/"
    os.makedirs(cache, exist_ok=True)
    with open(os.path.join(cache, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes() + np.ascontiguousarray(filters, np.float32).tobytes())
    return cache


@pytest.fixture(scope="module")
def songs(filters, torch_cuda):
    """ten recordings of 10 s and their hashprints under the filter fixture, computed once"""
    from hpfw_amd import synth
    pcm = np.stack([synth.gen_clip(800 + i, 10.0) for i in range(N_SONGS)])
    g = hpfw_amd.Gpu(0)
    try:
        g.set_filters(filters)
        hp = [h.copy() for h in g.extract(pcm)]
    finally:
        g.close()
    return pcm, hp, [f"song{i:02d}" for i in range(N_SONGS)]


def test_identifier_remove_and_add(tmp_path, filters, songs):
    from hpfw_amd import synth
    pcm, hp, names = songs
    sr = synth.SR
    queries = []
    for name, seg in (("q2", pcm[2][2 * sr:7 * sr]), ("q0", pcm[0][4 * sr:9 * sr]), ("q5", pcm[5][1 * sr:6 * sr]), ("q4", pcm[4][3 * sr:8 * sr])):
        queries.append(str(tmp_path / f"{name}.wav"))
        synth.write_wav(queries[-1], np.ascontiguousarray(seg))
    new_files = []
    for i in (0, 1):
        new_files.append(str(tmp_path / f"new{i}.wav"))
        synth.write_wav(new_files[-1], synth.gen_clip(900 + i, 8.0))
    gone = ["song02", "song05"]
    pairs = list(zip(hp, names))
    emptied = [(h[:0] if n in gone else h, n) for h, n in pairs]
    cache = _cache(tmp_path, filters)
    lsi, want = _identifier(filters, pairs, cache=cache), _identifier(filters, emptied, cache=cache)
    try:
        assert [hits[0][1] for _, hits in lsi.top(queries, 1)] == ["song02", "song00", "song05", "song04"]
        assert lsi.remove(gone) == 2 and lsi.live_names() == [n for n in names if n not in gone] and lsi.names == names
        searches = (lambda x: x.top(queries, 3), lambda x: x.top_votes(queries), lambda x: x.top_overlap(queries, 3, 100),
                    lambda x: x.top_warped(queries, 3, 0), lambda x: x.top_warped(queries, 2, 3))
        for i, search in enumerate(searches):
            got = search(lsi)
            assert got == search(want), i
            assert not any(g in repr(got) for g in gone), i
        with pytest.raises(KeyError):
            lsi.warp_path(queries[0], "song02")
        with pytest.raises(KeyError):
            lsi.remove(["song00", "song02"])
        assert lsi.live_names() == [n for n in names if n not in gone]
        # add: the old pairs plus the new ones
        assert lsi.add(new_files) == 2
        new_pairs = want.collector.calc_hashprints(new_files)
        want.build(emptied + new_pairs)
        assert lsi.names == want.names and len(lsi.names) == N_SONGS + 2
        got_hp, got_off = lsi._gpu.index_get()
        want_hp, want_off = want._gpu.index_get()
        assert got_hp.tobytes() == want_hp.tobytes() and np.array_equal(got_off, want_off)
        both = queries + new_files
        assert lsi.top(both, 3) == want.top(both, 3)
        assert [hits[0][1] for _, hits in lsi.top(new_files, 1)] == lsi.names[-2:]
        lsi.build(pairs)                                   # a fresh index forgets all removals
        assert lsi.live_names() == names and lsi.top(queries, 1)[0][1][0][1] == "song02"
    finally:
        lsi._gpu.close()
        want._gpu.close()


def test_identifier_remove_on_a_sharded_index(tmp_path, filters, songs):
    from hpfw_amd import synth
    pcm, hp, names = songs
    sr = synth.SR
    queries = []
    for name, seg in (("q2", pcm[2][2 * sr:7 * sr]), ("q3", pcm[3][4 * sr:9 * sr])):
        queries.append(str(tmp_path / f"{name}.wav"))
        synth.write_wav(queries[-1], np.ascontiguousarray(seg))
    pairs = list(zip(hp, names))
    cache = _cache(tmp_path, filters)
    one, sharded = _identifier(filters, pairs, cache=cache), _identifier(filters, pairs, cache=cache, devices=[0, 0, 0])
    try:
        assert sharded.remove(["song02", "song03"]) == 2 == one.remove(["song02", "song03"])
        assert sharded.top(queries, 3) == one.top(queries, 3) and sharded.top_votes(queries) == one.top_votes(queries)
        assert sharded.live_names() == one.live_names() and np.array_equal(sharded._gpu.index_offsets(), one._gpu.index_offsets())
        with pytest.raises(hpfw_amd.HpfwError) as e:
            sharded.add(queries)
        assert e.value.status == _lib.E_UNSUPPORTED
    finally:
        one._gpu.close()
        sharded._gpu.close()


@pytest.mark.parametrize("min_overlap", [None, 100])
def test_feed_with_a_removal_while_a_segment_is_open(filters, songs, min_overlap):
    """three songs through one feed in pushes of 2.5 s; the middle song is removed after the sixth push, while its segment is
    open.  The restatement: the feed's windows from extract_windows; the rows of the five windows completed before the removal
    from an identifier that holds everything, the later rows from one built with the song empty; one TimelineTracker over all"""
    from hpfw_amd import synth
    pcm, hp, names = songs
    sr, min_score = synth.SR, 8.0                           # (an exact window scores above 16, a window outside the index below 4)
    x = np.concatenate([pcm[0], pcm[1], pcm[2], synth.gen_clip(990, 7.5)])
    win, hop, n_before = 5 * sr, 5 * sr // 2, 5
    pairs = list(zip(hp, names))
    full = _identifier(filters, pairs)
    empty = _identifier(filters, [(h[:0] if n == "song01" else h, n) for h, n in pairs])
    try:
        w_hp = full.collector.gpu().extract_windows(x, win, hop, None, None)
        n_w = w_hp.shape[0]
        assert n_w == (x.size - win) // hop + 1 == 14
        rows_a, per_a = full._search_windows(w_hp[:n_before], None, None, min_overlap)
        rows_b, per_b = empty._search_windows(w_hp[n_before:], None, None, min_overlap)
        rows, per_window = np.concatenate([rows_a, rows_b]), per_a + per_b
        g = full._gpu.geometry(win)
        tracker = _lib.TimelineTracker(min_score, hop * g.m / (3.0 * win), win, hop)
        tracker.push(rows)
        tracker.finish()
        records = tracker.pop()
        tracker.close()
        want = []
        for sg in records:
            trim = None
            if min_overlap is not None:                    # by the length the recording had when it was added
                n_clip = hp[int(sg["clip"])].size
                a, _ = _lib.overlap_extent(per_window[int(sg["first"])][3], n_clip, g.n_hp, g.c - g.n_hp + 1, win, g.m)
                _, b = _lib.overlap_extent(per_window[int(sg["last"])][3], n_clip, g.n_hp, g.c - g.n_hp + 1, win, g.m)
                trim = (int(sg["first"]) * hop + a, int(sg["last"]) * hop + b, int(per_window[int(sg["first"])][3]))
            want.append(full._segment_tuple(sg, 0, 1.0, 3.0 * win / g.m / 44100.0, trim))
        middle = [sg for sg in records if int(sg["clip"]) == 1]
        assert len(middle) == 1 and int(middle[0]["last"]) == n_before - 1, records   # it ends at its last earlier window
        assert [int(sg["clip"]) for sg in records] == [0, 1, 2]
        got, wins = [], []
        with full.streams(1, min_score, windows=True, min_overlap=min_overlap) as live:
            for i, at in enumerate(range(0, x.size, hop)):
                if i == 6:
                    assert live.open()[0] is not None and live.open()[0][2] == "song01"
                    assert full.remove(["song01"]) == 1
                segs, rows_now = live.push([x[at:at + hop]])
                got += [sg for _, sg in segs]
                wins += [(w, row) for _, w, row in rows_now]
            got += [sg for _, sg in live.finish()]
        assert [w for w, _ in wins] == list(range(n_w))
        assert [row[:4] for _, row in wins] == [row[:4] for row in per_window]
        assert got == want, (got, want)
        assert [sg[2] for sg in got] == ["song00", "song01", "song02"]
        assert all(row[1] != "song01" for w, row in wins if w >= n_before)        # nothing later names the removed song
        assert any(row[1] == "song01" for w, row in wins if w < n_before)
    finally:
        full._gpu.close()
        empty._gpu.close()
