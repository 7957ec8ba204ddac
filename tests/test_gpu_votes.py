"""GPU tests of the voting search's device tally: the tally alone on the fixture of tests/votes_ref.py,
the sorted neighbour keys, the search against the host function (a round trip over it) and the oracle, the shard merge, the search over a
sharded index, LiveSongIdentification.top_votes end to end, and the C++ facades.  Byte for byte unless stated."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, multi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import votes_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_CLIP = 0xFFFFFFFF
_REF = {}                                                   # references computed once and shared, never changed


def _dev(torch, a):
    """a numpy array's bytes on the device (never an empty tensor: a null pointer is refused)"""
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * 8, np.uint8).copy()
    return torch.from_numpy(raw).cuda()


def _zeros(torch, n_bytes):
    return torch.zeros(n_bytes + 8, dtype=torch.uint8, device="cuda")


def _back(t, dtype, n):
    return t.cpu().numpy()[:n * np.dtype(dtype).itemsize].view(dtype).copy()


def _vote_records(votes, clip_base=0):
    """(clip or -1, offset, cnt) per query -> VOTE_DTYPE records as the library writes them"""
    out = np.zeros(len(votes), _lib.VOTE_DTYPE)
    for i, (clip, off, cnt) in enumerate(votes):
        out[i] = (NO_CLIP, 0, 0, 0.0, 0.0) if clip < 0 else (clip + clip_base, 0, off, cnt, 0.0)
    return out


def _oracle_votes(oracle, keys, w_first, db_off):
    out = []
    for q in range(w_first.size - 1):
        k = keys[w_first[q]:w_first[q + 1]]
        v = oracle.vote_windows(k, db_off) if k.shape[0] else None
        out.append((-1, 0, 0.0) if v is None or v["clip"] < 0 else (int(v["clip"]), int(v["offset"]), np.float32(v["cnt"])))
    return out


# ---- the tally alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [None, 64], ids=["default-groups", "groups-of-64"])
@pytest.mark.parametrize("clip_base", [0, 1000])
@pytest.mark.parametrize("n_q", [1, 7, 33])
def test_tally_alone_equals_the_literal_loop(gpu, oracle, torch_cuda, monkeypatch, n_q, clip_base, group):
    """the fixture's keys through vote_windows_dev; with groups of 64 windows the 33 queries fall into several groups with seams
    between queries"""
    keys, w_first, db_off = vr.fixture(n_q)
    if ("tally", n_q) not in _REF:
        _REF["tally", n_q] = _oracle_votes(oracle, keys, w_first, db_off)
    want = _vote_records(_REF["tally", n_q], clip_base)
    if group is not None:
        monkeypatch.setenv("HPFW_VOTES_GROUP_WINDOWS", str(group))
        assert n_q < 33 or w_first[-1] > 3 * group
    d_keys, d_off, d_out = _dev(torch_cuda, keys), _dev(torch_cuda, db_off), _zeros(torch_cuda, n_q * 24)
    gpu.vote_windows_dev(d_keys.data_ptr(), w_first, d_off.data_ptr(), db_off.size - 1, d_out.data_ptr(), clip_base=clip_base)
    torch_cuda.cuda.synchronize()
    got = _back(d_out, _lib.VOTE_DTYPE, n_q)
    assert got.tobytes() == want.tobytes(), [(i, got[i], want[i]) for i in range(n_q) if got[i] != want[i]][:3]


# ---- keys and search --------------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)


def _flipped(rng, seg, flips):
    seg = seg.copy()
    for _ in range(flips):
        seg ^= np.uint64(1) << rng.integers(0, 64, size=seg.size, dtype=np.uint64)
    return seg


def _workload():
    """the workload of test_gpu_parity.test_voting_search_matches_oracle: clip 5 repeats part of clip 0"""
    rng = np.random.default_rng(16)
    clips = [_rand(rng, n) for n in [400, 64, 63, 1500, 2320, 100, 1100]]
    clips[5] = clips[0][50:150].copy()
    qs = [_flipped(rng, clips[c][o:o + k], flips) for c, o, k, flips in [(3, 700, 200, 6), (4, 2000, 305, 12), (0, 50, 100, 0), (6, 10, 64, 3)]]
    qs += [_rand(rng, 90), _rand(rng, 40)]
    return clips, qs


def _ragged_case():
    """200 clips of 0 to 900 hashprints (most of them short), 40 queries of 1 to 400, some cut from clips"""
    rng = np.random.default_rng(41)
    lens = [int(x) for x in (900 * rng.random(200) ** 4)]
    lens[:6] = [0, 900, 63, 64, 65, 0]
    clips = [_rand(rng, n) for n in lens]
    q_lens = [63, 64, 65, 1, 400] + [1 + int(x) for x in (399 * rng.random(35) ** 2)]
    qs = [_rand(rng, k) for k in q_lens]
    cut = 0
    for i, k in enumerate(q_lens):
        long_enough = [c for c, n in enumerate(lens) if n >= k + 7]
        if i % 3 == 1 and k >= 64 and long_enough:
            c = long_enough[i % len(long_enough)]
            qs[i] = _flipped(rng, clips[c][7:7 + k], 8)
            cut += 1
    assert len(qs) == 40 and min(q_lens) == 1 and max(q_lens) == 400 and min(lens) == 0 and max(lens) == 900 and cut >= 3
    return clips, qs


def _reference(oracle, name, clips, qs):
    """(keys of all windows, votes per query) by the oracle, computed once per workload"""
    if name not in _REF:
        db, db_off = _lib._ragged(clips, np.uint64)
        db = db[:db_off[-1]]
        with ThreadPoolExecutor(8) as pool:                  # (the brute force leaves the interpreter while it runs)
            keys = list(pool.map(lambda x: oracle.knn_windows(db, db_off, x), qs))
        w_first = np.concatenate([[0], np.cumsum([k.shape[0] for k in keys])]).astype(np.int64)
        allk = np.concatenate(keys)
        _REF[name] = (allk, _oracle_votes(oracle, allk, w_first, db_off))
    return _REF[name]


def _index(gpu, clips):
    db, db_off = _lib._ragged(clips, np.uint64)
    gpu.index_clear()
    if len(clips):
        gpu.index_add(db, db_off)
    return db, db_off


def _search_dev(torch, gpu, q_hp, q_off, stream=None):
    n_q = q_off.size - 1
    d_q, d_out = _dev(torch, q_hp), _zeros(torch, n_q * 24)
    gpu.search_votes_dev(d_q.data_ptr(), q_off, d_out.data_ptr(), 0 if stream is None else stream.cuda_stream)
    (stream or torch.cuda).synchronize()
    return _back(d_out, _lib.VOTE_DTYPE, n_q)


def test_keys_on_the_device_are_sorted_and_exact(gpu, oracle, torch_cuda):
    clips, qs = _workload()
    _index(gpu, clips)
    q_hp, q_off = _lib._ragged(qs, np.uint64)
    want, _ = _reference(oracle, "workload", clips, qs)
    d_q, d_keys = _dev(torch_cuda, q_hp), _zeros(torch_cuda, want.size * 8)
    gpu.knn_windows_dev(d_q.data_ptr(), q_off, d_keys.data_ptr(), want.size)
    torch_cuda.cuda.synchronize()
    got = _back(d_keys, np.uint64, want.size).reshape(-1, 5)
    assert np.array_equal(got, want) and np.array_equal(got, gpu.knn_windows(q_hp, q_off))
    with pytest.raises(hpfw_amd.HpfwError) as e:
        gpu.knn_windows_dev(d_q.data_ptr(), q_off, d_keys.data_ptr(), want.size - 1)
    assert e.value.status == _lib.E_INVALID and "too small" in str(e.value)
    # an index of three items in all: two padding keys in every window
    small = [clips[0][:65], clips[3][:64], clips[4][:10]]
    db, db_off = _index(gpu, small)
    want3 = np.concatenate([oracle.knn_windows(db[:db_off[-1]], db_off, x) for x in qs if x.size >= 64])
    gpu.knn_windows_dev(d_q.data_ptr(), q_off, d_keys.data_ptr(), want.size)
    torch_cuda.cuda.synchronize()
    got3 = _back(d_keys, np.uint64, want.size).reshape(-1, 5)
    assert np.array_equal(got3, want3) and np.array_equal(got3, gpu.knn_windows(q_hp, q_off))
    assert np.all(got3[:, 3:] == vr.PAD) and np.all(got3[:, :3] != vr.PAD)


@pytest.mark.parametrize("group", [None, 64], ids=["default-groups", "groups-of-64"])
@pytest.mark.parametrize("case", ["workload", "ragged"])
def test_search_equals_the_host_function_and_the_oracle(gpu, oracle, torch_cuda, monkeypatch, case, group):
    """search_votes_dev with device pointers on a side stream = hpfw_gpu_search_votes = the oracle"""
    clips, qs = _workload() if case == "workload" else _ragged_case()
    _index(gpu, clips)
    q_hp, q_off = _lib._ragged(qs, np.uint64)
    _, votes = _reference(oracle, case, clips, qs)
    want = _vote_records(votes)
    if group is not None:
        monkeypatch.setenv("HPFW_VOTES_GROUP_WINDOWS", str(group))
    side = torch_cuda.cuda.Stream()
    with torch_cuda.cuda.stream(side):
        got = _search_dev(torch_cuda, gpu, q_hp, q_off, side)
    host = gpu.search_votes(q_hp, q_off)
    assert got.tobytes() == want.tobytes(), [(i, got[i], want[i]) for i in range(len(qs)) if got[i] != want[i]][:3]
    assert host.tobytes() == want.tobytes()
    assert (want["clip"] != NO_CLIP).sum() >= 4 and (want["clip"] == NO_CLIP).any()
    if case == "workload":
        assert [(int(v["clip"]), int(v["offset"])) for v in got[:3]] == [(3, -700), (4, -2000), (0, -50)]


def _offset_case():
    """clips of 130, 64, 63 and 0 hashprints; a query buffer whose first 17 hashprints belong to no query, then 100 hashprints
    cut from clip 0 at position 20 with 5 bit flips each, a copy of clip 1, 10 random hashprints and a query of none"""
    rng = np.random.default_rng(77)
    clips = [_rand(rng, n) for n in (130, 64, 63, 0)]
    qs = [_flipped(rng, clips[0][20:120], 5), clips[1].copy(), _rand(rng, 10), _rand(rng, 0)]
    return clips, qs, np.concatenate([_rand(rng, 17)] + qs), np.array([17, 117, 181, 191, 191], np.int64)


@pytest.mark.parametrize("group", [None, 16], ids=["default-groups", "groups-of-16"])
def test_host_calls_take_the_queries_from_q_off_0(gpu, oracle, torch_cuda, monkeypatch, group):
    """the host functions upload from q_off[0] on and rebase the offsets: ragged queries behind 17 unused hashprints give the
    oracle's keys and votes, and search_votes_dev on the same absolute offsets the same bytes; with groups of 16 windows the
    first query's 37 windows are a group of their own"""
    clips, qs, q_hp, q_off = _offset_case()
    _index(gpu, clips)
    want_keys, votes = _reference(oracle, "offset", clips, qs)
    want = _vote_records(votes)
    assert [(int(v["clip"]), int(v["offset"])) for v in want[:2]] == [(0, -20), (1, 0)] and np.all(want["clip"][2:] == NO_CLIP)
    assert want_keys.shape == (37 + 1, 5)
    if group is not None:
        monkeypatch.setenv("HPFW_VOTES_GROUP_WINDOWS", str(group))
    assert np.array_equal(gpu.knn_windows(q_hp, q_off), want_keys)
    assert gpu.search_votes(q_hp, q_off).tobytes() == want.tobytes()
    assert _search_dev(torch_cuda, gpu, q_hp, q_off).tobytes() == want.tobytes()


def test_search_edge_cases(gpu, torch_cuda):
    rng = np.random.default_rng(3)
    none = _vote_records([(-1, 0, 0.0)] * 3)
    q_hp, q_off = _lib._ragged([_rand(rng, 100), _rand(rng, 64), _rand(rng, 10)], np.uint64)
    gpu.index_clear()
    assert _search_dev(torch_cuda, gpu, q_hp, q_off).tobytes() == none.tobytes()                    # an empty index
    _index(gpu, [_rand(rng, 63), _rand(rng, 0), _rand(rng, 5)])
    assert _search_dev(torch_cuda, gpu, q_hp, q_off).tobytes() == none.tobytes()                    # no clip of 64
    assert gpu.search_votes(q_hp, q_off).tobytes() == none.tobytes()
    _index(gpu, [_rand(rng, 200)])
    got = _search_dev(torch_cuda, gpu, np.zeros(1, np.uint64), np.zeros(4, np.int64))               # empty queries
    assert got.tobytes() == none.tobytes()
    assert _search_dev(torch_cuda, gpu, np.zeros(1, np.uint64), np.zeros(1, np.int64)).size == 0    # no query
    short = _search_dev(torch_cuda, gpu, q_hp, q_off)
    assert short[0]["clip"] == 0 and short[1]["clip"] == 0 and short[2]["clip"] == NO_CLIP


# ---- the shard merge alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", [1, 45, 1000])
@pytest.mark.parametrize("n_shards", [1, 2, 3, 8])
def test_merge_alone_equals_numpy(gpu, torch_cuda, n_shards, n_win):
    rng = np.random.default_rng(100 * n_shards + n_win)
    lists, base, whole = vr.shard_lists(rng, n_shards, n_win)
    if n_win == 45:
        lists[:, 5] = vr.PAD                                # (a window whose lists are all padding, whatever the draw)
        whole[5] = vr.PAD
    d_in, d_out = _dev(torch_cuda, lists), _zeros(torch_cuda, n_win * 40)
    gpu.merge_knn_dev(d_in.data_ptr(), base, n_win, d_out.data_ptr())
    torch_cuda.cuda.synchronize()
    got = _back(d_out, np.uint64, n_win * 5).reshape(n_win, 5)
    assert np.array_equal(got, vr.merge_knn(lists, base)) and np.array_equal(got, whole)


# ---- the sharded index ------------------------------------------------------------------------------------------------------------
def _n_devices():
    """visible GPUs; a torch that does not import is an error here, not a skipped placement"""
    import torch
    return int(torch.cuda.device_count()) if torch.cuda.is_available() else 0


def _placements():
    """one GPU carries every shard; two devices are listed as skipped, not silently absent, where one GPU is visible"""
    n = _n_devices()
    marks = [] if n >= 2 else [pytest.mark.skip(reason=f"needs 2 GPUs, {n} visible")]
    return [[0], [0, 0], [0] * 8, pytest.param([0, 1], marks=marks, id="devices-0-1")]


@pytest.mark.parametrize("devices", _placements())
def test_group_search_equals_the_one_handle(gpu, oracle, torch_cuda, devices):
    clips, qs = _ragged_case()
    _, votes = _reference(oracle, "ragged", clips, qs)
    want = _vote_records(votes)
    db, db_off = _lib._ragged(clips, np.uint64)
    q_hp, q_off = _lib._ragged(qs, np.uint64)
    g = multi.GpuGroup(devices)
    try:
        g.index_build(db, db_off)
        got = g.search_votes(q_hp, q_off)
        assert got.tobytes() == want.tobytes(), [(i, got[i], want[i]) for i in range(len(qs)) if got[i] != want[i]][:3]
        assert g.search_votes(q_hp, q_off).tobytes() == want.tobytes()       # again: the offsets are on device 0 already
        g.index_build(np.zeros(1, np.uint64), np.zeros(1, np.int64))          # an empty index
        assert g.search_votes(q_hp, q_off).tobytes() == _vote_records([(-1, 0, 0.0)] * len(qs)).tobytes()
    finally:
        g.close()
    _index(gpu, clips)
    assert _search_dev(torch_cuda, gpu, q_hp, q_off).tobytes() == want.tobytes()


def test_group_search_with_a_shard_without_an_item_and_a_duplicate(gpu, torch_cuda):
    rng = np.random.default_rng(8)
    x = _rand(rng, 300)
    # three shards of two clips: the middle one holds no clip of 64 hashprints
    clips = [x, _rand(rng, 400), _rand(rng, 10), _rand(rng, 63), _rand(rng, 500), _rand(rng, 64)]
    qs = [_flipped(rng, x[100:250], 5), _flipped(rng, clips[4][30:130], 5), clips[5].copy(), _rand(rng, 80)]
    q_hp, q_off = _lib._ragged(qs, np.uint64)
    _index(gpu, clips)
    want = _search_dev(torch_cuda, gpu, q_hp, q_off)
    assert [(int(v["clip"]), int(v["offset"])) for v in want[:3]] == [(0, -100), (4, -30), (5, 0)]
    g = multi.GpuGroup([0, 0, 0])
    try:
        g.index_build(*_lib._ragged(clips, np.uint64))
        assert [multi.shard_range(6, s, 3) for s in range(3)] == [(0, 2), (2, 4), (4, 6)]
        assert g.search_votes(q_hp, q_off).tobytes() == want.tobytes()
    finally:
        g.close()
    # the query's clip is in both shards: every neighbour ties with its copy, and the lower global position wins
    clips = [_rand(rng, 350), x, _rand(rng, 200), x.copy()]
    qs = [x[40:200].copy(), _flipped(rng, x[100:250], 5)]
    q_hp, q_off = _lib._ragged(qs, np.uint64)
    _index(gpu, clips)
    want = _search_dev(torch_cuda, gpu, q_hp, q_off)
    assert [(int(v["clip"]), int(v["offset"])) for v in want] == [(1, -40), (1, -100)]
    g = multi.GpuGroup([0, 0])
    try:
        g.index_build(*_lib._ragged(clips, np.uint64))
        assert g.search_votes(q_hp, q_off).tobytes() == want.tobytes()
    finally:
        g.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
STARTS = [(2, 1.0), (0, 4.0), (5, 2.5), (3, 0.0)]           # (song, start in seconds) of the 5 s queries


def _noisy(x, seed):
    """gain 0.5 and white noise at 10 dB SNR, as synth.gen_query makes its queries"""
    seg = 0.5 * x.astype(np.float64)
    rng = np.random.default_rng([0x6E6F6973, seed])
    p = float(np.mean(seg ** 2)) + 1e-12
    seg = seg + np.sqrt(p / 10 ** (10.0 / 10)) * rng.standard_normal(seg.size)
    return np.clip(np.round(seg), -32768, 32767).astype(np.int16)


def _songs_and_queries(tmp_path):
    sr = synth.SR
    songs = [synth.gen_clip(i, 10.0) for i in range(6)]
    cuts = [songs[c][int(s * sr):int(s * sr) + 5 * sr] for c, s in STARTS] + [synth.gen_clip(103, 5.0)]
    song_files, query_files = [], []
    for i, x in enumerate(songs):
        song_files.append(str(tmp_path / f"song{i:02d}.wav"))
        synth.write_wav(song_files[-1], x)
    for i, x in enumerate(cuts):
        query_files.append(str(tmp_path / f"query{i}.wav"))
        synth.write_wav(query_files[-1], _noisy(x, i))
    return songs, song_files, query_files


def _filter_cache(path, filters):
    os.makedirs(path)
    with open(os.path.join(path, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes() + np.ascontiguousarray(filters, np.float32).tobytes())


def test_top_votes_end_to_end(tmp_path, filters, torch_cuda):
    """six songs of 10 s; four noisy 5 s queries cut from known starts and one that is in no song: on one handle and on two
    shards the right song at the right offset, the stranger below every true query, and the two placements agree exactly"""
    songs, _, query_files = _songs_and_queries(tmp_path)
    cache = str(tmp_path / "cache") + "/"
    _filter_cache(cache, filters)
    names = [f"song{i:02d}" for i in range(6)]
    results = []
    for devices in (None, [0, 0]):
        lsi = hpfw_amd.LiveSongIdentification(cache=cache, devices=devices)
        try:
            hp = list(lsi.collector.gpu().extract(np.stack(songs)))
            lsi.build(list(zip(hp, names)))
            got = lsi.top_votes(query_files)
            empty = lsi.top_votes(query_files[:1] + [str(tmp_path / "missing.wav")])
            assert empty[1] == (str(tmp_path / "missing.wav"), None) and empty[0] == got[0]
            lsi.build([])
            assert lsi.top_votes(query_files[:2]) == [(f, None) for f in query_files[:2]]          # the index has no item
        finally:
            lsi.close()
        print(devices, [(os.path.basename(f), v) for f, v in got])
        col_s = 5.0 / 403.0                                 # 5 s are 403 columns of the spectrogram
        for (label, vote), f, (song, start) in zip(got[:4], query_files, STARTS):
            cnt, name, offset = vote
            assert label == f and name == names[song] and abs(offset + start / col_s) <= 2, (label, vote)
        assert got[4][0] == query_files[4] and got[4][1][0] < min(v[0] for _, v in got[:4])
        results.append(got)
    assert results[0] == results[1]


PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/sharded_storage.h>
int main(int argc, char **argv)
{
    std::vector<std::string> to_index, to_search, *cur = nullptr;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--index")) cur = &to_index;
        else if (!std::strcmp(argv[i], "--search")) cur = &to_search;
        else if (cur) cur->push_back(argv[i]);
    }
    try {
        hpfw::GpuCollector collector;
        const auto prints = collector.prepare(to_index);
        hpfw::db::GpuStorage<hpfw::GpuCollector> one;
        hpfw::db::ShardedGpuStorage<hpfw::GpuCollector> sharded(std::vector<int>{0, 0});
        one.build(prints);
        sharded.build(prints);
        for (const auto &q : to_search) {
            const auto hp = collector.calc_hashprint(q);
            const auto a = one.find_votes(hp);
            const auto b = sharded.find_votes(hp);
            std::printf("one %s %.9g %lld\nsharded %s %.9g %lld\n", a.filename.c_str(), (double)a.cnt, (long long)a.offset,
                        b.filename.c_str(), (double)b.cnt, (long long)b.offset);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
"""


def test_cpp_find_votes_on_both_storages(tmp_path, filters, torch_cuda):
    """GpuStorage::find_votes (the host function on one handle) and ShardedGpuStorage{0, 0}::find_votes (two shards) print
    the same name, count and offset for the end-to-end queries"""
    _, song_files, query_files = _songs_and_queries(tmp_path)
    src, exe = tmp_path / "votes.cpp", str(tmp_path / "votes")
    src.write_text(PROGRAM)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib_dir,
                        "-lhpfw_gpu_multi", "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    work = tmp_path / "run"
    _filter_cache(str(work / "cache"), filters)
    r = subprocess.run([exe, "--index"] + song_files + ["--search"] + query_files, cwd=str(work), capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, HPFW_PREPARE_KEEP_FILTERS="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    one, sharded = [ln.split()[1:] for ln in lines if ln.startswith("one ")], [ln.split()[1:] for ln in lines if ln.startswith("sharded ")]
    print(r.stdout)
    assert len(one) == len(query_files) and one == sharded
    assert [rec[0] for rec in one[:4]] == [f"song{c:02d}" for c, _ in STARTS]
