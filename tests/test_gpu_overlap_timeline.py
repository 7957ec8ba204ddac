"""The scored overlap search, and timeline() and streams() under the overlap rule, on the GPU.  Every
search case runs under both kernel selections; the moments are compared integer for integer with the restatement of
tests/overlap_score_ref.py, the hits byte for byte with search_overlap of the same build."""
import math
import os

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import overlap_ref
import overlap_score_ref as ref
import timeline_ref

pytestmark = pytest.mark.gpu
WIN, HOP = 220500, 110250
_REF = {}                                                # references computed once, shared by both kernel selections


@pytest.fixture(params=["mfma", "popcount"])
def kernel(request):
    if request.param == "popcount":
        os.environ["HPFW_OVERLAP_POPC"] = "1"
    yield request.param
    os.environ.pop("HPFW_OVERLAP_POPC", None)


@pytest.fixture(scope="module")
def ov(torch_cuda):
    """a handle of this file's own: the searches need no filters, and the session's handle keeps its index"""
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


def _rand(n, seed):
    return np.random.default_rng([0x6F766C70, seed]).integers(0, 2 ** 64, n, dtype=np.uint64)


def _index(g, clips):
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    g.index_clear()
    g.index_set_clip_base(0)
    g.index_add(db_hp, db_off)
    return db_hp, db_off


def _splits(value):
    if value is None:
        os.environ.pop("HPFW_OVERLAP_SPLITS", None)
    else:
        os.environ["HPFW_OVERLAP_SPLITS"] = value


def _moments(stats):
    return [(int(r["n"]), int(r["sum"]), int(r["sum_sq"])) for r in stats]


# ---- 1. the moments are exact -------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 5, 63, 64, 143, 304, 305, 1023, 1024, 1025, 2320, 3000]     # the ragged index of test_gpu_overlap.py
Q_LENGTHS = [1, 64, 143, 304, 305, 1000]
EXCLUDE = [11, 0, 5, -1, 12, 3]                           # clip 0 is empty: it never has a candidate


def _ragged_case():
    if "ragged" not in _REF:
        clips = [_rand(n, 100 + i) for i, n in enumerate(LENGTHS)]
        queries = [_rand(k, 200 + i) for i, k in enumerate(Q_LENGTHS)]
        queries[3][:] = clips[11][1000:1304] ^ np.uint64(0x0000100000400001)   # (one query that belongs somewhere)
        dists = {(qi, c): overlap_ref.lag_dists(q, r) for qi, q in enumerate(queries) for c, r in enumerate(clips)}
        cands = {}
        for mo in sorted({1, 64, 100} | set(Q_LENGTHS)):
            for qi, q in enumerate(queries):
                cands[mo, qi] = [overlap_ref.clip_candidate_fast(q, r, mo, dists[qi, c]) for c, r in enumerate(clips)]
        _REF["ragged"] = (clips, queries, cands)
    return _REF["ragged"]


def test_moments_are_exact(ov, kernel):
    clips, queries, cands = _ragged_case()
    _index(ov, clips)
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    for mo in (1, 64, 100):
        want = [ref.row_moments(cands[mo, qi]) for qi in range(len(queries))]
        assert [w[0] for w in want] == [sum(n >= mo for n in LENGTHS) if kq >= mo else 0 for kq in Q_LENGTHS]
        for k in (1, 10):
            for splits in ((None, "1", "3") if (mo, k) == (100, 1) else (None,)):   # the clips of 2320 and 3000 have seams
                _splits(splits)
                try:
                    hits, stats = ov.search_overlap_scored(q_hp, q_off, k, mo)
                    plain = ov.search_overlap(q_hp, q_off, k, mo)
                finally:
                    _splits(None)
                assert hits.tobytes() == plain.tobytes(), (mo, k, splits)
                assert _moments(stats) == want, (mo, k, splits)
                assert (stats["pad"] == 0).all()
        for qi in range(len(queries)):                    # the best hit and its score equal the restatement's
            best = ref.best_clip(cands[mo, qi])
            if best is None:
                assert hits[qi, 0]["clip"] == _lib.NO_CLIP
                continue
            c, (dist, L, lag) = best
            assert tuple(int(v) for v in hits[qi, 0]) == (dist, c, lag, L)
            s = timeline_ref.hit_score(ref.rate(dist, L), True, *want[qi])
            got = _lib.hit_score(_lib.overlap_rate(dist, L), True, stats[qi])
            assert (math.isnan(s) and math.isnan(got)) or abs(got - s) <= 1e-12 * abs(s), (mo, qi, got, s)
        # an exclude list: the excluded clip is not counted; excluding a clip without a candidate changes nothing
        want_ex = [ref.row_moments(cands[mo, qi], EXCLUDE[qi]) for qi in range(len(queries))]
        hits, stats = ov.search_overlap_scored(q_hp, q_off, 10, mo, exclude=EXCLUDE)
        assert hits.tobytes() == ov.search_overlap(q_hp, q_off, 10, mo, exclude=EXCLUDE).tobytes()
        assert _moments(stats) == want_ex, mo
        assert want_ex[1] == want[1] and want_ex[3] == want[3]
        if mo == 64:
            assert want_ex[4][0] == want[4][0] - 1 and want_ex[0] == want[0] == (0, 0, 0)
    for qi, kq in enumerate(Q_LENGTHS):                   # min_overlap = the query's length: one query per call
        for k in (1, 10):
            hits, stats = ov.search_overlap_scored(queries[qi], np.array([0, kq], np.int64), k, kq)
            assert hits.tobytes() == ov.search_overlap(queries[qi], np.array([0, kq], np.int64), k, kq).tobytes()
            assert _moments(stats) == [ref.row_moments(cands[kq, qi])], (qi, k)


def test_empty_inputs(ov, kernel):
    q_hp, q_off = _lib._ragged([_rand(304, 1), _rand(5, 2)], np.uint64)
    ov.index_clear()
    hits, stats = ov.search_overlap_scored(q_hp, q_off, 3, 4)
    assert (hits["clip"] == _lib.NO_CLIP).all() and _moments(stats) == [(0, 0, 0)] * 2        # an empty index
    _index(ov, [_rand(400, 3), _rand(0, 4), _rand(3, 5), _rand(9, 6)])
    hits, stats = ov.search_overlap_scored(q_hp, q_off, 3, 6)
    assert [m[0] for m in _moments(stats)] == [2, 0]                                          # a query below min_overlap
    hits, stats = ov.search_overlap_scored(np.zeros(1, np.uint64), np.zeros(3, np.int64), 2, 1)
    assert (hits["clip"] == _lib.NO_CLIP).all() and _moments(stats) == [(0, 0, 0)] * 2        # empty queries
    hits, stats = ov.search_overlap_scored(np.zeros(1, np.uint64), np.zeros(1, np.int64), 2, 1)
    assert hits.shape == (0, 2) and stats.shape == (0,)


# ---- 2. row slices and query groups ---------------------------------------------------------------------------------------------
N_TINY, N_TINY_Q = 8200, 100


def test_row_slices_and_query_groups(ov, kernel):
    """8 200 clips of 8 hashprints: the stats kernel cuts a row into 8200 // 4096 = 2 slices, and with 64 splits a group of
    the host loop holds 2^26 // (8200 * 64) // 32 * 32 = 96 queries, so that 100 queries take two groups"""
    assert min(64, N_TINY // 4096) == 2 and (1 << 26) // (N_TINY * 64) // 32 * 32 == 96 < N_TINY_Q
    if "tiny" not in _REF:
        db = _rand(N_TINY * 8, 900).reshape(N_TINY, 8)
        queries = _rand(N_TINY_Q * 8, 901).reshape(N_TINY_Q, 8)
        for i in range(0, N_TINY_Q, 3):                   # a third of the queries overlap a clip, shifted by i % 5 - 2
            s = i % 5 - 2
            c = db[(i * 83) % N_TINY]
            queries[i, max(0, -s):8 - max(0, s)] = c[max(0, s):8 - max(0, -s)]
        rows = ref.tiny_rows(db, queries, 4)
        rng = np.random.default_rng(902)
        for qi, c in zip(rng.integers(0, N_TINY_Q, 50), rng.integers(0, N_TINY, 50)):
            assert (int(rows[qi][0][c]), int(rows[qi][1][c]), int(rows[qi][2][c])) == overlap_ref.clip_candidate(queries[qi], db[c], 4)
        _REF["tiny"] = (db, queries, [ref.tiny_moments(r) for r in rows], [ref.tiny_best(r) for r in rows])
    db, queries, want, best = _REF["tiny"]
    ov.index_clear()
    ov.index_set_clip_base(0)
    ov.index_add(db.ravel(), np.arange(N_TINY + 1, dtype=np.int64) * 8)
    q_off = np.arange(N_TINY_Q + 1, dtype=np.int64) * 8
    exclude = np.full(N_TINY_Q, -1, np.int32)
    exclude[97] = best[97][1]                             # a query of the second group leaves its best clip out
    _splits("64")
    try:
        hits, stats = ov.search_overlap_scored(queries.ravel(), q_off, 2, 4)
        plain = ov.search_overlap(queries.ravel(), q_off, 2, 4)
        hits_ex, stats_ex = ov.search_overlap_scored(queries.ravel(), q_off, 2, 4, exclude=exclude)
    finally:
        _splits(None)
    assert hits.tobytes() == plain.tobytes()
    assert [tuple(int(v) for v in h) for h in hits[:, 0]] == best
    got = _moments(stats)
    assert all(m[0] == N_TINY for m in got)
    bad = [qi for qi in range(N_TINY_Q) if got[qi] != want[qi]]
    assert not bad, (bad[:5], got[bad[0]], want[bad[0]])
    r = ref.rate(best[97][0], best[97][3])
    assert _moments(stats_ex)[97] == (N_TINY - 1, want[97][1] - r, want[97][2] - r * r) and hits_ex[97, 0]["clip"] != best[97][1]
    assert _moments(stats_ex)[:97] == want[:97] and _moments(stats_ex)[98:] == want[98:]
    assert [int(best[i][2]) for i in range(0, 15, 3)] == [(i % 5 - 2) for i in range(0, 15, 3)] and best[0][0] == 0


# ---- 3. device pointers on a side stream ----------------------------------------------------------------------------------------
def test_device_pointers_on_a_side_stream(ov, kernel, torch_cuda):
    torch = torch_cuda
    clips = _ragged_case()[0]
    _index(ov, clips)
    queries = [_rand(k, 700 + i) for i, k in enumerate([304, 64, 0, 305, 143] * 8)]
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    exclude = np.array([(i % 14) - 1 for i in range(len(queries))], np.int32)
    want_hits, want_stats = ov.search_overlap_scored(q_hp, q_off, 4, 64, exclude=exclude)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_q = torch.from_numpy(q_hp.view(np.int64)).cuda()
        d_out = torch.zeros(len(queries) * 4 * 16, dtype=torch.uint8, device="cuda")
        d_stats = torch.full((len(queries) * 24,), 0xAB, dtype=torch.uint8, device="cuda")   # (the call zeroes the rows itself)
        ov.search_overlap_scored_dev(d_q.data_ptr(), q_off, 4, 64, d_out.data_ptr(), d_stats.data_ptr(), exclude=exclude,
                                     stream=side.cuda_stream)
    side.synchronize()
    assert d_out.cpu().numpy().tobytes() == want_hits.tobytes()
    assert d_stats.cpu().numpy().tobytes() == want_stats.tobytes()
    assert (want_stats["n"] > 0).any() and (want_stats["n"][2::5] == 0).all()


# ---- 4. and 5. concert (C) end to end -------------------------------------------------------------------------------------------
STRONG, WEAK = [0, 1, 2, 3, 5] + list(range(7, 15)), [4, 6, 15, 16]
# (clip, first window, last window, from, to in seconds) and the lags by geometry: 80.6 columns a second
SEGMENTS = [(2, 0, 3, 1.5, 11.5), (6, 5, 5, 13.0, 16.0), (4, 7, 10, 18.5, 28.5), (1, 11, 14, 28.5, 38.5)]
COL_S = 5.0 / 403.0


def _lsi(filters):
    """an identifier whose collector holds the filter fixture and whose index holds songs 0-5 and the item"""
    songs, item, names = ref.concert_c_index()
    lsi = hpfw_amd.LiveSongIdentification()
    ext = lsi.collector.gpu()
    ext.set_filters(filters)
    hp = list(ext.extract(songs)) + [ext.extract(item[None])[0]]
    lsi.build(list(zip(hp, names)))
    return lsi, hp, names


def _concert_reference(oracle, filters):
    """the restatement over oracle hashprints: per window (clip, dist, lag, overlap, score), lo, hi"""
    if "concert" not in _REF:
        songs, item, _ = ref.concert_c_index()
        idx = list(oracle.Plan(songs.shape[1]).extract_batch(filters, songs, 16)) + [oracle.Plan(item.size).extract(filters, item)]
        x = ref.concert_c()
        w_hp = oracle.Plan(WIN).extract_batch(filters, timeline_ref.windows_of(x, WIN, HOP), 16)
        db_hp, db_off = _lib._ragged(idx, np.uint64)
        rows = [ref.search_scored(db_hp, db_off, q, 100) for q in w_hp]
        _REF["concert"] = (x, idx, [(c, d, lag, L, s) for c, d, lag, L, _, s in rows])
    return _REF["concert"]


def test_timeline_of_concert_c(tmp_path, filters, oracle, torch_cuda, kernel):
    """concert (C): song 2, the item, song 4 and song 1 whole between stretches outside the index.  The restated scores of the
    windows that must be strong are at least 16.01 (lo), those of windows 4, 6, 15 and 16 at most 3.77 (hi): min_score is
    their geometric mean"""
    x, idx, want = _concert_reference(oracle, filters)
    lo, hi = min(want[w][4] for w in STRONG), max(want[w][4] for w in WEAK)
    print(f"lo {lo:.3f} hi {hi:.3f} ratio {lo / hi:.3f}")
    assert lo / hi >= 1.5
    min_score = math.sqrt(lo * hi)
    path = str(tmp_path / "concert_c.wav")
    synth.write_wav(path, x)
    lsi, hp, names = _lsi(filters)
    try:
        assert [h.size for h in hp] == [707] * 6 + [143] and all(np.array_equal(a, b) for a, b in zip(hp, idx))
        segs, wins = lsi.timeline(path, min_score, windows=True, min_overlap=100)
        assert len(wins) == 17 == len(want)
        rows = []
        for w, (row, (c, d, lag, L, s)) in enumerate(zip(wins, want)):
            print(f"window {w:2d}: clip {row[0]} dist {row[2]} lag {row[3]} overlap {row[7]} score {row[4]:.3f}")
            assert len(row) == 8 and (row[0], row[2], row[3], row[7]) == (c, d, lag, L) and row[1] == names[c] and row[5:7] == (0, 1.0), (w, row, want[w])
            assert abs(row[4] - s) <= 1e-12 * abs(s), (w, row[4], s)
            rows.append((c, lag, 0, 1.0, s))
        for clip, first, last, t0, _ in SEGMENTS:          # the lags by geometry, to within 2 columns
            for w in range(first, last + 1):
                assert want[w][0] == clip and abs(want[w][2] - (w * 2.5 - t0) / COL_S) <= 2, (w, want[w])
        assert (want[0][3], want[3][3], want[5][3]) == (183, 223, 143)
        g = lsi._gpu.geometry(WIN)
        assert (g.c, g.n_hp) == (403, 304)
        want_segs = timeline_ref.segments(rows, min_score, HOP * g.m / (3.0 * WIN), WIN, HOP)
        assert [(s["clip"], s["first"], s["last"]) for s in want_segs] == [s[:3] for s in SEGMENTS]
        assert len(segs) == len(want_segs)
        clip_len = [h.size for h in idx]
        for got, s, (clip, first, last, t0, t1) in zip(segs, want_segs, SEGMENTS):
            a, b, first_lag = ref.trimmed(s, rows, clip_len, 304, 100, WIN, HOP, g.m)
            assert got[:3] == (a / synth.SR, b / synth.SR, names[clip]) and got[5:] == (0, 1.0), (got, s)
            assert abs(got[3] - s["best_score"]) <= 1e-12 * s["best_score"]
            assert first_lag == 0 == got[4]                 # each begins inside its first window: played from its start
            assert abs(got[0] - t0) <= 4 * COL_S and abs(got[1] - t1) <= 4 * COL_S, (got, t0, t1)
        # the plain rule: the item is shorter than a window, so it is never counted and no segment names it
        plain = lsi.timeline(path, min_score)
        assert all(name != "item" for _, _, name, *_ in plain)
        # refusals, each before anything runs
        for kw, status in ((dict(shifts=[0, 2]), _lib.E_UNSUPPORTED), (dict(tempos=[1.0, 1.04]), _lib.E_UNSUPPORTED)):
            with pytest.raises(hpfw_amd.HpfwError) as e:
                lsi.timeline(path, min_score, min_overlap=100, **kw)
            assert e.value.status == status
        for mo in (305, 0, -1):
            for call in (lambda: lsi.timeline(path, min_score, min_overlap=mo), lambda: lsi.streams(2, min_score, min_overlap=mo)):
                with pytest.raises(hpfw_amd.HpfwError) as e:
                    call()
                assert e.value.status == _lib.E_INVALID
        sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
        sharded._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
        for call in (lambda: sharded.timeline(path, min_score, min_overlap=100), lambda: sharded.streams(2, min_score, min_overlap=100),
                     lambda: sharded.top_overlap([path], 1, 100)):
            with pytest.raises(hpfw_amd.HpfwError) as e:
                call()
            assert e.value.status == _lib.E_UNSUPPORTED
        assert lsi.timeline(path, min_score, min_overlap=304) is not None     # the window's own length is the largest allowed
    finally:
        lsi._gpu.close()


FACADE = r"""
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/live_streams.h>
using Storage = hpfw::db::GpuStorage<hpfw::GpuCollector>;
static void print(const char *tag, int feed, const hpfw::TimelineSegment &s)
{
    std::printf("%s %d %s %.17g %.17g %.17g %.17g\n", tag, feed, s.filename.c_str(), s.start_s, s.end_s, s.score, s.offset_s);
}
template <typename F>
static int refused(F f)
{
    try {
        f();
    } catch (const std::runtime_error &) {
        return 1;
    }
    return 0;
}
int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    Storage storage;
    storage.load(argv[1]);
    std::vector<float> filters((size_t)HPFW_FILTERS * HPFW_FRAME_SIZE);
    std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char *>(filters.data()), (std::streamsize)(filters.size() * 4));
    if (hpfw_gpu_set_filters(storage.handle(), filters.data()) != 0) return 3;
    hpfw::LiveStreamsOptions opt;
    opt.min_score = std::atof(argv[4]);
    opt.min_overlap = 100;
    opt.keep_windows = true;
    const hpfw::Timeline t = hpfw::timeline(storage, storage.handle(), argv[3], opt);
    for (size_t w = 0; w < t.windows.size(); ++w)
        std::printf("W 0 %zu %u %d %u %.17g\n", w, t.windows[w].clip, t.windows[w].offset, t.overlaps[w], t.windows[w].score);
    for (const auto &s : t.segments) print("S", 0, s);
    int64_t n = 0;
    if (hpfw_gpu_wav_read_pcm16(argv[3], nullptr, 0, &n) != 0) return 4;
    std::vector<int16_t> pcm((size_t)n);
    if (hpfw_gpu_wav_read_pcm16(argv[3], pcm.data(), n, &n) != 0) return 4;
    hpfw::LiveStreams<Storage> live(storage, storage.handle(), 2, opt);
    const int64_t sizes[2] = {100003, 35797};
    int64_t at[2] = {0, 0};
    while (at[0] < n || at[1] < n) {
        std::vector<hpfw::LiveChunk> chunks;
        for (int f = 0; f < 2; ++f) {
            const int64_t m = std::min(sizes[f], n - at[f]);
            if (m > 0) chunks.push_back({f, pcm.data() + at[f], m});
            at[f] += m;
        }
        for (const auto &s : live.push(chunks)) print("L", s.feed, s.segment);
        for (const auto &w : live.windows()) std::printf("V %d %lld %u %d\n", w.feed, (long long)w.window, w.hit.clip, w.hit.offset);
    }
    for (const auto &s : live.finish()) print("L", s.feed, s.segment);
    hpfw::TimelineOptions bad = opt;
    int r = 0;
    bad.shifts = {0, 2};
    r += refused([&] { hpfw::timeline(storage, storage.handle(), argv[3], bad); });
    bad.shifts.clear();
    bad.tempos = {1.0f, 1.04f};
    r += refused([&] { hpfw::timeline(storage, storage.handle(), argv[3], bad); });
    bad.tempos.clear();
    bad.min_overlap = 305;
    r += refused([&] { hpfw::timeline(storage, storage.handle(), argv[3], bad); });
    hpfw::LiveStreamsOptions bad_live = opt;
    bad_live.min_overlap = 305;
    r += refused([&] { hpfw::LiveStreams<Storage> x(storage, storage.handle(), 2, bad_live); });
    std::printf("R %d\n", r);
    return 0;
}
"""


def test_cpp_facades_on_concert_c(tmp_path, filters, oracle, torch_cuda):
    """hpfw::timeline and hpfw::LiveStreams under TimelineOptions::min_overlap give the windows and segments of the Python
    ones, number for number; the program is what this test is about"""
    import subprocess
    x, _, want = _concert_reference(oracle, filters)
    min_score = math.sqrt(min(want[w][4] for w in STRONG) * max(want[w][4] for w in WEAK))
    path = str(tmp_path / "concert_c.wav")
    synth.write_wav(path, x)
    lsi, hp, names = _lsi(filters)
    try:
        want_segs, want_wins = lsi.timeline(path, min_score, windows=True, min_overlap=100)
    finally:
        lsi._gpu.close()
    with open(tmp_path / "dump.cereal", "wb") as f:       # GpuStorage::load: count, then per clip the name and the hashprints
        f.write(np.uint64(len(names)).tobytes())
        for name, h in zip(names, hp):
            f.write(np.uint64(len(name)).tobytes() + name.encode() + np.uint64(h.size).tobytes() + np.ascontiguousarray(h, np.uint64).tobytes())
    np.ascontiguousarray(filters, np.float32).tofile(tmp_path / "filters.f32")
    src = tmp_path / "facade.cpp"
    src.write_text(FACADE)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "facade"),
           "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "facade"), str(tmp_path / "dump.cereal"), str(tmp_path / "filters.f32"), path, repr(min_score)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines()]

    def same(a, b):
        return a == b or (math.isnan(a) and math.isnan(b))

    wins = [ln for ln in lines if ln[0] == "W"]
    assert len(wins) == 17
    for ln, row in zip(wins, want_wins):
        assert (int(ln[3]), int(ln[4]), int(ln[5])) == (row[0], row[3], row[7]) and same(float(ln[6]), row[4]), (ln, row)
    for tag, feed in (("S", 0), ("L", 0), ("L", 1)):
        got = [(float(ln[3]), float(ln[4]), ln[2], float(ln[5]), float(ln[6])) for ln in lines if ln[0] == tag and int(ln[1]) == feed]
        assert got == [s[:5] for s in want_segs], (tag, feed, got, want_segs)
    for feed in (0, 1):
        live = [(int(ln[2]), int(ln[3]), int(ln[4])) for ln in lines if ln[0] == "V" and int(ln[1]) == feed]
        assert live == [(w, row[0], row[3]) for w, row in enumerate(want_wins)]
    assert ["R", "4"] in lines


def test_streams_of_concert_c(tmp_path, filters, oracle, torch_cuda, kernel):
    """concert (C) pushed into two feeds in chunks of odd sizes: per feed exactly the windows and segments of timeline()"""
    x, _, want = _concert_reference(oracle, filters)
    min_score = math.sqrt(min(want[w][4] for w in STRONG) * max(want[w][4] for w in WEAK))
    path = str(tmp_path / "concert_c.wav")
    synth.write_wav(path, x)
    lsi, _, _ = _lsi(filters)
    try:
        want_segs, want_wins = lsi.timeline(path, min_score, windows=True, min_overlap=100)
        assert len(want_segs) == 4 and len(want_wins) == 17
        segs, wins = {0: [], 1: []}, {0: [], 1: []}
        with lsi.streams(2, min_score, windows=True, min_overlap=100) as live:
            at, sizes = [0, 0], [100003, 35797]            # (odd, below a window; the second feed lags behind the first)
            while min(at) < x.size:
                chunks = {f: x[at[f]:at[f] + sizes[f]] for f in (0, 1) if at[f] < x.size}
                at = [min(at[f] + sizes[f], x.size) for f in (0, 1)]
                new, rows = live.push(chunks)
                for f, w, row in rows:
                    assert w == len(wins[f])
                    wins[f].append(row)
                for f, sg in new:
                    segs[f].append(sg)
            assert live.open()[0] is None                   # the last song ended 6.5 s before the feed did
            for f, sg in live.finish():
                segs[f].append(sg)
            assert all(not lags for lags in live._lags)
        for f in (0, 1):
            assert len(wins[f]) == 17
            for got, w in zip(wins[f], want_wins):
                assert got[:4] == w[:4] and got[5:] == w[5:] and (got[4] == w[4] or (math.isnan(got[4]) and math.isnan(w[4]))), (f, got, w)
            assert segs[f] == want_segs, (f, segs[f], want_segs)
    finally:
        lsi._gpu.close()
