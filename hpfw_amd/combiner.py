"""AudioCombiner in Python: the reference's C++ class (include/hpfw/audioproblems/combiner/combiner.h:15-132) over the
GPU Mel front end, the uint16 hashprints of HashPrint<uint16_t, MelSpectrogram<>, 32, 50> and the exact-hash inverted
index with its offset votes (hpfw_amd/csrc/k_combiner.hip).

prepare(files)  = read the WAVs, learn the filters if none are set, hashprints per file
build(pairs)    = build_db (:90-97): recordings numbered in the order given
find(hp)        = find (:100-132) with the query's own recording given as `exclude` instead of its name
align(hp, k)    = per recording the most votes on one offset and the smallest such offset, k best recordings
combine(files)  = combine (:23-33): prints what the reference prints, returns the results

Beyond the reference: with keep_audio=True the offsets of align() -- hashprint columns, 441 samples --
are refined to the sample by the exact cross-correlation of the PCM (hpfw_amd/csrc/k_xcorr.hip):
refine(query, hits) = per hit the offset in samples, the polarity and the normalised peak of the correlation
place(n, edges)     = a spanning forest over pairwise offsets: every recording's start on its event's timeline (host only)
layout(...)         = align all against all, refine the best hit of every pair, place
"""
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib


class CombineResult(NamedTuple):
    """SearchResult of combiner.h:76-81; name "" and rec None when no event matched"""
    name: str
    rec: Optional[int]
    cnt: int
    confidence: int
    offset: int


class AlignHit(NamedTuple):
    name: str
    rec: int
    peak: int
    offset: int


class RefinedHit(NamedTuple):
    """query[n + offset_samples] ~ recording[n]; inverted: the two have opposite polarity; score: r / (|a| |b|) of the
    segment at the peak, in [-1, 1]; peak: the votes of the hit that was refined"""
    name: str
    rec: int
    offset_samples: int
    inverted: bool
    score: float
    peak: int


class Component(NamedTuple):
    """recordings of one event: members ascending, starts[k] the first sample of members[k] on the common timeline (the
    earliest is 0), inverted[k] its polarity against members[0], residuals (i, j, offset - (start_j - start_i)) of the
    edges the spanning tree did not use, strongest first"""
    members: Tuple[int, ...]
    starts: Tuple[int, ...]
    inverted: Tuple[bool, ...]
    residuals: Tuple[Tuple[int, int, int], ...]


def place(n_rec: int, edges) -> List[Component]:
    """edges (i, j, offset_samples, score, inverted): start_j = start_i + offset.  The edges sorted by (|score| desc, i, j)
    grow a spanning forest (union-find: an edge inside a tree is not used); per tree the starts follow the tree's edges
    from its lowest id.  Components by their lowest id; the result does not depend on the order of `edges`."""
    es = sorted(((int(i), int(j), int(off), float(sc), bool(inv)) for i, j, off, sc, inv in edges),
                key=lambda e: (-abs(e[3]), e[0], e[1], e[2], e[4], e[3]))
    for i, j, _, sc, _ in es:
        if not (0 <= i < n_rec and 0 <= j < n_rec) or i == j or sc != sc:
            raise ValueError(f"place: bad edge ({i}, {j}) of {n_rec} recordings")
    parent = list(range(n_rec))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    adj = [[] for _ in range(n_rec)]
    rest = []
    for e in es:
        i, j, off, _, inv = e
        a, b = root(i), root(j)
        if a == b:
            rest.append(e)
            continue
        parent[max(a, b)] = min(a, b)
        adj[i].append((j, off, inv))
        adj[j].append((i, -off, inv))
    start, pol, comp = [0] * n_rec, [False] * n_rec, [-1] * n_rec
    out = []
    for first in range(n_rec):
        if comp[first] >= 0:
            continue
        comp[first] = len(out)
        members, todo = [first], [first]
        while todo:
            x = todo.pop()
            for y, off, inv in adj[x]:
                if comp[y] < 0:
                    comp[y], start[y], pol[y] = len(out), start[x] + off, pol[x] != inv
                    members.append(y)
                    todo.append(y)
        members.sort()
        base = min(start[m] for m in members)
        out.append([tuple(members), tuple(start[m] - base for m in members), tuple(pol[m] for m in members), []])
    for i, j, off, _, _ in rest:
        out[comp[i]][3].append((i, j, off - (start[j] - start[i])))
    return [Component(m, s, p, tuple(r)) for m, s, p, r in out]


def refine_geometry(n_q: int, n_r: int, frames_q, frames_r, len_q: int, len_r: int, d: int, seg_len: int):
    """the segment of a hit with column offset d (query column - recording column) between a query of n_q columns and len_q
    samples and a recording of n_r columns and len_r samples: (D0, q, len), or None when the columns or the samples do not
    overlap.  o* = the middle column of the overlap, c* = o* + d, D0 = 441 (frame_q[c*] - frame_r[o*]); the segment is
    len = min(seg_len, sample overlap) samples of the recording centred on 441 frame_r[o*], clamped into the overlap."""
    o_lo, o_hi = max(0, -d), min(n_r, n_q - d)
    if o_lo >= o_hi:
        return None
    o = (o_lo + o_hi - 1) // 2
    d0 = 441 * (int(frames_q[o + d]) - int(frames_r[o]))
    s_lo, s_hi = max(0, -d0), min(len_r, len_q - d0)
    if s_lo >= s_hi:
        return None
    n = min(int(seg_len), s_hi - s_lo)
    q = min(max(441 * int(frames_r[o]) - n // 2, s_lo), s_hi - n)
    return d0, q, n


def xcorr_score(r, energy_a, energy_b) -> float:
    """r / (sqrt(energy_a) sqrt(energy_b)) in float64 -- the integers converted first, then exactly these operations -- or 0
    when an energy is 0"""
    ea, eb = float(int(energy_a)), float(int(energy_b))
    if ea == 0.0 or eb == 0.0:
        return 0.0
    return float(int(r)) / (math.sqrt(ea) * math.sqrt(eb))


class AudioCombiner:
    def __init__(self, device: int = 0, filters: Optional[np.ndarray] = None, resample: bool = False, keep_audio: bool = False):
        """resample: prepare() reads WAV files at any rate in [8 000, 192 000] Hz and converts them to 44.1 kHz on the GPU
        (off: 44.1 kHz only, as before).  keep_audio: prepare() keeps every file's mono 44.1 kHz PCM and the frames its
        hashprint columns came from on the host, for refine() and layout() (off: nothing is kept, as before)"""
        self._gpu = _lib.Gpu(device)
        self._resample = resample
        self._keep_audio = keep_audio
        self._audio = {}                                  # name -> (int16 PCM, int32 frame of every kept column)
        self._has_filters = False
        self.names: List[str] = []
        self._hp: List[np.ndarray] = []
        if filters is not None:
            self.set_filters(filters)

    def close(self):
        self._gpu.close()

    def set_filters(self, filters_colmajor):
        """16 x (33 * 32) floats, column-major (hpfw_gpu_cfg_set_filters)"""
        self._gpu.cfg_set_filters(_lib.COMBINER_CONFIG, filters_colmajor)
        self._has_filters = True

    def prepare(self, filenames: Sequence[str]) -> List[Tuple[str, np.ndarray]]:
        """(name, uint16 hashprints) per file, in the order given; learns the filters from these files if none are set"""
        pcm = [self._read(f) for f in filenames]
        if not self._has_filters:
            cfg = _lib.COMBINER_CONFIG
            self._gpu.cfg_cov_reset(cfg)
            for x in pcm:
                if x.size:                               # an empty file adds nothing (and gets no hashprints)
                    self._gpu.mel_cov_accumulate(x)
            self._gpu.cfg_learn_filters(cfg)             # installs them
            self._has_filters = True
        if self._keep_audio:
            for f, x in zip(filenames, pcm):
                self._audio[f] = (x, self._gpu.mel_kept_frames(x)[0] if x.size else np.zeros(0, np.int32))
        return [(f, self._gpu.mel_hashprints(x)[0] if x.size else np.zeros(0, np.uint16)) for f, x in zip(filenames, pcm)]

    def _read(self, filename):
        return _lib.read_wav_44k(self._gpu, filename, self._resample)

    def build(self, pairs: Sequence[Tuple[str, np.ndarray]]):
        names = [name for name, _ in pairs]
        if len(set(names)) != len(names):
            raise ValueError("AudioCombiner: duplicate recording names (the reference keys its votes by name)")
        self._gpu.combiner_clear()
        self.names = names
        self._hp = [np.ascontiguousarray(hp, np.uint16) for _, hp in pairs]
        if pairs:
            self._gpu.combiner_add(self._hp)

    def _rec(self, exclude):
        if exclude is None:
            return -1
        if isinstance(exclude, str):
            return self.names.index(exclude) if exclude in self.names else -1
        return int(exclude)

    def find_many(self, hps: Sequence[np.ndarray], exclude=None) -> List[CombineResult]:
        ex = [-1] * len(hps) if exclude is None else [self._rec(e) for e in exclude]
        out = self._gpu.combiner_find(list(hps), ex)
        return [CombineResult(self.names[int(r["rec"])] if r["rec"] != _lib.NO_REC else "",
                              None if r["rec"] == _lib.NO_REC else int(r["rec"]),
                              int(r["cnt"]), int(r["confidence"]), int(r["offset"])) for r in out]

    def find(self, hp: np.ndarray, exclude=None) -> CombineResult:
        """exclude: a recording id or name (the query's own recording), None for none"""
        return self.find_many([hp], None if exclude is None else [exclude])[0]

    def align_many(self, hps: Sequence[np.ndarray], k: int, exclude=None) -> List[List[AlignHit]]:
        ex = [-1] * len(hps) if exclude is None else [self._rec(e) for e in exclude]
        out = self._gpu.combiner_align(list(hps), k, ex)
        return [[AlignHit(self.names[int(h["rec"])], int(h["rec"]), int(h["peak"]), int(h["offset"]))
                 for h in row if h["rec"] != _lib.NO_REC] for row in out]

    def align(self, hp: np.ndarray, k: int, exclude=None) -> List[AlignHit]:
        return self.align_many([hp], k, None if exclude is None else [exclude])[0]

    # ---- sample-accurate offsets ------------------------------------------------------------
    def _refine_pairs(self, pairs, seg_len, radius):
        """pairs (query id, AlignHit): one RefinedHit each, all in one call of the exact cross-correlation.  Only the two
        slices a job reads are packed and uploaded."""
        if not self._keep_audio:
            raise ValueError("AudioCombiner: refine needs keep_audio=True")
        if not (1 <= seg_len <= _lib.XCORR_MAX_LEN and 0 <= radius <= _lib.XCORR_MAX_RADIUS):
            raise ValueError("AudioCombiner: seg_len in 1 .. 2^22 and radius in 0 .. 4096")
        slices, jobs, geo, at = [], [], [], 0
        for qi, hit in pairs:
            xq, fq = self._audio[self.names[qi]]
            xr, fr = self._audio[self.names[hit.rec]]
            g = refine_geometry(self._hp[qi].size, self._hp[hit.rec].size, fq, fr, xq.size, xr.size, hit.offset, seg_len)
            geo.append(g)
            if g is None:
                continue
            d0, q, n = g
            p = q + d0
            a0, a1 = max(0, p - radius), min(xq.size, p + radius + n)    # what of the query the lags can reach
            a1 = max(a1, a0)
            slices += [xq[a0:a1], xr[q:q + n]]
            jobs.append((at, a1 - a0, at + (a1 - a0), n, p - a0, 0, n, radius, 0))
            at += (a1 - a0) + n
        peaks = iter(self._gpu.xcorr(np.concatenate(slices), np.array(jobs, _lib.XCORR_JOB_DTYPE)) if jobs else ())
        out = []
        for (qi, hit), g in zip(pairs, geo):
            if g is None:                                 # nothing to correlate: the hit as it is, score 0
                out.append(RefinedHit(hit.name, hit.rec, 441 * hit.offset, False, 0.0, hit.peak))
                continue
            pk = next(peaks)
            out.append(RefinedHit(hit.name, hit.rec, g[0] + int(pk["lag"]), bool(pk["r"] < 0),
                                  xcorr_score(pk["r"], pk["energy_a"], pk["energy_b"]), hit.peak))
        return out

    def refine(self, query, hits: Sequence[AlignHit], seg_len: int = 1 << 18, radius: int = 1024) -> List[RefinedHit]:
        """query: the id or name of an indexed recording, hits: what align() gave for its hashprints.  Per hit the offset in
        samples, query[n + offset_samples] ~ recording[n]: the hit's column offset mapped to samples through the kept frames
        of both, then moved to the largest |r| of the exact cross-correlation of a segment of seg_len samples over lags
        -radius .. radius"""
        qi = self.names.index(query) if isinstance(query, str) else int(query)
        return self._refine_pairs([(qi, h) for h in hits], seg_len, radius)

    def layout(self, min_peak: int, min_score: float, k: int = 8, seg_len: int = 1 << 18, radius: int = 1024) -> List[Component]:
        """every indexed recording on the timeline of its event: align all against all (k best each), per unordered pair the hit
        with the larger peak (ties: the smaller query id), those with peak >= min_peak refined, those with |score| >= min_score
        placed (place()).  min_peak and min_score depend on the material: there are no defaults."""
        pairs = self._layout_pairs(min_peak, k)
        refined = self._refine_pairs(pairs, seg_len, radius) if pairs else []
        edges = [(qi, r.rec, r.offset_samples, r.score, r.inverted) for (qi, _), r in zip(pairs, refined) if abs(r.score) >= min_score]
        return place(len(self.names), edges)

    def _layout_pairs(self, min_peak, k):
        """(query id, AlignHit) per unordered pair of recordings with a hit of peak >= min_peak: the hit with the larger peak"""
        n = len(self.names)
        best = {}
        for qi, hits in enumerate(self.align_many(self._hp, k, list(range(n))) if n else []):
            for h in hits:
                key = (min(qi, h.rec), max(qi, h.rec))
                if key not in best or h.peak > best[key][1].peak:      # (queries ascend: a tie keeps the smaller id)
                    best[key] = (qi, h)
        return [best[key] for key in sorted(best) if best[key][1].peak >= min_peak]

    def combine(self, filenames: Sequence[str]) -> List[CombineResult]:
        """combiner.h:23-33: index the files unless an index exists, then find every file with itself excluded"""
        filenames = list(filenames)
        if not self.names:
            self.build(self.prepare(filenames))
        known = {n: i for i, n in enumerate(self.names)}
        missing = [f for f in filenames if f not in known]
        extra = dict(self.prepare(missing)) if missing else {}
        hps = [self._hp[known[f]] if f in known else extra[f] for f in filenames]
        res = self.find_many(hps, [known.get(f, -1) for f in filenames])
        for f, r in zip(filenames, res):
            print(f"FINDING {f}")
            print(f"{r.name} {r.cnt} {r.confidence} {r.offset}")
            print()
        return res
