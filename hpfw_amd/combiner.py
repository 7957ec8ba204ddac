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

For recorders whose clocks differ, and for the audio of the event (hpfw_amd/csrc/k_warp.hip):
refine_drift(query, hits, min_score) = per hit offset and drift: a chain of short anchors outward, a Theil-Sen line
place_affine(n, edges)               = the same forest with affine maps composed along it (host only)
layout_drift(...)                    = align all against all, refine_drift the best hit of every pair, place_affine
render(component)                    = the mix of a component's members on its clock, or every member's track
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


class DriftHit(NamedTuple):
    """query[n + offset + drift n] ~ recording[n] with drift = drift_ppm 1e-6: the Theil-Sen line through the lags of the
    used anchors.  inverted: the polarity of the used anchors (the centre's when it is used, else the majority's); score: the
    median |score| of the used anchors; anchors: how many were correlated, used: how many of them had |score| >= min_score;
    rms: of the used lags against the line, in samples"""
    name: str
    rec: int
    offset: float
    drift_ppm: float
    inverted: bool
    score: float
    anchors: int
    used: int
    rms: float


class WarpedComponent(NamedTuple):
    """recordings of one event whose clocks differ: sample n of members[k] sits at starts[k] + rates[k] n on the clock of the
    lowest id (the earliest start is 0), inverted[k] its polarity against members[0]; residuals (i, j, samples, ppm) of the
    edges the spanning tree did not use, strongest first: the edge's offset against the placement's at the centre of the
    pair's overlap (at the recording's sample 0 when place_affine is not given the lengths), and its drift against it"""
    members: Tuple[int, ...]
    starts: Tuple[float, ...]
    rates: Tuple[float, ...]
    inverted: Tuple[bool, ...]
    residuals: Tuple[Tuple[int, int, float, float], ...]


def place_affine(n_rec: int, edges, lengths=None) -> List[WarpedComponent]:
    """edges (i, j, offset, drift, score, inverted): sample n of j sits at offset + (1 + drift) n of i.  The same forest as
    place() -- edges by (|score| desc, i, j), union-find, components by their lowest id -- with the affine maps composed in
    float64 along the tree from the lowest id, whose clock is the component's.  lengths: the recordings' lengths in samples,
    for the centre of an unused edge's overlap.  With all drifts 0 and integer offsets this is place()."""
    es = sorted(((int(i), int(j), float(off), float(dr), float(sc), bool(inv)) for i, j, off, dr, sc, inv in edges),
                key=lambda e: (-abs(e[4]), e[0], e[1], e[2], e[3], e[5], e[4]))
    for i, j, off, dr, sc, _ in es:
        if not (0 <= i < n_rec and 0 <= j < n_rec) or i == j or sc != sc or off != off or not abs(dr) < 0.5:
            raise ValueError(f"place_affine: bad edge ({i}, {j}) of {n_rec} recordings")
    parent = list(range(n_rec))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    adj = [[] for _ in range(n_rec)]
    rest = []
    for e in es:
        i, j, off, dr, _, inv = e
        a, b = root(i), root(j)
        if a == b:
            rest.append(e)
            continue
        parent[max(a, b)] = min(a, b)
        adj[i].append((j, off, dr, inv, True))
        adj[j].append((i, off, dr, inv, False))
    start, rate, pol, comp = [0.0] * n_rec, [1.0] * n_rec, [False] * n_rec, [-1] * n_rec
    out = []
    for first in range(n_rec):
        if comp[first] >= 0:
            continue
        comp[first] = len(out)
        members, todo = [first], [first]
        while todo:
            x = todo.pop()
            for y, off, dr, inv, forward in adj[x]:
                if comp[y] >= 0:
                    continue
                if forward:                              # y's sample n is x's sample off + (1 + dr) n
                    start[y], rate[y] = start[x] + rate[x] * off, rate[x] * (1.0 + dr)
                else:                                    # x's sample n is y's sample off + (1 + dr) n
                    rate[y] = rate[x] / (1.0 + dr)
                    start[y] = start[x] - rate[y] * off
                comp[y], pol[y] = len(out), pol[x] != inv
                members.append(y)
                todo.append(y)
        members.sort()
        base = min(start[m] for m in members)
        for m in members:
            start[m] -= base
        out.append([tuple(members), tuple(start[m] for m in members), tuple(rate[m] for m in members),
                    tuple(pol[m] for m in members), []])
    for i, j, off, dr, _, _ in rest:
        # the placement's map from j's samples to i's: (start_j + rate_j n - start_i) / rate_i
        p_off, p_rate = (start[j] - start[i]) / rate[i], rate[j] / rate[i]
        at = 0.0
        if lengths is not None:                          # the centre of the overlap, in j's samples
            lo, hi = max(0.0, -off / (1.0 + dr)), min(float(lengths[j]), (float(lengths[i]) - off) / (1.0 + dr))
            at = (lo + hi) / 2.0 if hi > lo else 0.0
        out[comp[i]][4].append((i, j, (off - p_off) + ((1.0 + dr) - p_rate) * at, ((1.0 + dr) - p_rate) * 1e6))
    return [WarpedComponent(m, s, r, p, tuple(res)) for m, s, r, p, res in out]


def _predict(trail, fallback, pos):
    """the lag expected at sample `pos`: on the line through the last two used anchors (pos, lag, ...) of `trail`, the last
    one's lag while there is one, `fallback` while there is none"""
    if not trail:
        return fallback
    if len(trail) == 1:
        return trail[-1][1]
    (n1, l1), (n2, l2) = trail[-2][:2], trail[-1][:2]
    return l2 + int(round((l2 - l1) * (pos - n2) / (n2 - n1)))


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
        self._device = int(device)
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

    # ---- clock drift and rendering ------------------------------------------------------------
    def _drift_pairs(self, pairs, min_score, anchor_len, anchor_hop, radius):
        """pairs (query id, AlignHit): one (DriftHit, the centre samples of its used anchors) each.  Anchor 0 of a pair is
        refine()'s job with seg_len = anchor_len; round t correlates the t-th anchor on each side of every pair in ONE call,
        around the lag the line through the last two used anchors of that side predicts (the last one's lag while there is
        one; an anchor below min_score is not used and the prediction carries over it).  A second pass correlates every anchor
        again with the query read on the recording's clock by the first pass's line; the result is the line of the second."""
        if not self._keep_audio:
            raise ValueError("AudioCombiner: refine_drift needs keep_audio=True")
        if not (1 <= anchor_len <= _lib.XCORR_MAX_LEN and 0 <= radius <= _lib.XCORR_MAX_RADIUS and anchor_hop >= 1):
            raise ValueError("AudioCombiner: anchor_len in 1 .. 2^22, anchor_hop >= 1 and radius in 0 .. 4096")
        chains = []                                       # per pair: None, or its audio, its anchors and what the rounds found
        for qi, hit in pairs:
            xq, fq = self._audio[self.names[qi]]
            xr, fr = self._audio[self.names[hit.rec]]
            g = refine_geometry(self._hp[qi].size, self._hp[hit.rec].size, fq, fr, xq.size, xr.size, hit.offset, anchor_len)
            if g is None:
                chains.append(None)
                continue
            d0, q, n = g
            centre, left, right = _lib.drift_anchors(max(0, -d0), min(xr.size, xq.size - d0), q, n, anchor_len, anchor_hop)
            # points: (centre sample of the anchor, lag, score, used), the centre anchor first; trail[side]: the used ones
            # of that side going outward, the centre included
            chains.append(dict(xq=xq, xr=xr, d0=d0, len=n, starts=((centre,), left, right), points=[], trail=([], [])))
        live = [c for c in chains if c is not None]
        rounds = max((max(len(c["starts"][1]), len(c["starts"][2])) for c in live), default=-1) + 1
        for t in range(rounds):
            todo = [(c, None, c["starts"][0][0]) for c in live] if t == 0 else \
                [(c, side, c["starts"][1 + side][t - 1]) for c in live for side in (0, 1) if t <= len(c["starts"][1 + side])]
            slices, jobs, guesses, at = [], [], [], 0
            for c, side, start in todo:
                n, xq = c["len"], c["xq"]
                guess = c["d0"] if side is None else _predict(c["trail"][side], c["d0"], start + n // 2)
                p = start + guess
                a0 = min(max(0, p - radius), xq.size)
                a1 = max(a0, min(xq.size, p + radius + n))
                slices += [xq[a0:a1], c["xr"][start:start + n]]
                jobs.append((at, a1 - a0, at + (a1 - a0), n, p - a0, 0, n, radius, 0))
                guesses.append(guess)
                at += (a1 - a0) + n
            if not jobs:
                continue
            peaks = self._gpu.xcorr(np.concatenate(slices), np.array(jobs, _lib.XCORR_JOB_DTYPE))
            for (c, side, start), guess, pk in zip(todo, guesses, peaks):
                score = xcorr_score(pk["r"], pk["energy_a"], pk["energy_b"])
                point = (start + c["len"] // 2, guess + int(pk["lag"]), score, abs(score) >= min_score)
                c["points"].append(point)
                if point[3]:
                    for s in ((0, 1) if side is None else (side,)):
                        c["trail"][s].append(point)
        # Second pass.  Inside an anchor the drift smears the peak over anchor_len x drift samples (42 at 650 ppm over 2^16), and
        # the lag of a smeared peak is good to a few samples only.  With the first line (a, b) the query is read on the
        # recording's clock around every anchor -- the time warp of section 16, with the integer lag the line predicts at the
        # anchor's centre -- and the anchor is correlated again: the peak is sharp, its lag an integer measurement at the centre.
        for c in live:
            first = [pt for pt in c["points"] if pt[3]]
            c["line"] = _lib.drift_fit([pt[0] for pt in first], [pt[1] for pt in first])[:2] if first else None
            c["first"], c["points"] = c["points"], []
        todo = [(c, start) for c in live if c["line"] is not None for group in c["starts"] for start in group]
        for n in sorted({c["len"] for c, _ in todo}):
            batch = [(c, start) for c, start in todo if c["len"] == n]
            slices, tracks, lags, at = [], np.zeros(len(batch), _lib.WARP_TRACK_DTYPE), [], 0
            for k, (c, start) in enumerate(batch):
                a, b = c["line"]
                b = min(max(b, -2.0 ** -10), 2.0 ** -10)
                mid = start + n // 2
                lag = int(round(a + b * mid))
                # output m stands for the recording's sample start - radius + m: the query at that + lag + b (that - mid)
                bend = b * (start - radius - mid)
                whole = math.floor(bend)
                pos0, f0 = start - radius + lag + whole, min(int((bend - whole) * 2.0 ** 40), (1 << 40) - 1)
                reach = int(abs(b) * (n + 2 * radius)) + 2 + 32
                lo, hi = min(max(0, pos0 - reach), c["xq"].size), min(max(0, pos0 + n + 2 * radius + reach), c["xq"].size)
                slices.append(c["xq"][lo:hi])
                tracks[k] = (at, hi - lo, pos0 - lo, f0, int(round(b * 2.0 ** 40)), 1, 0)
                lags.append(lag)
                at += hi - lo
            bent = self._gpu.warp(np.concatenate(slices), tracks, 0, n + 2 * radius)
            jobs = [(k * (n + 2 * radius), n + 2 * radius, bent.size + k * n, n, radius, 0, n, radius, 0) for k in range(len(batch))]
            pcm = np.concatenate([bent.ravel()] + [c["xr"][start:start + n] for c, start in batch])
            peaks = self._gpu.xcorr(pcm, np.array(jobs, _lib.XCORR_JOB_DTYPE))
            for (c, start), lag, pk in zip(batch, lags, peaks):
                score = xcorr_score(pk["r"], pk["energy_a"], pk["energy_b"])
                c["points"].append((start + n // 2, lag + int(pk["lag"]), score, abs(score) >= min_score))
        out = []
        for (qi, hit), c in zip(pairs, chains):
            used = [pt for pt in c["points"] if pt[3]] if c is not None else []
            if not used:                                  # nothing to go by: the hit as it is, score 0
                out.append((DriftHit(hit.name, hit.rec, float(441 * hit.offset), 0.0, False, 0.0, len(c["first"]) if c else 0, 0, 0.0), ()))
                continue
            a, b, rms = _lib.drift_fit([pt[0] for pt in used], [pt[1] for pt in used])   # (the centre first when it is used)
            neg = [pt[2] < 0 for pt in used]
            inverted = neg[0] if c["points"][0][3] else 2 * sum(neg) > len(neg)
            out.append((DriftHit(hit.name, hit.rec, a, b * 1e6, bool(inverted), float(np.median([abs(pt[2]) for pt in used])),
                                 len(c["points"]), len(used), rms), tuple(pt[0] for pt in used)))
        return out

    def refine_drift(self, query, hits: Sequence[AlignHit], min_score: float, anchor_len: int = 1 << 16, anchor_hop: int = 1 << 21,
                     radius: int = 1024) -> List[DriftHit]:
        """query: the id or name of an indexed recording, hits: what align() gave for its hashprints.  Per hit the line
        query[n + offset + drift n] ~ recording[n]: short anchors of anchor_len samples every anchor_hop samples outward from
        refine()'s segment, each correlated over lags -radius .. radius around what the anchors before it predict, and the
        Theil-Sen line through the lags of those with |score| >= min_score (which depends on the material: no default).  The
        default hop follows from the radius: 2^21 samples x 2^-10 x 1/2 ~ 1024, so the chain cannot lose a drift the time map
        admits.  Short anchors, because drift smears the peak inside a segment: 64 samples at 977 ppm over 2^16."""
        qi = self.names.index(query) if isinstance(query, str) else int(query)
        return [h for h, _ in self._drift_pairs([(qi, h) for h in hits], min_score, anchor_len, anchor_hop, radius)]

    def layout_drift(self, min_peak: int, min_score: float, k: int = 8, anchor_len: int = 1 << 16, anchor_hop: int = 1 << 21,
                     radius: int = 1024, details: bool = False):
        """layout() for recorders whose clocks differ: align all against all, the best hit of every pair with peak >= min_peak
        through refine_drift, those with a used anchor placed by place_affine().  details: also (query id, DriftHit, the centre
        samples of the used anchors) of every pair."""
        pairs = self._layout_pairs(min_peak, k)
        hits = self._drift_pairs(pairs, min_score, anchor_len, anchor_hop, radius) if pairs else []
        edges = [(qi, h.rec, h.offset, h.drift_ppm * 1e-6, h.score, h.inverted) for (qi, _), (h, _) in zip(pairs, hits) if h.used]
        comps = place_affine(len(self.names), edges, [self._audio[n][0].size for n in self.names])
        return (comps, [(qi, h, at) for (qi, _), (h, at) in zip(pairs, hits)]) if details else comps

    def render(self, component, gains=None, tracks: bool = False, chunk: int = 1 << 24) -> np.ndarray:
        """the event of a WarpedComponent (layout_drift) or a Component (layout: rates 1) as audio on the component's clock:
        int16 [n_out], the mix, or with `tracks` [n_members][n_out], every member alone.  gains: signed Q15 per member
        (default round(2^15 / n_members), negative for inverted members).  The members' PCM is uploaded once and rendered
        `chunk` outputs at a time.  A member at rate 1 with an integer start comes out in `tracks` as a shifted bit-exact copy."""
        import torch
        if not self._keep_audio:
            raise ValueError("AudioCombiner: render needs keep_audio=True")
        members = list(component.members)
        rates = list(getattr(component, "rates", (1.0,) * len(members)))
        if gains is None:
            g = int(round((1 << 15) / max(len(members), 1)))
            gains = [-g if inv else g for inv in component.inverted]
        if len(gains) != len(members) or chunk < 1:
            raise ValueError("AudioCombiner: render takes one gain per member and chunk >= 1")
        pcm = [self._audio[self.names[m]][0] for m in members]
        tr = np.zeros(len(members), _lib.WARP_TRACK_DTYPE)
        n_out, at = 0, 0
        for k, (x, start, rate) in enumerate(zip(pcm, component.starts, rates)):
            i0, f0, d = _lib.time_map_q40(float(start), float(rate) - 1.0)
            tr[k] = (at, x.size, i0, f0, d, int(gains[k]), 0)
            n_out = max(n_out, int(math.ceil(float(start) + float(rate) * x.size)))
            at += x.size
        rows = len(members) if tracks else 1
        out = np.zeros((rows, n_out), np.int16)
        if out.size:
            d_pcm = torch.from_numpy(np.concatenate(pcm)).to(f"cuda:{self._device}")
            d_out = torch.empty((rows, min(chunk, n_out)), dtype=torch.int16, device=d_pcm.device)
            call = self._gpu.warp_dev if tracks else self._gpu.mix_dev
            s = torch.cuda.current_stream(d_pcm.device).cuda_stream
            for m0 in range(0, n_out, chunk):
                n = min(chunk, n_out - m0)
                piece = d_out[:, :n].contiguous() if n < d_out.shape[1] else d_out
                call(d_pcm.data_ptr(), at, tr, m0, n, piece.data_ptr(), s)
                out[:, m0:m0 + n] = piece.cpu().numpy()
        return out if tracks else out[0]

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
