"""LiveSongIdentification in Python: the reference's C++ class
(include/hpfw/audioproblems/live-song-id/live_song_id.h:19-60) and its notebook
(examples/python/liveid.ipynb cells 2-12) over the GPU collector and the GPU scan.

index(files)  = storage.build(collector.prepare(files))           live_song_id.h:31-33
search(files) = per query: calc_hashprint -> find -> report       live_song_id.h:35-54
top(files, k) = the notebook's "ten best tracks" per query        liveid.ipynb cell 9
top_votes(files) = the reference's default storage, AnnStorage::find: per query the winning (track, offset) bucket of the
                   votes of its 0.8 s windows (annoy_storage.h:41-63, exact neighbours)
timeline(file) = the songs of one long recording, window by window (not in the reference)
streams(n)     = the same for n feeds that are still running, as their samples arrive
"""
import os
from fractions import Fraction
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .collector import ParallelCollector


class _ShardedIndex:
    """what LiveSongIdentification asks of its index handle, over a hpfw_amd.multi.GpuGroup: the index sharded over the
    given devices (one ordinal per shard), every search and its result as the one handle's"""

    def __init__(self, devices):
        from . import multi
        self.group = multi.GpuGroup(devices)
        self._first = _lib.Gpu.from_handle(self.group.handle(0))
        for name in ("index_offsets", "index_remove", "search_topk", "search_topk_scored", "search_topk_transposed",
                     "search_topk_transposed_scored", "search_votes"):
            setattr(self, name, getattr(self.group, name))
        self.geometry, self.resample = self._first.geometry, self._first.resample

    def index_clear(self):
        self.group.index_build(np.zeros(1, np.uint64), np.zeros(1, np.int64))

    def index_add(self, hp, offsets):
        self.group.index_build(hp, offsets)               # (build() clears first: the one add is the whole index)

    def extract_windows(self, extractor, pcm, win, hop, tempos, shifts):
        """the windows sharded over the group, under the filters and the projection mode of `extractor`"""
        self.group.set_filters(extractor.get_filters())
        for i in range(self.group.shards):
            _lib.Gpu.from_handle(self.group.handle(i)).set_projection(extractor.get_projection())
        return self.group.extract_windows(pcm, win, hop, tempos, shifts)

    def close(self):
        self.group.close()


def rate_fraction(max_rate) -> Tuple[int, int]:
    """(rate_num, rate_den) of a threshold in mismatching bits per hashprint for the catalogue self-join: an int or a Fraction
    is taken as it is, a float through Fraction(max_rate).limit_denominator(1024).  Anything else, a denominator above 1024
    and a rate outside [0, 64] raise HPFW_E_INVALID."""
    if isinstance(max_rate, bool) or not isinstance(max_rate, (int, Fraction, float)):
        raise _lib.HpfwError("max_rate must be an int, a Fraction or a float", _lib.E_INVALID)
    if isinstance(max_rate, float):
        if not 0.0 <= max_rate <= 64.0:                   # (NaN and the infinities as well)
            raise _lib.HpfwError("max_rate must be in [0, 64]", _lib.E_INVALID)
        max_rate = Fraction(max_rate).limit_denominator(1024)
    rate = Fraction(max_rate)
    if rate.denominator > 1024 or not 0 <= rate <= 64:
        raise _lib.HpfwError("max_rate must be in [0, 64] with a denominator of at most 1024", _lib.E_INVALID)
    return rate.numerator, rate.denominator


def duplicate_groups(pairs, names: Sequence[str]) -> List[List[str]]:
    """the connected components of duplicates()'s pairs as lists of names: every list in the order of `names` (the index's),
    the lists by their first member; a name no pair mentions is in no list (a host union-find)"""
    slot = {}
    for i, name in enumerate(names):
        slot.setdefault(name, i)
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for pair in pairs:
        a, b = find(slot[pair[0]]), find(slot[pair[1]])
        if a != b:
            parent[max(a, b)] = min(a, b)                 # a component's root is its first slot
    groups = {}
    for x in sorted(parent):
        groups.setdefault(find(x), []).append(names[x])
    return [groups[root] for root in sorted(groups)]


def keep_new(pairs, n_index: int, n_new: int) -> List[bool]:
    """which recordings of a batch add_new() keeps, from the join's pairs with among_new = 1: pairs of ids (a, b, ...) with
    n_index <= b < n_index + n_new the batch's recordings in their order and a < b an indexed recording (a < n_index) or an
    earlier one of the batch.  Recording i is kept unless some pair (a, n_index + i) has an a that is indexed or an earlier
    kept recording of the batch: of a new song that comes twice the first is kept, and a recording that only duplicates a
    dropped one is kept (what it duplicates is then not in the index).  A pure host function."""
    partners = [[] for _ in range(n_new)]
    for pair in pairs:
        a, b = int(pair[0]), int(pair[1])
        if not (0 <= a < b and n_index <= b < n_index + n_new):
            raise ValueError(f"keep_new: ({a}, {b}) is no pair of the join of {n_new} recordings against {n_index}")
        partners[b - n_index].append(a)
    keep = []
    for i in range(n_new):
        keep.append(not any(a < n_index or keep[a - n_index] for a in partners[i]))
    return keep


class LiveSongIdentification:
    def __init__(self, cache: str = "", device: int = 0, resample: bool = False, devices: Optional[Sequence[int]] = None):
        """resample: index and search WAV files at any rate in [8 000, 192 000] Hz (ParallelCollector(resample=True));
        devices: one device ordinal per shard (an ordinal may repeat) -- the index is sharded over them and top(), search()
        and timeline() give what they give on one device; None: one handle on `device`"""
        self.collector = ParallelCollector(resample=resample)
        self._resample = resample
        self.collector.load(cache)                       # the constructor loads the cache, live_song_id.h:24
        self._cache = cache
        self._gpu = _lib.Gpu(device) if devices is None else _ShardedIndex(list(devices))
        self.names: List[str] = []
        self._removed = set()                            # slots of self.names whose recording was removed
        self._added_len: List[int] = []                  # per slot the hashprints the recording had when it was added

    def close(self):
        self.collector.save(self._cache)                 # the destructor saves it, live_song_id.h:28
        self._gpu.close()

    def build(self, hashprints: Sequence[Tuple[np.ndarray, str]]):
        """MemoryStorage::build (storage.h:21-25) from prepare()'s (array, name) pairs"""
        self.names = [name for _, name in hashprints]
        self._removed = set()                            # a fresh index forgets all removals
        self._added_len = [int(hp.size) for hp, _ in hashprints]
        self._gpu.index_clear()
        if self.names:
            off = np.zeros(len(hashprints) + 1, np.int64)
            np.cumsum([hp.size for hp, _ in hashprints], out=off[1:])
            flat = np.concatenate([hp for hp, _ in hashprints]) if off[-1] else np.zeros(1, np.uint64)
            self._gpu.index_add(flat, off)

    def index(self, filenames: Sequence[str]):
        self.build(self.collector.prepare(list(filenames)))

    # ---- index maintenance: slots of self.names are ids and stay; a removed recording's slot is empty
    def live_names(self) -> List[str]:
        """the recordings that remain, in slot order"""
        removed = getattr(self, "_removed", ())
        return [name for i, name in enumerate(self.names) if i not in removed]

    def _live_slots(self, name):
        removed = getattr(self, "_removed", ())
        return [i for i, n in enumerate(self.names) if n == name and i not in removed]

    def remove(self, names: Sequence[str]) -> int:
        """removes the recordings named from the index in place, on one device and with devices=: every live slot carrying one
        of the names goes, self.names keeps its length, and no search names them afterwards; returns the slots removed.  An
        unknown or already removed name raises KeyError before anything changes; a name may repeat in the list."""
        slots = []
        for name in dict.fromkeys(names):
            live = self._live_slots(name)
            if not live:
                raise KeyError(name)
            slots += live
        if slots:
            self._gpu.index_remove(slots)
            self._removed.update(slots)
        return len(slots)

    def add(self, filenames: Sequence[str]) -> int:
        """appends the recordings of the files to the index: their hashprints by collector.calc_hashprints under the filters
        in force (nothing is re-learned), their stems behind self.names; returns the recordings added.  A file that yields no
        hashprint is left out.  An identifier made with devices= raises HPFW_E_UNSUPPORTED: a sharded index is rebuilt."""
        self._no_shards("adding to the index")
        return self._append(self._new_hashprints(filenames))

    def _new_hashprints(self, filenames):
        """[(hashprints, name)] of the files that yield any, as add() takes them"""
        return [(hp, name) for hp, name in self.collector.calc_hashprints(list(filenames)) if hp is not None and hp.size]

    def _append(self, pairs) -> int:
        """add()'s second half: (hashprints, name) pairs behind the index, with the bookkeeping of their slots"""
        if pairs:
            off = np.zeros(len(pairs) + 1, np.int64)
            np.cumsum([hp.size for hp, _ in pairs], out=off[1:])
            self._gpu.index_add(np.concatenate([hp for hp, _ in pairs]), off)
            self.names += [name for _, name in pairs]
            self._added_len += [int(hp.size) for hp, _ in pairs]
        return len(pairs)

    # ---- catalogue self-join: which recordings of the index duplicate or contain each other
    def duplicates(self, max_rate, min_overlap: int):
        """the pairs of indexed recordings whose best alignment by the overlap rule, over at least min_overlap hashprints,
        has at most max_rate mismatching bits per hashprint (an int, a Fraction or a float: rate_fraction()); neither has a
        default.  [(name_a, name_b, dist, overlap, lag)] in index order of (a, b): column 0 of a lies on column lag of b
        (negative: a begins before b does), overlap columns are compared and dist bits of them differ.  Removed recordings
        never appear.  An identifier made with devices= raises HPFW_E_UNSUPPORTED.

        What to remove is the caller's decision, for example everything but the first recording of each group:
            groups = lsi.duplicate_groups(lsi.duplicates(16, 304))
            lsi.remove([name for group in groups for name in group[1:]])"""
        num, den = rate_fraction(max_rate)
        self._no_shards("the catalogue self-join")
        pairs = self._gpu.index_selfjoin(int(min_overlap), num, den)
        return [(self.names[int(p["a"])], self.names[int(p["b"])], int(p["dist"]), int(p["overlap"]), int(p["lag"])) for p in pairs]

    # ---- local self-join: which recordings of the index share a passage, and where
    def shared_passages(self, max_rate: int, min_score: int):
        """the pairs of indexed recordings that share a passage: the best run of consecutive hashprints on any diagonal of
        the two, at max_rate - (mismatching bits) a hashprint, scores at least min_score.  max_rate, 1..31 mismatching bits
        per hashprint, and min_score >= 1 have no default: the caller decides.  [(name_a, name_b, score, lag, a_start, length,
        dist)] in index order of (a, b): columns a_start .. a_start + length - 1 of a lie on columns lag + a_start onwards of b
        and differ from them in dist bits; score = max_rate * length - dist.  One passage a pair; removed recordings never
        appear.  An identifier made with devices= raises HPFW_E_UNSUPPORTED."""
        self._no_shards("the local self-join")
        pairs = self._gpu.index_localjoin(int(max_rate), int(min_score))
        return [(self.names[int(p["a"])], self.names[int(p["b"])], int(p["score"]), int(p["lag"]), int(p["a_start"]), int(p["length"]),
                 int(p["dist"])) for p in pairs]

    def duplicate_groups(self, pairs) -> List[List[str]]:
        """the connected components of duplicates()'s pairs as lists of names in index order (duplicate_groups())"""
        return duplicate_groups(pairs, self.live_names())

    # ---- ingest check: what of a batch of files the index already holds, before they are added
    def _join(self, new, rate, min_overlap, among_new):
        """DUP_PAIR_DTYPE records of the join of _new_hashprints()'s pairs against the index; rate: rate_fraction()'s"""
        num, den = rate
        if not new:
            return np.zeros(0, _lib.DUP_PAIR_DTYPE)
        off = np.zeros(len(new) + 1, np.int64)
        np.cumsum([hp.size for hp, _ in new], out=off[1:])
        return self._gpu.index_join(np.concatenate([hp for hp, _ in new]), off, int(min_overlap), num, den, int(bool(among_new)))

    def _named(self, pairs, new):
        names = self.names + [name for _, name in new]
        return [(names[int(p["a"])], names[int(p["b"])], int(p["dist"]), int(p["overlap"]), int(p["lag"])) for p in pairs]

    def known(self, filenames: Sequence[str], max_rate, min_overlap: int, among_new: bool = True):
        """what duplicates() would report in addition after add(filenames), without the index changing: the pairs (a, b) with b
        one of the files and a an indexed recording or, with among_new, an earlier file of the batch, by duplicates()'s rule,
        threshold and order.  [(name_a, name_b, dist, overlap, lag)]; name_b is the name add() would give the file.  Files that
        yield no hashprint are left out and take no id, as in add().  An identifier made with devices= raises
        HPFW_E_UNSUPPORTED."""
        rate = rate_fraction(max_rate)                    # (refused before any file is read)
        self._no_shards("the ingest check")
        new = self._new_hashprints(filenames)
        return self._named(self._join(new, rate, min_overlap, among_new), new)

    def add_new(self, filenames: Sequence[str], max_rate, min_overlap: int):
        """add() of the files the index does not hold yet: the files are extracted once and joined against the index and each
        other (known() with among_new), a file is kept unless a reported pair pairs it with an indexed recording or with an
        earlier kept file of the batch (keep_new()), and the kept files are added from the hashprints already extracted.
        Returns (the names added, known()'s pairs).  An identifier made with devices= raises HPFW_E_UNSUPPORTED."""
        rate = rate_fraction(max_rate)
        self._no_shards("the ingest check")
        new = self._new_hashprints(filenames)
        pairs = self._join(new, rate, min_overlap, True)
        keep = keep_new([(int(p["a"]), int(p["b"])) for p in pairs], len(self.names), len(new))
        named = self._named(pairs, new)                   # (before the index grows: ids of the batch as the join gave them)
        kept = [pair for pair, k in zip(new, keep) if k]
        self._append(kept)
        return [name for _, name in kept], named

    # ---- search within a subset of the index
    def _within_slots(self, within) -> List[int]:
        """the sorted live slots that carry one of the names; an unknown or removed name raises KeyError, as remove() does"""
        slots = set()
        for name in dict.fromkeys(within):
            live = self._live_slots(name)
            if not live:
                raise KeyError(name)
            slots.update(live)
        return sorted(slots)

    def _check_within(self, within, min_overlap=None):
        """what top(), timeline() and streams() refuse of within, before anything runs on a device"""
        if within is None:
            return
        if min_overlap is not None:
            raise _lib.HpfwError("within: the overlap rule does not search within a set", _lib.E_UNSUPPORTED)
        if isinstance(self._gpu, _ShardedIndex):
            raise _lib.HpfwError("the search within a set is not available on a sharded index", _lib.E_UNSUPPORTED)

    def _one_set(self, within, n_q):
        """within (names or None) as _search_windows and top() take it: None, or (set_off, set_clips, q_set) with every one of
        the n_q queries in the one set"""
        if within is None:
            return None
        slots = self._within_slots(within)
        return np.array([0, len(slots)], np.int64), np.array(slots, np.int32), np.zeros(n_q, np.int32)

    def top(self, filenames: Sequence[str], k: int = 10, shifts: Optional[Sequence[int]] = None,
            tempos: Optional[Sequence[float]] = None, within: Optional[Sequence[str]] = None):
        """per query (label, [(distance, name, offset) x <= k]) ordered by (distance, position in the
        database); None in place of the list for a file that yields no hashprint.  shifts: bin shifts of the query's
        constant-Q spectrogram to search as well (t semitones above the indexed recording is
        s = 2t): each clip's smallest distance over them, and every hit is (distance, name, offset, shift).  tempos:
        tempo factors (query tempo / indexed tempo) to search, each combined with every shift:
        every hit is (distance, name, offset, shift, tempo), shift 0 when shifts is None, offset in the indexed
        recording; a query too short for the slowest tempo yields None.  within: names of indexed recordings -- the search
        runs over the live slots carrying them alone and answers what an identifier of just those recordings would (DESIGN.md
        section 24); an unknown or removed name raises KeyError before anything runs, an identifier made with devices= raises
        HPFW_E_UNSUPPORTED"""
        self._check_within(within)
        sets = self._one_set(within, 0)                   # (names -> slots: a KeyError comes before any file is read)
        if tempos is not None:
            return self._top_tempo(list(filenames), k, None if shifts is None else list(shifts), list(tempos), sets)
        if shifts is not None:
            return self._top_transposed(list(filenames), k, list(shifts), sets)
        hps = self.collector.calc_hashprints(list(filenames))
        good = [i for i, (hp, _) in enumerate(hps) if hp is not None and hp.size]
        out = [(f, None) for f in filenames]
        if good and self.names:
            off = np.zeros(len(good) + 1, np.int64)
            np.cumsum([hps[i][0].size for i in good], out=off[1:])
            q = np.concatenate([hps[i][0] for i in good])
            if sets is None:
                hits = self._gpu.search_topk(q, off, k)
            else:
                hits = self._gpu.search_topk_within(q, off, k, sets[0], sets[1], np.zeros(len(good), np.int32))
            for row, i in zip(hits, good):
                out[i] = (filenames[i], [(int(h["dist"]), self.names[int(h["clip"])], int(h["offset"]))
                                         for h in row if h["clip"] != 0xFFFFFFFF])
        return out

    def top_votes(self, filenames: Sequence[str]):
        """the reference's default search (AnnStorage::find, annoy_storage.h:41-63, with exact neighbours; DESIGN.md section
        19): per query position the 5 nearest 64-hashprint windows of the index vote 1 / (distance + 1) for (track, offset),
        and the first bucket to exceed the running maximum wins.  Per query (label, (cnt, name, offset)), offset the
        reference's i - p in hashprints (query position minus position in the track: a query cut from column s of a track
        gives -s); None in place of the tuple for a file that yields fewer than 64 hashprints, and when the index has no item"""
        hps = self.collector.calc_hashprints(list(filenames))
        good = [i for i, (hp, _) in enumerate(hps) if hp is not None and hp.size >= 64]
        out = [(f, None) for f in filenames]
        if good and self.names:
            off = np.zeros(len(good) + 1, np.int64)
            np.cumsum([hps[i][0].size for i in good], out=off[1:])
            votes = self._votes(np.concatenate([hps[i][0] for i in good]), off)
            for v, i in zip(votes, good):
                if v["clip"] != _lib.NO_CLIP:
                    out[i] = (filenames[i], (float(v["cnt"]), self.names[int(v["clip"])], int(v["offset"])))
        return out

    def _votes(self, q_hp, q_off):
        """VOTE_DTYPE [n_q] by the device tally, on one handle as on a sharded index"""
        return self._gpu.search_votes(q_hp, q_off)

    def top_overlap(self, filenames: Sequence[str], k: int, min_overlap: int):
        """top() by the overlap search: the query may overhang either end of an indexed recording, and
        clips are ordered by mismatching bits per overlapping hashprint over at least min_overlap hashprints (no default:
        the caller decides).  Per query (label, [(distance, name, lag, overlap) x <= k]): query column 0 lies on column lag of
        the recording (negative: the query begins before it does), overlap columns are compared.  None in place of the list
        for a file that yields no hashprint.  An identifier made with devices= raises HPFW_E_UNSUPPORTED."""
        if isinstance(self._gpu, _ShardedIndex):
            raise _lib.HpfwError("the overlap search is not available on a sharded index", _lib.E_UNSUPPORTED)
        hps = self.collector.calc_hashprints(list(filenames))
        good = [i for i, (hp, _) in enumerate(hps) if hp is not None and hp.size]
        out = [(f, None) for f in filenames]
        if good and self.names:
            off = np.zeros(len(good) + 1, np.int64)
            np.cumsum([hps[i][0].size for i in good], out=off[1:])
            hits = self._gpu.search_overlap(np.concatenate([hps[i][0] for i in good]), off, k, min_overlap)
            for row, i in zip(hits, good):
                out[i] = (filenames[i], [(int(h["dist"]), self.names[int(h["clip"])], int(h["lag"]), int(h["overlap"]))
                                         for h in row if h["clip"] != 0xFFFFFFFF])
        return out

    def _no_shards(self, what):
        if isinstance(self._gpu, _ShardedIndex):
            raise _lib.HpfwError(f"{what} is not available on a sharded index", _lib.E_UNSUPPORTED)

    def top_warped(self, filenames: Sequence[str], k: int, candidates: int):
        """top() by the warped search: the query may run faster or slower than the indexed recording
        inside the window (local slope 1/2 .. 2), distances on top()'s scale.  candidates has no default: 0 warps every
        indexed recording against every query, k..64 re-ranks that many best recordings of the plain search.  Per query
        (label, [(distance, name, start, end) x <= k]): the query's first hashprint lies on column start of the recording and
        its last on column end.  None in place of the list for a file that yields no hashprint.  No shifts, no tempos
        (Gpu.dtw_pairs takes any hashprints a caller extracts); an identifier made with devices= raises HPFW_E_UNSUPPORTED."""
        self._no_shards("the warped search")
        hps = self.collector.calc_hashprints(list(filenames))
        good = [i for i, (hp, _) in enumerate(hps) if hp is not None and hp.size]
        out = [(f, None) for f in filenames]
        if good and self.names:
            off = np.zeros(len(good) + 1, np.int64)
            np.cumsum([hps[i][0].size for i in good], out=off[1:])
            hits = self._gpu.search_dtw(np.concatenate([hps[i][0] for i in good]), off, k, candidates)
            for row, i in zip(hits, good):
                out[i] = (filenames[i], [(int(h["dist"]), self.names[int(h["clip"])], int(h["start"]), int(h["end"]))
                                         for h in row if h["clip"] != _lib.NO_CLIP])
        return out

    def top_local(self, filenames: Sequence[str], k: int, max_rate: int):
        """top() by the local search: which part of the query is which part of which recording.  A run
        of consecutive query hashprints on one diagonal of a recording scores max_rate * length - dist; max_rate, 1..31
        mismatching bits per hashprint, has no default: the caller decides.  Per query (label, [(score, name, lag, q_start,
        length, dist) x <= k]), larger score first: query hashprints q_start .. q_start + length - 1 lie on columns lag + q_start
        onwards of the recording and differ from them in dist bits.  None in place of the list for a file that yields no
        hashprint.  No shifts, no tempos; an identifier made with devices= raises HPFW_E_UNSUPPORTED."""
        self._no_shards("the local search")
        hps = self.collector.calc_hashprints(list(filenames))
        good = [i for i, (hp, _) in enumerate(hps) if hp is not None and hp.size]
        out = [(f, None) for f in filenames]
        if good and self.names:
            off = np.zeros(len(good) + 1, np.int64)
            np.cumsum([hps[i][0].size for i in good], out=off[1:])
            hits = self._gpu.search_local(np.concatenate([hps[i][0] for i in good]), off, k, max_rate)
            for row, i in zip(hits, good):
                out[i] = (filenames[i], [(int(h["score"]), self.names[int(h["clip"])], int(h["lag"]), int(h["q_start"]),
                                         int(h["length"]), int(h["dist"])) for h in row if h["clip"] != _lib.NO_CLIP])
        return out

    def warp_path(self, filename: str, name: str):
        """(distance, columns): columns int32, the column of the indexed recording `name` every hashprint of the query file
        lies on.  None for a file that yields no hashprint or a recording too short for the query;
        an unknown name raises KeyError; an identifier made with devices= raises HPFW_E_UNSUPPORTED."""
        self._no_shards("the warped path")
        live = self._live_slots(name)                      # (a removed name is unknown)
        if not live:
            raise KeyError(name)
        hp = self.collector.calc_hashprints([filename])[0][0]
        if hp is None or not hp.size:
            return None
        hit, path = self._gpu.dtw_path(hp, live[0])
        if hit["clip"] == _lib.NO_CLIP:
            return None
        return int(hit["dist"]), path

    def columns_to_seconds(self, columns, window_s: float = 5.0):
        """columns of an indexed recording (warp_path, the offsets of top()) in seconds, by the conversion timeline() uses for
        its offsets: one column is 3 win / m samples of the geometry of a window of window_s seconds"""
        win = int(round(window_s * 44100))
        return np.asarray(columns, np.float64) * (3.0 * win / self._gpu.geometry(win).m / 44100.0)

    def _top_transposed(self, filenames: List[str], k: int, shifts: List[int], sets=None):
        shifts = _lib.check_shifts(shifts)
        return self._top_sets(filenames, k, len(shifts), lambda g, x: g.extract_transposed(x, shifts)[0],
                              lambda h: (shifts[int(h["shift_index"])],), "transposed", sets)

    def _top_tempo(self, filenames: List[str], k: int, shifts: Optional[List[int]], tempos: List[float], sets=None):
        if shifts is not None:
            shifts = _lib.check_shifts(shifts)
        n_s = len(shifts) if shifts else 1
        _lib.check_tempos(tempos, 0 if shifts is None else len(shifts))

        def decode(h):
            j, i = divmod(int(h["shift_index"]), n_s)                 # variant v = j max(S, 1) + i
            return (shifts[i] if shifts else 0, tempos[j])
        return self._top_sets(filenames, k, len(tempos) * n_s, lambda g, x: g.extract_tempo(x, tempos, shifts)[0], decode,
                              "tempo", sets)

    def _top_sets(self, filenames: List[str], k: int, n_sets: int, extract, decode, what: str, within=None):
        """the search of n_sets hashprint sets per query (extract(gpu, pcm) -> [n_sets][n_hp]) merged per clip
        (hpfw_gpu_search_topk_transposed); decode(hit) -> what a hit adds to (distance, name, offset); within: None, or
        _one_set()'s set of clips for every query"""
        extractor = self.collector.gpu()                  # the collector's filters
        if extractor.get_projection() != 1:
            raise _lib.HpfwError(f"{what} search needs projection mode 1 (fixed point)", _lib.E_INVALID)
        out = [(f, None) for f in filenames]
        sets, good = [], []
        for i, f in enumerate(filenames):
            # a file that yields no hashprint gets None, as calc_hashprints gives it: unreadable or at another rate
            # (HPFW_E_IO), empty, too short or too long (HPFW_E_UNSUPPORTED); every other failure is raised
            try:
                x = _lib.read_wav_44k(self._gpu, f, self._resample)
                if x.size == 0:
                    continue
                sets.extend(extract(extractor, x))
            except _lib.HpfwError as e:
                if e.status in (_lib.E_IO, _lib.E_UNSUPPORTED):
                    continue
                raise
            good.append(i)
        if good and self.names:
            off = np.zeros(len(sets) + 1, np.int64)
            np.cumsum([hp.size for hp in sets], out=off[1:])
            if within is None:
                hits = self._gpu.search_topk_transposed(np.concatenate(sets), off, n_sets, k)
            else:
                hits = self._gpu.search_topk_transposed_within(np.concatenate(sets), off, n_sets, k, within[0], within[1],
                                                               np.zeros(len(good), np.int32))
            for row, i in zip(hits, good):
                out[i] = (filenames[i], [(int(h["dist"]), self.names[int(h["clip"])], int(h["offset"])) + decode(h)
                                         for h in row if h["clip"] != 0xFFFFFFFF])
        return out

    def timeline(self, filename: str, min_score: float, window_s: float = 5.0, hop_s: float = 2.5,
                 shifts: Optional[Sequence[int]] = None, tempos: Optional[Sequence[float]] = None,
                 tol_cols: Optional[float] = None, max_gap: int = 1, min_windows: int = 1, windows: bool = False,
                 min_overlap: Optional[int] = None, within: Optional[Sequence[str]] = None):
        """the set list of one long recording: windows of window_s seconds every hop_s seconds, each
        searched for its best clip and scored by how far that clip stands out from the others (hpfw_gpu_hit_score);
        consecutive windows with score >= min_score that name the same clip at consistent offsets form a segment
        (hpfw_gpu_timeline_segments; tol_cols None = max(2, 0.08 hop in columns)).
        Returns [(start_s, end_s, name, score, offset_s, shift, tempo)]: the segment's extent in the recording, the score,
        shift and tempo of its best window, and where in the indexed recording its first window starts.  windows=True:
        (segments, [(clip index or None, name or None, distance, offset, score, shift, tempo) per window]).
        An unreadable file or one shorter than a window gives []; every other failure raises.
        min_overlap=N: every window is searched by the overlap rule over at least N hashprints, so a
        window that begins before a song does or runs past its end, and an indexed item shorter than the window, are found.
        offset is then the lag (negative: the window begins before the clip does), the score is that of the hit's rate among
        the rates of the other clips, start_s / end_s are trimmed to the part of the first and last window that lies on the
        clip, offset_s is max(0, first lag) in seconds, and a window tuple carries the overlap as an eighth element.  Not
        with shifts or tempos and not on an identifier made with devices= (HPFW_E_UNSUPPORTED).
        within=names: every window is searched within the live slots carrying those names, as top()
        does it, and gives what an identifier of just those recordings gives.  The scores are against the moments of the set's
        clips: how far a song stands out from the set, not from the catalogue; a set with fewer than 3 counted clips scores
        NaN, as an index of 2 clips does, and no window is strong.  An unknown or removed name raises KeyError before anything
        runs.  Not with min_overlap and not on an identifier made with devices= (HPFW_E_UNSUPPORTED)."""
        win, hop = int(round(window_s * 44100)), int(round(hop_s * 44100))
        self._check_within(within, min_overlap)
        slots = None if within is None else self._within_slots(within)
        self._check_min_overlap(min_overlap, shifts, tempos, win, hop)
        if shifts is not None:
            shifts = _lib.check_shifts(shifts)
        if tempos is not None:
            tempos = _lib.check_tempos(tempos, 0 if shifts is None else len(shifts))
        variants = shifts is not None or tempos is not None
        extractor = self.collector.gpu()                  # the collector's filters
        if variants and extractor.get_projection() != 1:
            raise _lib.HpfwError("timeline with shifts or tempos needs projection mode 1 (fixed point)", _lib.E_INVALID)
        empty = ([], []) if windows else []
        _lib.window_count(0, win, hop)                     # (a bad window or hop raises whatever the file holds)
        try:
            x = _lib.read_wav_44k(self._gpu, filename, self._resample)
        except _lib.HpfwError as e:
            if e.status == _lib.E_IO:
                return empty
            raise
        if _lib.window_count(x.size, win, hop) == 0:
            return empty
        if isinstance(self._gpu, _ShardedIndex):
            hp = self._gpu.extract_windows(extractor, x, win, hop, tempos, shifts)
        else:
            hp = extractor.extract_windows(x, win, hop, tempos, shifts)
        sets = None if slots is None else (np.array([0, len(slots)], np.int64), np.array(slots, np.int32), np.zeros(hp.shape[0], np.int32))
        rows, per_window = self._search_windows(hp, shifts, tempos, min_overlap, sets)
        m = self._gpu.geometry(win).m
        segs = _lib.timeline_segments(rows, min_score, hop * m / (3.0 * win), win, hop, tol_cols, max_gap, min_windows)
        out = [self._segment_tuple(sg, *per_window[int(sg["best_window"])][5:7], 3.0 * win / m / 44100.0,
                                   None if min_overlap is None else
                                   self._trim(sg, per_window[int(sg["first"])][3], per_window[int(sg["last"])][3], win, hop))
               for sg in segs]
        return (out, per_window) if windows else out

    def _check_min_overlap(self, min_overlap, shifts, tempos, win, hop):
        """what timeline() and streams() refuse of min_overlap, before anything runs on a device"""
        if min_overlap is None:
            return
        if shifts is not None or tempos is not None:
            raise _lib.HpfwError("min_overlap: the overlap rule has no shifts and no tempos", _lib.E_UNSUPPORTED)
        if isinstance(self._gpu, _ShardedIndex):
            raise _lib.HpfwError("the overlap search is not available on a sharded index", _lib.E_UNSUPPORTED)
        _lib.window_count(0, win, hop)                     # (a bad window is refused as such)
        n_hp = self._gpu.geometry(win).n_hp
        if not 1 <= int(min_overlap) <= n_hp:
            raise _lib.HpfwError(f"min_overlap must be in 1..{n_hp}, the hashprints of a window", _lib.E_INVALID)

    def _search_windows_overlap(self, hp, min_overlap):
        """_search_windows by the overlap rule: a window's record carries the lag as its offset, its
        score is that of the hit's rate against the moments of the clips' rates, and its tuple ends with the overlap"""
        n_w, k_q = hp.shape
        hits, stats = self._gpu.search_overlap_scored(hp, np.arange(n_w + 1, dtype=np.int64) * k_q, 1, int(min_overlap))
        rows = np.zeros(n_w, _lib.WINDOW_HIT_DTYPE)
        per_window = []
        for w in range(n_w):
            h = hits[w, 0]
            if h["clip"] == _lib.NO_CLIP:
                rows[w] = (_lib.NO_CLIP, 0, 0, 0, 1.0, np.nan)
                per_window.append((None, None, None, None, float("nan"), 0, 1.0, 0))
                continue
            clip, dist, lag, overlap = int(h["clip"]), int(h["dist"]), int(h["lag"]), int(h["overlap"])
            score = _lib.hit_score(_lib.overlap_rate(dist, overlap), True, stats[w])
            rows[w] = (clip, lag, 0, 0, 1.0, score)
            per_window.append((clip, self.names[clip], dist, lag, score, 0, 1.0, overlap))
        return rows, per_window

    def _trim(self, sg, first_lag, last_lag, win, hop):
        """(start, end, first lag) of a segment of windows searched by the overlap rule: the samples of its first and last
        window that lie on the clip (hpfw_gpu_overlap_extent)"""
        g = self._gpu.geometry(win)
        # the clip's length as it was added: a segment open on a recording that has been removed since ends as it would have
        # ended had the feed stopped matching
        added, clip = getattr(self, "_added_len", ()), int(sg["clip"])
        n_clip = added[clip] if clip < len(added) else int(np.diff(self._gpu.index_offsets())[clip])
        a, _ = _lib.overlap_extent(first_lag, n_clip, g.n_hp, g.c - g.n_hp + 1, win, g.m)
        _, b = _lib.overlap_extent(last_lag, n_clip, g.n_hp, g.c - g.n_hp + 1, win, g.m)
        return int(sg["first"]) * hop + a, int(sg["last"]) * hop + b, int(first_lag)

    def _search_windows(self, hp, shifts, tempos, min_overlap=None, sets=None):
        """the scored search of the windows' hashprints hp [n_w][k_q] or, with variants, [n_w][n_sets][k_q] (shifts and tempos
        as checked): (WINDOW_HIT_DTYPE [n_w] for the segment rule, [(clip index or None, name or None, distance, offset, score,
        shift, tempo) per window]).  timeline() and LiveStreams.push() share it.  min_overlap: None, or the overlap rule.
        sets: None, or (set_off, set_clips, q_set [n_w]) -- window w is searched within set q_set[w] (-1: the whole index) and
        scored against that set's moments, in the one search."""
        if min_overlap is not None:
            return self._search_windows_overlap(hp, min_overlap)
        variants = shifts is not None or tempos is not None
        n_s = len(shifts) if shifts else 1
        n_sets = (len(tempos) if tempos else 1) * n_s
        n_w, k_q = hp.shape[0], hp.shape[-1]
        off = np.arange(n_w * n_sets + 1, dtype=np.int64) * k_q
        if variants and sets is not None:
            hits, stats = self._gpu.search_topk_transposed_within(hp, off, n_sets, 1, *sets, scored=True)
        elif variants:
            hits, stats = self._gpu.search_topk_transposed_scored(hp, off, n_sets, 1)
        elif sets is not None:
            hits, stats = self._gpu.search_topk_within(hp, off, 1, *sets, scored=True)
        else:
            hits, stats = self._gpu.search_topk_scored(hp, off, 1)
        clip_len = np.diff(self._gpu.index_offsets())
        rows = np.zeros(n_w, _lib.WINDOW_HIT_DTYPE)
        per_window = []
        for w in range(n_w):
            h = hits[w, 0]
            v = int(h["shift_index"]) if variants else 0
            j, i = divmod(max(v, 0), n_s)                  # variant v = j max(S, 1) + i
            shift, tempo = (shifts[i] if shifts else 0), (tempos[j] if tempos else 1.0)
            if h["clip"] == _lib.NO_CLIP:
                rows[w] = (_lib.NO_CLIP, 0, 0, 0, 1.0, np.nan)
                per_window.append((None, None, None, None, float("nan"), 0, 1.0))
                continue
            clip = int(h["clip"])
            score = _lib.hit_score(int(h["dist"]), clip_len[clip] >= k_q, stats[w, v] if variants else stats[w])
            rows[w] = (clip, int(h["offset"]), v, 0, tempo, score)
            per_window.append((clip, self.names[clip], int(h["dist"]), int(h["offset"]), score, shift, tempo))
        return rows, per_window

    def _segment_tuple(self, sg, shift, tempo, col_s, trim=None):
        """a SEGMENT_DTYPE record as timeline() returns it; shift, tempo: those of its best window, col_s: one index column
        in seconds; trim: None, or _trim() of a segment found by the overlap rule"""
        start, end, first = (int(sg["start"]), int(sg["end"]), int(sg["first_offset"])) if trim is None else trim
        if trim is not None:
            first = max(first, 0)                          # a window that begins before the clip starts at the clip's start
        return (start / 44100.0, end / 44100.0, self.names[int(sg["clip"])], float(sg["best_score"]), first * col_s, shift, tempo)

    def streams(self, n_streams: int, min_score: float, window_s: float = 5.0, hop_s: float = 2.5,
                shifts: Optional[Sequence[int]] = None, tempos: Optional[Sequence[float]] = None,
                tol_cols: Optional[float] = None, max_gap: int = 1, min_windows: int = 1, capacity_s: Optional[float] = None,
                windows: bool = False, rate=44100, min_overlap: Optional[int] = None, within=None):
        """the timelines of n_streams live feeds as their samples arrive (hpfw_amd.streams.LiveStreams):
        per feed exactly what timeline() gives for a file that holds everything pushed to it.  Feeds are mono PCM16.  rate: the
        feeds' sample rate, one int for all or one per feed; another rate than 44 100 Hz is taken only by an identifier made with
        resample=True, as files at other rates are (HPFW_E_UNSUPPORTED otherwise), and is converted chunk by chunk on the GPU:
        the feed then yields what timeline() gives for a file at that rate, once H zero samples have been pushed behind its end
        (LiveStreams.tail).  capacity_s: seconds of audio a feed's ring holds (None: two windows).  min_overlap: as timeline()'s,
        with its refusals.  within: None, one list of names for all feeds, or one entry per feed (a list of names or None):
        a feed's windows are searched within its set and scored against the set's moments, as timeline(within=) does (fewer
        than 3 counted clips: NaN), and one push is still one search; the names become slots here, with timeline()'s KeyError
        and refusals."""
        from .streams import LiveStreams
        self._check_within(within, min_overlap)
        if within is not None:
            per_feed = [within] * int(n_streams) if all(isinstance(w, str) for w in within) else list(within)
            if len(per_feed) != int(n_streams):
                raise ValueError("within: one list of names, or one entry per feed")
            within = [None if w is None else self._within_slots(w) for w in per_feed]
        rates = [int(rate)] * int(n_streams) if np.ndim(rate) == 0 else [int(r) for r in rate]
        other = [r for r in rates if r != 44100]
        if other and not self._resample:
            raise _lib.HpfwError(f"live feeds are 44.1 kHz mono PCM16: a feed at {other[0]} Hz has to be converted before it is pushed",
                                 _lib.E_UNSUPPORTED)
        return LiveStreams(self, n_streams, min_score, window_s, hop_s, shifts, tempos, tol_cols, max_gap, min_windows, capacity_s,
                           windows, rates if other else None, min_overlap, within)

    def search(self, filenames: Sequence[str], shifts: Optional[Sequence[int]] = None,
               tempos: Optional[Sequence[float]] = None):
        """prints what the reference prints (live_song_id.h:38,47-48,53); returns (wrong, accuracy).  With shifts the
        line of a match also names its shift in bins, with tempos its shift and tempo"""
        wrong = 0
        for label, best in self.top(filenames, 1, shifts, tempos):
            print("=> Finding", label)
            if not best:
                continue
            dist, name, offset = best[0][:3]
            if os.path.splitext(os.path.basename(name))[0] not in label:
                wrong += 1
            if tempos is not None:
                print(f"=> {name} {dist} {offset} shift {best[0][3]} tempo {best[0][4]:g}\n")
            elif shifts is None:
                print(f"=> {name} {dist} {offset}\n")
            else:
                print(f"=> {name} {dist} {offset} shift {best[0][3]}\n")
        acc = 1 - wrong / float(len(filenames)) if filenames else 1.0
        print(f"=> {wrong} {acc:g}")
        return wrong, acc
