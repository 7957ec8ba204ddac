"""LiveStreams: the timelines of feeds that are still running.

LiveSongIdentification.timeline() reads a finished file; LiveSongIdentification.streams() takes the samples of any number of
feeds as they arrive.  Every window that has become complete is hashed in one extraction pass over all feeds (the rings and
their two kernels: hpfw_gpu_streams_*, k_streams.hip), searched and scored as timeline() does it, and a segmenter per feed
(hpfw_timeline_tracker) hands out each segment as soon as nothing can continue it.  A window is an independent clip, so what
a feed yields is exactly timeline() of a file that holds everything pushed to it, however the samples were cut into chunks.

Feeds are mono PCM16 at 44.1 kHz or, with rates=, at any integer rate in [8 000, 192 000] Hz.  A feed at another rate is
converted to 44.1 kHz chunk by chunk on its way into its ring (k_streams_resample.hip), the resampler's history carried from
push to push: the ring receives exactly the samples the conversion of the whole feed as one file gives, each as soon as the
last input it reads has arrived, so that such a feed yields timeline() of a file at its rate.  The last H outputs of a feed
that has ended wait for inputs that never come: tail(feed) zero samples pushed behind it bring them out.
"""
import numpy as np

from . import _lib


class LiveStreams:
    def __init__(self, lsi, n_streams, min_score, window_s=5.0, hop_s=2.5, shifts=None, tempos=None, tol_cols=None, max_gap=1,
                 min_windows=1, capacity_s=None, windows=False, rates=None, min_overlap=None, within=None):
        """within: None, or per feed the sorted slots its windows are searched within (None: the whole index), as
        LiveSongIdentification.streams() makes them from names"""
        self._lsi = lsi
        win, hop = int(round(window_s * 44100)), int(round(hop_s * 44100))
        lsi._check_min_overlap(min_overlap, shifts, tempos, win, hop)
        self._min_overlap = min_overlap
        self._lags = [{} for _ in range(n_streams)]       # overlap rule: per feed {window: lag} from the open segment's first on
        # search within sets: the restricted feeds' sets in CSR form and each feed's set (-1: none)
        self._sets = None
        if within is not None and any(w is not None for w in within):
            if min_overlap is not None:
                raise _lib.HpfwError("within: the overlap rule does not search within a set", _lib.E_UNSUPPORTED)
            lists = [w for w in within if w is not None]
            feed_set = np.cumsum([w is not None for w in within]) - 1
            self._sets = (np.concatenate([[0], np.cumsum([len(w) for w in lists])]).astype(np.int64),
                          np.array([c for w in lists for c in w], np.int32),
                          np.where([w is not None for w in within], feed_set, -1).astype(np.int32))
        self._shifts = None if shifts is None else _lib.check_shifts(shifts)
        self._tempos = None if tempos is None else _lib.check_tempos(tempos, 0 if shifts is None else len(self._shifts))
        self._windows = bool(windows)
        self._gs = None
        capacity = 0 if capacity_s is None else int(round(capacity_s * 44100))
        extractor = lsi.collector.gpu()                   # the collector's filters
        self._gs = extractor.streams(n_streams, win, hop, capacity, self._tempos, self._shifts, rates)
        m = lsi._gpu.geometry(win).m
        self._col_s = 3.0 * win / m / 44100.0             # one index column in seconds
        self._tracker_args = (min_score, hop * m / (3.0 * win), win, hop, tol_cols, max_gap, min_windows)
        self._trackers = [_lib.TimelineTracker(*self._tracker_args) for _ in range(n_streams)]
        self.n_streams, self.win, self.hop, self.capacity = n_streams, win, hop, self._gs.capacity
        self.rates = [int(r) for r in self._gs.rates]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        for t in getattr(self, "_trackers", []):
            t.close()
        if getattr(self, "_gs", None) is not None:
            self._gs.close()
            self._gs = None

    def room(self):
        """the samples every feed can take now, at the feed's rate"""
        return self._gs.room()

    def tail(self, feed):
        """the zero samples to push behind a feed that has ended so that its last outputs come out: H of its rate's filter
        (0 at 44.1 kHz).  With them the feed has given what a file of its samples gives."""
        return _lib.streams_tail(self.rates[int(feed)])

    def _variant(self, v):
        n_s = len(self._shifts) if self._shifts else 1
        j, i = divmod(max(int(v), 0), n_s)                # variant v = j max(S, 1) + i
        return (self._shifts[i] if self._shifts else 0), (self._tempos[j] if self._tempos else 1.0)

    def _tuple(self, sg, feed):
        trim = None
        if self._min_overlap is not None:                 # the extent of the first and last window on the clip
            lags = self._lags[feed]
            trim = self._lsi._trim(sg, lags[int(sg["first"])], lags[int(sg["last"])], self.win, self.hop)
        return self._lsi._segment_tuple(sg, *self._variant(sg["best_variant"]), self._col_s, trim)

    def _forget(self, feed, upto):
        """drops the lags no segment can ask for any more: those before the open segment, or all up to window `upto`"""
        cur = self._trackers[feed].open()
        keep = upto + 1 if cur is None else int(cur["first"])
        for w in [w for w in self._lags[feed] if w < keep]:
            del self._lags[feed][w]

    def push(self, chunks):
        """chunks: a list with one int16 array or None per feed (at the feed's rate), or {feed: array}.  Appends them, hashes and searches every
        window that has become complete, and returns [(feed, segment)]: the segments these windows closed, as timeline()
        returns them with start_s / end_s counted from the feed's start.  With windows=True at creation:
        (segments, [(feed, window, per-window tuple of timeline(windows=True))])."""
        if isinstance(chunks, dict):
            if any(not 0 <= int(f) < self.n_streams for f in chunks):
                raise ValueError("no such feed")
            chunks = [chunks.get(f) for f in range(self.n_streams)]
        segments, wins = [], []
        if self._gs.push(chunks):
            which, hp = self._gs.extract()
            sets = None if self._sets is None else (self._sets[0], self._sets[1], self._sets[2][which["feed"]])
            rows, per_window = self._lsi._search_windows(hp, self._shifts, self._tempos, self._min_overlap, sets)
            wins = [(int(w["feed"]), int(w["window"]), row) for w, row in zip(which, per_window)]
            if self._min_overlap is not None:
                for f, w, row in wins:
                    self._lags[f][w] = row[3]
            for feed in np.unique(which["feed"]):         # (ascending; a feed's windows are in order)
                t = self._trackers[int(feed)]
                t.push(rows[which["feed"] == feed])
                segments += [(int(feed), self._tuple(sg, int(feed))) for sg in t.pop()]
                if self._min_overlap is not None:
                    self._forget(int(feed), int(which["window"][which["feed"] == feed].max()))
        return (segments, wins) if self._windows else segments

    def open(self):
        """per feed the segment in progress as it would close now, whatever min_windows, or None"""
        cur = [t.open() for t in self._trackers]
        return [None if sg is None else self._tuple(sg, f) for f, sg in enumerate(cur)]

    def finish(self, feed=None):
        """closes the segment in progress of one feed, or of every feed, and returns [(feed, segment)] it released"""
        out = []
        for f in (range(self.n_streams) if feed is None else [int(feed)]):
            self._trackers[f].finish()
            out += [(f, self._tuple(sg, f)) for sg in self._trackers[f].pop()]
            self._lags[f].clear()
        return out

    def reset(self, feed):
        """the feed starts again at sample 0 and window 0 (a feed that reconnects); its segment in progress is dropped"""
        self._gs.reset(feed)
        self._trackers[int(feed)].close()
        self._trackers[int(feed)] = _lib.TimelineTracker(*self._tracker_args)
        self._lags[int(feed)].clear()
