"""LiveSongIdentification in Python: the reference's C++ class
(include/hpfw/audioproblems/live-song-id/live_song_id.h:19-60) and its notebook
(examples/python/liveid.ipynb cells 2-12) over the GPU collector and the GPU scan.

index(files)  = storage.build(collector.prepare(files))           live_song_id.h:31-33
search(files) = per query: calc_hashprint -> find -> report       live_song_id.h:35-54
top(files, k) = the notebook's "ten best tracks" per query        liveid.ipynb cell 9
"""
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .collector import ParallelCollector


class LiveSongIdentification:
    def __init__(self, cache: str = "", device: int = 0, resample: bool = False):
        """resample: index and search WAV files at any rate in [8 000, 192 000] Hz (ParallelCollector(resample=True))"""
        self.collector = ParallelCollector(resample=resample)
        self._resample = resample
        self.collector.load(cache)                       # the constructor loads the cache, live_song_id.h:24
        self._cache = cache
        self._gpu = _lib.Gpu(device)
        self.names: List[str] = []

    def close(self):
        self.collector.save(self._cache)                 # the destructor saves it, live_song_id.h:28
        self._gpu.close()

    def build(self, hashprints: Sequence[Tuple[np.ndarray, str]]):
        """MemoryStorage::build (storage.h:21-25) from prepare()'s (array, name) pairs"""
        self.names = [name for _, name in hashprints]
        self._gpu.index_clear()
        if self.names:
            off = np.zeros(len(hashprints) + 1, np.int64)
            np.cumsum([hp.size for hp, _ in hashprints], out=off[1:])
            flat = np.concatenate([hp for hp, _ in hashprints]) if off[-1] else np.zeros(1, np.uint64)
            self._gpu.index_add(flat, off)

    def index(self, filenames: Sequence[str]):
        self.build(self.collector.prepare(list(filenames)))

    def top(self, filenames: Sequence[str], k: int = 10, shifts: Optional[Sequence[int]] = None,
            tempos: Optional[Sequence[float]] = None):
        """per query (label, [(distance, name, offset) x <= k]) ordered by (distance, position in the
        database); None in place of the list for a file that yields no hashprint.  shifts: bin shifts of the query's
        constant-Q spectrogram to search as well (t semitones above the indexed recording is
        s = 2t): each clip's smallest distance over them, and every hit is (distance, name, offset, shift).  tempos:
        tempo factors (query tempo / indexed tempo) to search, each combined with every shift:
        every hit is (distance, name, offset, shift, tempo), shift 0 when shifts is None, offset in the indexed
        recording; a query too short for the slowest tempo yields None"""
        if tempos is not None:
            return self._top_tempo(list(filenames), k, None if shifts is None else list(shifts), list(tempos))
        if shifts is not None:
            return self._top_transposed(list(filenames), k, list(shifts))
        hps = self.collector.calc_hashprints(list(filenames))
        good = [i for i, (hp, _) in enumerate(hps) if hp is not None and hp.size]
        out = [(f, None) for f in filenames]
        if good and self.names:
            off = np.zeros(len(good) + 1, np.int64)
            np.cumsum([hps[i][0].size for i in good], out=off[1:])
            hits = self._gpu.search_topk(np.concatenate([hps[i][0] for i in good]), off, k)
            for row, i in zip(hits, good):
                out[i] = (filenames[i], [(int(h["dist"]), self.names[int(h["clip"])], int(h["offset"]))
                                         for h in row if h["clip"] != 0xFFFFFFFF])
        return out

    def _top_transposed(self, filenames: List[str], k: int, shifts: List[int]):
        shifts = _lib.check_shifts(shifts)
        return self._top_sets(filenames, k, len(shifts), lambda g, x: g.extract_transposed(x, shifts)[0],
                              lambda h: (shifts[int(h["shift_index"])],), "transposed")

    def _top_tempo(self, filenames: List[str], k: int, shifts: Optional[List[int]], tempos: List[float]):
        if shifts is not None:
            shifts = _lib.check_shifts(shifts)
        n_s = len(shifts) if shifts else 1
        _lib.check_tempos(tempos, 0 if shifts is None else len(shifts))

        def decode(h):
            j, i = divmod(int(h["shift_index"]), n_s)                 # variant v = j max(S, 1) + i
            return (shifts[i] if shifts else 0, tempos[j])
        return self._top_sets(filenames, k, len(tempos) * n_s, lambda g, x: g.extract_tempo(x, tempos, shifts)[0], decode,
                              "tempo")

    def _top_sets(self, filenames: List[str], k: int, n_sets: int, extract, decode, what: str):
        """the search of n_sets hashprint sets per query (extract(gpu, pcm) -> [n_sets][n_hp]) merged per clip
        (hpfw_gpu_search_topk_transposed); decode(hit) -> what a hit adds to (distance, name, offset)"""
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
            hits = self._gpu.search_topk_transposed(np.concatenate(sets), off, n_sets, k)
            for row, i in zip(hits, good):
                out[i] = (filenames[i], [(int(h["dist"]), self.names[int(h["clip"])], int(h["offset"])) + decode(h)
                                         for h in row if h["clip"] != 0xFFFFFFFF])
        return out

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
