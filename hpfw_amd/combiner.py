"""AudioCombiner in Python: the reference's C++ class (include/hpfw/audioproblems/combiner/combiner.h:15-132) over the
GPU Mel front end, the uint16 hashprints of HashPrint<uint16_t, MelSpectrogram<>, 32, 50> and the exact-hash inverted
index with its offset votes (hpfw_amd/csrc/k_combiner.hip).

prepare(files)  = read the WAVs, learn the filters if none are set, hashprints per file
build(pairs)    = build_db (:90-97): recordings numbered in the order given
find(hp)        = find (:100-132) with the query's own recording given as `exclude` instead of its name
align(hp, k)    = per recording the most votes on one offset and the smallest such offset, k best recordings
combine(files)  = combine (:23-33): prints what the reference prints, returns the results
"""
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


class AudioCombiner:
    def __init__(self, device: int = 0, filters: Optional[np.ndarray] = None, resample: bool = False):
        """resample: prepare() reads WAV files at any rate in [8 000, 192 000] Hz and converts them to 44.1 kHz on the GPU
        (off: 44.1 kHz only, as before)"""
        self._gpu = _lib.Gpu(device)
        self._resample = resample
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
