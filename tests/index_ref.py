"""The rule of removal from the index in numpy: the clips named become empty, the hashprints of the
others keep their order and lie back to back, ids stay."""
import numpy as np


def remove(hp, off, ids):
    """(hp uint64 [off[-1]], off int64 [C + 1], ids: any order, repeats allowed) -> (hp', off') of the same C clips"""
    hp = np.asarray(hp, np.uint64)
    off = np.asarray(off, np.int64)
    n_clips = off.size - 1
    gone = np.zeros(n_clips, bool)
    for c in ids:
        c = int(c)
        if not 0 <= c < n_clips:
            raise ValueError(f"clip {c} outside [0, {n_clips})")
        gone[c] = True
    lengths = np.where(gone, 0, np.diff(off))
    new_off = np.concatenate([[off[0]], off[0] + np.cumsum(lengths)]).astype(np.int64)
    keep = [hp[off[c]:off[c + 1]] for c in range(n_clips) if not gone[c]]
    new_hp = np.concatenate(keep).astype(np.uint64) if keep else np.zeros(0, np.uint64)
    return new_hp, new_off


def mixed(n, seed=0):
    """n hashprints that are a mixing function of their position (splitmix64): a misplaced word shows"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + (np.uint64(seed) << np.uint64(40))) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
