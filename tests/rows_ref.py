"""Plain restatements of S6's row stage (integers only; nothing of the library or the oracle is used): the pass order of
the length-n2 transform, its fused radix groups, the loader class of the row kernel, and the row lengths n2 the planner's
split rule (tests/cols_ref.py) reaches over every clip length it accepts."""
import functools

import cols_ref

N1_MAX = 8192               # the longest column transform (plan.cpp: "clip too long" above it)
MAX_POINTS = 36             # largest fused pair (fft_rows.h kRowsMaxPoints)


def pass_order(n2):
    """passes of the row transform (plan.cpp): the descending radix list taken alternately from its front and its back,
    [7, 7, 5, 5, 4, 3] -> [7, 3, 7, 4, 5, 5], so that neighbouring passes have small products"""
    desc = cols_ref.radix_list(n2)
    out = []
    lo, hi = 0, len(desc)
    while lo < hi:
        out.append(desc[lo])
        lo += 1
        if lo < hi:
            hi -= 1
            out.append(desc[hi])
    return out


def groups(n2):
    """fused groups (r1, r2) of the row transform: neighbouring passes fused while their product is <= 36, else (r, 1)"""
    r = pass_order(n2)
    out = []
    i = 0
    while i < len(r):
        if i + 1 < len(r) and r[i] * r[i + 1] <= MAX_POINTS:
            out.append((r[i], r[i + 1]))
            i += 2
        else:
            out.append((r[i], 1))
            i += 1
    return out


def seq(n2):
    """the group sequence as tests/emu/emu_rows.cpp prints it: '7x3,5x3,5x4'"""
    return ",".join(f"{a}x{b}" for a, b in groups(n2))


def loader_class(n2):
    """which loader of rows2_body (fft_rows.h) the row length takes: 0 (n2 % 4 == 0: 16-byte pieces), 2 (n2 % 4 == 2:
    scalar path, even n2) or "odd" (scalar path)"""
    return "odd" if n2 & 1 else n2 % 4


@functools.lru_cache(maxsize=None)
def row_lengths():
    """{n2: the smallest 7-smooth n >= 54243 that the rule splits with that n2 and n1 <= 8192}, in the order of n"""
    first = {}
    for n in cols_ref.smooth_lengths(cols_ref.FIRST_LENGTH, N1_MAX * cols_ref.N2_MAX):
        n1, n2 = cols_ref.split(n)
        if n1 <= N1_MAX and n2 not in first:
            first[n2] = n
    return first
