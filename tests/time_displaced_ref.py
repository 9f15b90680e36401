"""Numpy reference of the time-displaced recording (include/dqmc_hip.h "time-displaced recording"), built on
measurement_ref.packed_step and _bin.  Like measurement_ref every function returns (value, abs_sum) per element:
abs_sum is the same sum with every factor replaced by its absolute value, the quantity a rounding bound is proportional
to.  Matrices are lists of per-block N x N arrays; dir_of[src, trg] is the 0-based direction of a pair."""
import numpy as np

import measurement_ref as MR

GREENS, DENSITY = 1, 2
DENSITY_NAMES = ("CDC", "SDCx", "SDCy", "SDCz")
_PACKED = dict(zip(DENSITY_NAMES, ("CDS", "SDSx", "SDSy", "SDSz")))


def src_of_table(dir_of, nd):
    """The host construction of dqmc_set_time_displaced: src_of[d, j] = the source i with dir_of[i, j] = d, walking the
    pairs direction by direction (sources outer, targets inner); None unless nd == n and every source and every target
    meets each direction exactly once."""
    dir_of = np.asarray(dir_of)
    n = dir_of.shape[0]
    if nd != n:
        return None
    src_of = np.full((nd, n), -1, dtype=np.int64)
    seen = np.zeros((n, nd), dtype=bool)
    for d in range(nd):
        for i, j in zip(*np.nonzero(dir_of == d)):  # row-major: i outer, j inner
            if seen[i, d] or src_of[d, j] >= 0:
                return None
            seen[i, d] = True
            src_of[d, j] = i
    return src_of


def row0_tuple(G):
    """(G00, G0l, Gl0, Gll) of row 0: (G, G - I, G, G)"""
    return G, [g - np.eye(g.shape[0]) for g in G], G, G


def greens_row(blocks, dir_of, nd):
    """[b][d] = (1/N) sum over the pairs (i, j) of direction d of blocks[b][i, j] -> (value, abs_sum), each [nb, nd]"""
    n = blocks[0].shape[0]
    va = [MR._bin(dir_of, nd, g, np.abs(g), 1.0 / n) for g in blocks]
    return np.stack([v for v, _ in va]), np.stack([a for _, a in va])


def rows(g00, steps, dir_of, nd, every=1, what=GREENS | DENSITY):
    """The sample of one walker.  steps[l - 1] = (G0l, Gl0, Gll) at l = 1..slices as the CombinedGreensIterator yields
    them.  -> {name: (value, abs_sum)} with Gl0, G0l [nb, R, nd] and CDC, SDCx, SDCy, SDCz [R, nd]"""
    assert len(steps) % every == 0
    tuples = [row0_tuple(g00)] + [(g00,) + tuple(steps[l - 1]) for l in range(every, len(steps) + 1, every)]
    out = {}
    if what & GREENS:
        for name, pos in (("Gl0", 2), ("G0l", 1)):
            va = [greens_row(t[pos], dir_of, nd) for t in tuples]
            out[name] = (np.stack([v for v, _ in va], axis=1), np.stack([a for _, a in va], axis=1))
    if what & DENSITY:
        per = [MR.packed_step(*t, dir_of, nd) for t in tuples]
        for name in DENSITY_NAMES:
            out[name] = (np.stack([p[_PACKED[name]][0] for p in per]), np.stack([p[_PACKED[name]][1] for p in per]))
    return out


def names(what):
    return (("Gl0", "G0l") if what & GREENS else ()) + (DENSITY_NAMES if what & DENSITY else ())


def size(nb, R, nd, what):
    """doubles of a sample (the accumulator has one more: the sample count)"""
    return (2 * nb * R * nd if what & GREENS else 0) + (4 * R * nd if what & DENSITY else 0)


def split(flat, nb, R, nd, what):
    """a flat sample / accumulator body in the element order of the header -> {name: array}"""
    out, off = {}, 0
    for name in names(what):
        shape = (nb, R, nd) if name in ("Gl0", "G0l") else (R, nd)
        cnt = int(np.prod(shape))
        out[name] = np.asarray(flat[off:off + cnt]).reshape(shape)
        off += cnt
    assert off == len(flat), (off, len(flat))
    return out
