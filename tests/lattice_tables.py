"""Vectorised numpy restatements of the host-side lattice iterators (montecarlo.jl_amd/lattices.py; the reference's
src/lattices/lattice_iterators.jl:131-190, 258-467) and of the launch plan of the current-current LDS kernel
(cc_setup, csrc/unequal_time.inl).  The package's EachSitePairByDistance is a Python double loop over all (origin,
target) pairs; the tables here are the same algorithm over all pairs at once, so that a test can afford a 24 x 24
lattice.  The device needs dir_of, ndirections(), trg_of and K only: the objects below are duck-typed stand-ins for
the package's iterators in set_pair_directions / set_local_targets / set_current_targets."""
import numpy as np

SQRT3_2 = 0.8660254037844386


def _geometry(l):
    """positions (n x D) and lattice vectors, as montecarlo.jl_amd/lattices.py has them; the lattice kind is read
    off the attributes (Lx: triangular, dim: cubic, L: square, else chain)"""
    if hasattr(l, "Lx"):
        a1, a2 = np.array([0.5, SQRT3_2]), np.array([1.0, 0.0])
        pos = np.array([a1 * (i + 1) + a2 * (j + 1) for j in range(l.Ly) for i in range(l.Lx)])
        return pos, [a1 * l.Lx, np.array([float(l.Ly), 0.0])]
    if hasattr(l, "dim"):
        if l.dim != 3:
            raise NotImplementedError("positions of CubicLattice are defined for D = 3 only")
        L = l.L
        pos = np.array([[i + 1.0, j + 1.0, k + 1.0] for k in range(L) for j in range(L) for i in range(L)])
        return pos, [np.array([float(L), 0.0, 0.0]), np.array([0.0, float(L), 0.0]), np.array([0.0, 0.0, float(L)])]
    if hasattr(l, "L"):
        L = l.L
        pos = np.array([[i + 1.0, j + 1.0] for j in range(L) for i in range(L)])
        return pos, [np.array([float(L), 0.0]), np.array([0.0, float(L)])]
    return np.arange(1.0, l.sites + 1.0)[:, None], [np.array([float(l.sites)])]


def _images(vs):
    out = [np.zeros(len(vs[0]))]
    for v in vs:
        out = [e - v for e in out] + out + [e + v for e in out]
    return out


def _directed_norm(v, eps):
    """norm + eps * angle(v, e_x) for the rows of v (the angle in two dimensions only)"""
    ln = np.sqrt((v * v).sum(axis=1))
    if v.shape[1] != 2:
        return ln
    big = ln > eps
    safe = np.where(big, ln, 1.0)
    angle = np.arccos(np.clip(v[:, 0] / safe, -1.0, 1.0))
    angle = np.where(v[:, 1] < 0, 2 * np.pi - angle, angle)
    return np.where(big, ln + eps * angle, ln)


class Tables:
    """a direction table: dir_of[src, trg] (0-based direction of the pair), ndirections(), directions"""

    def __init__(self, dir_of, nd, directions=None):
        self.dir_of = np.ascontiguousarray(dir_of, dtype=np.int32)
        self._nd = int(nd)
        self.directions = directions

    def ndirections(self):
        return self._nd


def fast_pairs(lattice, eps=1e-6):
    """EachSitePairByDistance(lattice).dir_of / ndirections() / directions: the minimal image by the same sequential
    comparison over the 3^D images, distinct displacements numbered by first occurrence (origin outer, target inner)
    and then stably sorted by directed_norm"""
    pos, vs = _geometry(lattice)
    n, D = pos.shape
    wrap = _images(vs)
    base = (pos[:, None, :] - pos[None, :, :]).reshape(n * n, D)  # row = origin * n + target
    d = base + wrap[0]
    dn = _directed_norm(d, eps)
    for v in wrap[1:]:
        new = base + v
        nn = _directed_norm(new, eps)
        take = nn + eps < dn
        d = np.where(take[:, None], new, d)
        dn = np.where(take, nn, dn)
    # displacements of different directions differ by at least half a lattice spacing; equal ones by rounding noise
    key = np.round(d, 5) + 0.0
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    by_first = np.argsort(first, kind="stable")            # unique id, in the order of first occurrence
    dirs = d[first[by_first]]
    order = np.argsort(_directed_norm(dirs, eps), kind="stable")
    rank_of_unique = np.empty(len(first), dtype=np.int64)
    rank_of_unique[by_first[order]] = np.arange(len(first))
    dir_of = rank_of_unique[inv].reshape(n, n)
    return Tables(dir_of, len(first), [dirs[k].copy() for k in order])


class QuadTables:
    """EachLocalQuadByDistance{K} / EachLocalQuadBySyncedDistance{K} as the device sees them: pairs_by_dir, trg_of
    (n x K, -1 where a source has no target in a direction) and K"""

    def __init__(self, pairs, trg_of, synced=False):
        self.pairs_by_dir = pairs
        self.trg_of = np.ascontiguousarray(trg_of, dtype=np.int32)
        self.K = int(self.trg_of.shape[1])
        self.synced = bool(synced)

    def ndirections(self):
        nd = self.pairs_by_dir.ndirections()
        return (nd, self.K) if self.synced else (nd, self.K, self.K)


def fast_quads(lattice, K=None, pairs=None, synced=False):
    """trg_of[src, k] = the target of src in direction k < K (K defaults to 1 + the number of neighbour rows)"""
    pairs = pairs if pairs is not None else fast_pairs(lattice)
    if K is None:
        K = 1 + lattice.neighs.shape[0]
    if K > pairs.ndirections():
        raise ValueError("K exceeds the number of directions of the lattice")
    n = pairs.dir_of.shape[0]
    trg_of = -np.ones((n, K), dtype=np.int32)
    for k in range(K):
        hit = pairs.dir_of == k
        cnt = hit.sum(axis=1)
        if (cnt > 1).any():
            raise ValueError("more than one target per direction: lattice with a basis is not supported")
        trg_of[:, k] = np.where(cnt == 1, hit.argmax(axis=1), -1)
    return QuadTables(pairs, trg_of, synced)


CC_KMAX = 8
CC_LDS_BUDGET = 80 * 1024


def cc_plan(n, K, W, trg_of, dir_of, nd):
    """the plan rule of cc_setup, line by line: None for the general kernel (cc_pairs_kernel), else
    dict(C, umax, nchunks, chunks_per_wg, n_wg, threads, lds_bytes) of cc_lds_kernel"""
    trg_of, dir_of = np.asarray(trg_of), np.asarray(dir_of)
    # precondition: K <= CC_KMAX, n <= 1024, n_dirs == n and, for every s1, a different direction for every s2
    if K > CC_KMAX or n > 1024 or nd != n:
        return None
    for s1 in range(n):
        if len(np.unique(dir_of[s1])) != n:
            return None
    C = 16
    while C >= 1:
        nchunks = (n + C - 1) // C
        umax = 0
        for c in range(nchunks):
            u = set()
            for s in range(c * C, min(n, (c + 1) * C)):
                u.add(s)
                u.update(int(t) for t in trg_of[s, :K] if t >= 0)
            umax = max(umax, len(u))
        lds = 8 * (2 * umax * n + n * K) + 4 * C * n
        if lds <= CC_LDS_BUDGET:
            groups = max(1, min(nchunks, (512 + W - 1) // W))  # about two workgroups per CU over all walkers
            chunks_per_wg = (nchunks + groups - 1) // groups
            n_wg = (nchunks + chunks_per_wg - 1) // chunks_per_wg
            return dict(C=C, umax=umax, nchunks=nchunks, chunks_per_wg=chunks_per_wg, n_wg=n_wg,
                        threads=min(1024, (n + 63) // 64 * 64), lds_bytes=lds)
        C //= 2
    return None


def plan_tuple(p):
    """(C, chunks, chunks per workgroup, workgroups, threads) of a cc_plan, None for the general kernel"""
    return None if p is None else (p["C"], p["nchunks"], p["chunks_per_wg"], p["n_wg"], p["threads"])
