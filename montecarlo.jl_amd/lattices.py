"""Host-side lattices (src/lattices/square.jl:25-60, chain.jl:19-41, cubic.jl:19-70, triangular.jl:1-119,
abstract.jl:99-115).

Integer tables are 1-based like the reference's so that they compare verbatim with
its fixtures (test/flavortests_DQMC.jl:22-24)."""
import numpy as np


class AbstractLattice:
    def __len__(self):
        return self.sites

    def neighbors(self, directed=False):
        """neighbors(l, Val(directed)), src/lattices/abstract.jl:99-108"""
        if directed:  # src-major, then the rows of neighs
            return [(src + 1, int(trg)) for src in range(self.sites) for trg in self.neighs[:, src]]
        return [(int(b[0]), int(b[1])) for b in self.bonds]


class SquareLattice(AbstractLattice):
    """SquareLattice(L): neighs rows = up, right, down, left (square.jl:47-60).  nnn rows = upright, downright, downleft,
    upleft: the four next-nearest (diagonal) neighbours, built with the same circshift convention (an extension: the
    reference's square lattice has no such table)."""

    def __init__(self, L):
        self.L = L
        self.sites = L * L
        lat = np.arange(1, L * L + 1).reshape((L, L), order="F")
        self.lattice = lat
        up = np.roll(lat, -1, axis=0)       # circshift(lattice, (-1, 0))
        right = np.roll(lat, -1, axis=1)    # circshift(lattice, (0, -1))
        down = np.roll(lat, 1, axis=0)
        left = np.roll(lat, 1, axis=1)
        self.neighs = np.vstack([x.reshape(-1, order="F") for x in (up, right, down, left)]).astype(np.int64)
        diag = [np.roll(lat, s, axis=(0, 1)) for s in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        self.nnn = np.vstack([x.reshape(-1, order="F") for x in diag]).astype(np.int64)
        self.n_bonds = 2 * self.sites
        bonds = np.zeros((self.n_bonds, 3), dtype=np.int64)
        b = 0
        for src in lat.reshape(-1, order="F"):
            bonds[b] = (src, self.neighs[0, src - 1], 0); b += 1
            bonds[b] = (src, self.neighs[1, src - 1], 0); b += 1
        self.bonds = bonds

    def next_neighbors(self, directed=False):
        """the diagonal neighbours as neighbors() lists the nearest ones: directed, src-major (src, trg) over the rows of
        nnn; else every diagonal bond once (src, its upright and its downright neighbour)"""
        rows = self.nnn if directed else self.nnn[:2]
        return [(src + 1, int(trg)) for src in range(self.sites) for trg in rows[:, src]]


class RectangularLattice(AbstractLattice):
    """RectangularLattice(Lx, Ly): the periodic Lx x Ly square-net torus, site 1 + x + Lx y (x fastest; column-major reshape
    of 1:Lx*Ly to (Lx, Ly)).  neighs rows = up (x + 1), right (y + 1), down, left; nnn rows = upright, downright, downleft,
    upleft; bonds = up and right of every source (2 Lx Ly rows; along an axis of length 2 the coinciding neighbours stand
    twice): SquareLattice's circshift convention throughout, and RectangularLattice(L, L) has SquareLattice(L)'s tables.
    An extension: the reference has no such lattice.  Not a SquareLattice: it has no single L, so no `isinstance(l,
    SquareLattice)` branch takes it by accident."""

    def __init__(self, Lx, Ly):
        Lx, Ly = int(Lx), int(Ly)
        if Lx < 2 or Ly < 2:
            raise ValueError("RectangularLattice: Lx and Ly must be at least 2 (Lx = %d, Ly = %d)" % (Lx, Ly))
        self.Lx, self.Ly = Lx, Ly
        self.sites = Lx * Ly
        lat = np.arange(1, self.sites + 1).reshape((Lx, Ly), order="F")
        self.lattice = lat
        near = [np.roll(lat, -1, axis=0), np.roll(lat, -1, axis=1), np.roll(lat, 1, axis=0), np.roll(lat, 1, axis=1)]
        self.neighs = np.vstack([x.reshape(-1, order="F") for x in near]).astype(np.int64)
        diag = [np.roll(lat, s, axis=(0, 1)) for s in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        self.nnn = np.vstack([x.reshape(-1, order="F") for x in diag]).astype(np.int64)
        self.n_bonds = 2 * self.sites
        bonds = np.zeros((self.n_bonds, 3), dtype=np.int64)
        b = 0
        for src in lat.reshape(-1, order="F"):
            bonds[b] = (src, self.neighs[0, src - 1], 0); b += 1
            bonds[b] = (src, self.neighs[1, src - 1], 0); b += 1
        self.bonds = bonds

    next_neighbors = SquareLattice.next_neighbors


class Chain(AbstractLattice):
    """Chain(nsites): neighs rows = right, left (chain.jl:36-41)."""

    def __init__(self, nsites):
        self.sites = nsites
        c = np.arange(1, nsites + 1)
        self.neighs = np.vstack([np.roll(c, -1), np.roll(c, 1)]).astype(np.int64)
        self.n_bonds = nsites
        self.bonds = np.array([(s, self.neighs[0, s - 1], 0) for s in c], dtype=np.int64)


class CubicLattice(AbstractLattice):
    """CubicLattice(D, L) (cubic.jl:23-56): site x_1 + L x_2 + L^2 x_3 + ... (column-major reshape of 1:L^D); neighs rows
    1..D are the "uprights" (circshift by -1 along dimension d), rows D+1..2D the "downlefts"."""

    def __init__(self, D, L):
        self.L, self.dim = L, D
        self.sites = L ** D
        lat = np.arange(1, self.sites + 1).reshape((L,) * D, order="F")
        self.lattice = lat
        ups = [np.roll(lat, -1, axis=d).reshape(-1, order="F") for d in range(D)]
        downs = [np.roll(lat, 1, axis=d).reshape(-1, order="F") for d in range(D)]
        self.neighs = np.vstack(ups + downs).astype(np.int64)
        self.n_bonds = D * self.sites
        bonds = np.zeros((self.n_bonds, 3), dtype=np.int64)
        b = 0
        for src in lat.reshape(-1, order="F"):
            for trg in self.neighs[:D, src - 1]:
                bonds[b] = (src, trg, 0); b += 1
        self.bonds = bonds


class TriangularLattice(AbstractLattice):
    """TriangularLattice(L; Lx=L, Ly=L) (triangular.jl:24-57): site i + Lx (j - 1) (column-major reshape of 1:Lx*Ly);
    neighs rows = up (i+1), upright (i+1, j+1), right (j+1), down, downleft, left (Julia circshift semantics, :60-78);
    ext_neighs the same rows two steps away (R + 2a, :81-99).  The bonds table lists neighs[1:3] then ext_neighs[1:3] for
    each source; the hopping matrix takes neighs only, so the ext bonds carry no hopping.  Kept as the reference has them:
    positions() puts upright at distance sqrt(3), and the geometric nearest neighbour (i+1, j-1) is no hopping neighbour
    (DESIGN 4.7)."""

    def __init__(self, L, Lx=None, Ly=None):
        Lx = L if Lx is None else Lx
        Ly = L if Ly is None else Ly
        self.L, self.Lx, self.Ly = L, Lx, Ly
        self.sites = Lx * Ly
        lat = np.arange(1, self.sites + 1).reshape((Lx, Ly), order="F")
        self.lattice = lat

        def table(k):  # circshift(lattice, (-k, 0)), (-k, -k), (0, -k), (k, 0), (k, k), (0, k)
            shifts = ((-k, 0), (-k, -k), (0, -k), (k, 0), (k, k), (0, k))
            cart = np.stack([np.roll(lat, s, axis=(0, 1)) for s in shifts])
            return np.vstack([c.reshape(-1, order="F") for c in cart]).astype(np.int64), cart
        self.neighs, self.neighs_cartesian = table(1)
        self.ext_neighs, self.ext_neighs_cartesian = table(2)
        self.isAsite = np.array([(i + 1) % 2 == 0 for j in range(Ly) for i in range(Lx)])
        self.n_bonds = 6 * self.sites
        bonds = np.zeros((self.n_bonds, 3), dtype=np.int64)
        b = 0
        for src in lat.reshape(-1, order="F"):
            for trg in list(self.neighs[:3, src - 1]) + list(self.ext_neighs[:3, src - 1]):
                bonds[b] = (src, trg, 0); b += 1
        self.bonds = bonds


class BilayerSquareLattice(AbstractLattice):
    """BilayerSquareLattice(L): two periodic L x L square layers, site 1 + x + L y + L^2 z (z = 0, 1 the layer; column-major
    reshape of 1:2 L^2 to (L, L, 2)).  neighs rows = up, right, down, left inside the layer (the SquareLattice circshift
    convention, per layer), then perp: the same (x, y) in the other layer.  The bonds table lists up and right for every
    source and perp for the sources of layer 0, so every physical bond stands once (5 L^2; at L = 2 the periodic in-plane
    bonds count twice, as on SquareLattice(2)).  On the torus Z_L x Z_L x Z_2 it is a Bravais lattice with the layer swap
    as its z translation: one target per direction, as many directions as sites.  An extension: the reference has no such
    lattice.  Not a SquareLattice: no nnn table, no t'."""

    def __init__(self, L):
        self.L = L
        self.sites = 2 * L * L
        lat = np.arange(1, self.sites + 1).reshape((L, L, 2), order="F")
        self.lattice = lat
        rows = [np.roll(lat, -1, axis=0), np.roll(lat, -1, axis=1), np.roll(lat, 1, axis=0), np.roll(lat, 1, axis=1),
                lat[:, :, ::-1]]
        self.neighs = np.vstack([x.reshape(-1, order="F") for x in rows]).astype(np.int64)
        self.n_bonds = 5 * L * L
        bonds = np.zeros((self.n_bonds, 3), dtype=np.int64)
        b = 0
        for src in lat.reshape(-1, order="F"):
            bonds[b] = (src, self.neighs[0, src - 1], 0); b += 1
            bonds[b] = (src, self.neighs[1, src - 1], 0); b += 1
            if src <= L * L:
                bonds[b] = (src, self.neighs[4, src - 1], 0); b += 1
        self.bonds = bonds


class HoneycombLattice(AbstractLattice):
    """HoneycombLattice(L): L x L periodic cells of two sites, 2 L^2 sites.  Geometry of the reference's positions
    (honeycomb.jl:130-135): v1 = (sqrt(3)/2, -1/2), v2 = (sqrt(3)/2, 1/2), the B site of a cell at (1/sqrt(3), 0) from
    its A site.  Site order as that comprehension lists them: the sublattice o runs fastest, then y, then x, so site
    1 + o + 2 (y + L x) sits at o b + x v1 + y v2 (x, y = 0 .. L - 1, o = 0: A, 1: B).  neighs has 3 rows: for an A site of
    cell R the B sites of cells R, R - v1 and R - v2 (periodic); for a B site the three inverse steps, the A sites of R,
    R + v1 and R + v2.  bonds lists the three rows of every A source: every physical bond once, 3 L^2 rows.  At L = 1 the
    three neighbours of a site coincide and count three times in the hopping matrix (T[0, 1] = -3 t), as the periodic
    bonds of SquareLattice(2) count twice.  `sublattice` is 0 on A and 1 on B, isAsite its negation; `lattice` [x, y, o]
    holds the site of a cell coordinate.  An extension: the reference's honeycomb.jl is commented out and keeps other
    tables.  A lattice with a basis: 3 L^2 directions (EachSitePairByDistance), not one per site."""

    def __init__(self, L):
        self.L = L
        self.sites = 2 * L * L
        lat = np.zeros((L, L, 2), dtype=np.int64)
        for x in range(L):
            for y in range(L):
                for o in range(2):
                    lat[x, y, o] = 1 + o + 2 * (y + L * x)
        self.lattice = lat
        self.sublattice = np.array([i % 2 for i in range(self.sites)], dtype=np.int64)
        self.isAsite = self.sublattice == 0
        neighs = np.zeros((3, self.sites), dtype=np.int64)
        for x in range(L):
            for y in range(L):
                a, b = lat[x, y, 0] - 1, lat[x, y, 1] - 1
                neighs[:, a] = (lat[x, y, 1], lat[(x - 1) % L, y, 1], lat[x, (y - 1) % L, 1])
                neighs[:, b] = (lat[x, y, 0], lat[(x + 1) % L, y, 0], lat[x, (y + 1) % L, 0])
        self.neighs = neighs
        self.n_bonds = 3 * L * L
        bonds = np.zeros((self.n_bonds, 3), dtype=np.int64)
        b = 0
        for src in range(1, self.sites + 1, 2):  # the A sites, ascending
            for trg in neighs[:, src - 1]:
                bonds[b] = (src, trg, 0); b += 1
        self.bonds = bonds


HONEYCOMB_V1 = np.array([0.8660254037844386, -0.5])
HONEYCOMB_V2 = np.array([0.8660254037844386, 0.5])
HONEYCOMB_B = np.array([0.5773502691896258, 0.0])


def strip_subsystem(lattice, width, axis=0):
    """The 0-based sites, ascending, whose integer coordinate along `axis` is below `width`: the strip subsystem of an
    entanglement cut (DQMC.set_entanglement), for SquareLattice, RectangularLattice, CubicLattice, TriangularLattice and
    BilayerSquareLattice, whose `lattice` array carries the coordinates (axis 0 runs fastest in the site index).  On a HoneycombLattice the
    coordinates are the cell coordinates (x, y) along v1 and v2 (axis 0 or 1): both sublattice sites of a cell belong to
    the strip."""
    if isinstance(lattice, HoneycombLattice):
        if int(axis) not in (0, 1):
            raise ValueError("strip_subsystem: axis %r of a HoneycombLattice (0 or 1: the cell coordinates)" % (axis,))
        if not 1 <= int(width) <= lattice.L:
            raise ValueError("strip_subsystem: width %r outside 1 .. %d" % (width, lattice.L))
        return np.sort(np.take(lattice.lattice, np.arange(int(width)), axis=int(axis)).reshape(-1)).astype(np.int64) - 1
    if not isinstance(lattice, (SquareLattice, RectangularLattice, CubicLattice, TriangularLattice, BilayerSquareLattice)):
        raise TypeError("strip_subsystem: SquareLattice, RectangularLattice, CubicLattice, TriangularLattice or "
                        "BilayerSquareLattice, not %s" % type(lattice).__name__)
    lat = lattice.lattice
    if not 0 <= int(axis) < lat.ndim:
        raise ValueError("strip_subsystem: axis %r of a %d-dimensional lattice" % (axis, lat.ndim))
    if not 1 <= int(width) <= lat.shape[int(axis)]:
        raise ValueError("strip_subsystem: width %r outside 1 .. %d" % (width, lat.shape[int(axis)]))
    return np.sort(np.take(lat, np.arange(int(width)), axis=int(axis)).reshape(-1)).astype(np.int64) - 1


def build_checkerboard(l):
    """src/flavors/DQMC/abstract.jl:23-54 (used here only to pin the bond tables)."""
    bonds = l.neighbors(False)
    n_bonds = len(bonds)
    edges_used = np.zeros(n_bonds, dtype=np.int64)
    cb = np.zeros((3, n_bonds), dtype=np.int64)
    groups = []
    gs = ge = 1
    while edges_used.min() == 0:
        sites_used = np.zeros(len(l), dtype=np.int64)
        for idx, (src, trg) in enumerate(bonds):
            if edges_used[idx] or sites_used[src - 1] or sites_used[trg - 1]:
                continue
            edges_used[idx] = sites_used[src - 1] = sites_used[trg - 1] = 1
            cb[:, ge - 1] = (src, trg, idx + 1)
            ge += 1
        groups.append((gs, ge - 1))
        gs = ge
    return cb, groups, len(groups)


# ---------------------------------------------------------------------------
# EachSitePairByDistance (src/lattices/lattice_iterators.jl:131-190)
def _check_cubic(l):
    if l.dim != 3:  # cubic.jl:69-70 define positions and lattice_vectors for D = 3 only
        raise NotImplementedError("positions / lattice_vectors of CubicLattice are defined for D = 3 only (D = %d)" % l.dim)


def _positions(l):
    """positions(l) (square.jl:72, chain.jl:52, cubic.jl:69, triangular.jl:113-116): cartesian coordinates"""
    if isinstance(l, TriangularLattice):  # a1 = (0.5, sqrt(3) / 2) along i, a2 = (1, 0) along j, 1-based (i, j)
        a1, a2 = np.array([0.5, 0.8660254037844386]), np.array([1.0, 0.0])
        return [a1 * (i + 1) + a2 * (j + 1) for j in range(l.Ly) for i in range(l.Lx)]
    if isinstance(l, SquareLattice):
        return [np.array([i + 1.0, j + 1.0]) for j in range(l.L) for i in range(l.L)]
    if isinstance(l, RectangularLattice):
        return [np.array([i + 1.0, j + 1.0]) for j in range(l.Ly) for i in range(l.Lx)]
    if isinstance(l, CubicLattice):
        _check_cubic(l)
        return [np.array([i + 1.0, j + 1.0, k + 1.0]) for k in range(l.L) for j in range(l.L) for i in range(l.L)]
    if isinstance(l, BilayerSquareLattice):
        return [np.array([i + 1.0, j + 1.0, k + 1.0]) for k in range(2) for j in range(l.L) for i in range(l.L)]
    if isinstance(l, HoneycombLattice):  # honeycomb.jl:130-135
        return [o * HONEYCOMB_B + HONEYCOMB_V1 * x + HONEYCOMB_V2 * y for x in range(l.L) for y in range(l.L) for o in range(2)]
    return [np.array([i + 1.0]) for i in range(l.sites)]


def _lattice_vectors(l):
    if isinstance(l, TriangularLattice):  # triangular.jl:118
        return [np.array([0.5, 0.8660254037844386]) * l.Lx, np.array([float(l.Ly), 0.0])]
    if isinstance(l, SquareLattice):
        return [np.array([float(l.L), 0.0]), np.array([0.0, float(l.L)])]
    if isinstance(l, RectangularLattice):
        return [np.array([float(l.Lx), 0.0]), np.array([0.0, float(l.Ly)])]
    if isinstance(l, CubicLattice):
        _check_cubic(l)
        return [np.array([float(l.L), 0.0, 0.0]), np.array([0.0, float(l.L), 0.0]), np.array([0.0, 0.0, float(l.L)])]
    if isinstance(l, BilayerSquareLattice):  # the layer swap is the z translation: period 2
        return [np.array([float(l.L), 0.0, 0.0]), np.array([0.0, float(l.L), 0.0]), np.array([0.0, 0.0, 2.0])]
    if isinstance(l, HoneycombLattice):
        return [HONEYCOMB_V1 * l.L, HONEYCOMB_V2 * l.L]
    return [np.array([float(l.sites)])]


def _slot_displacements(l, eps=1e-9):
    """-> images[k][i]: the minimum-image displacements r_j - r_i of the directed slot (i, k), j = neighs[k, i], as a list
    of vectors: one, or several of equal length where the lattice has a period of 2 along the bond (both +v and -v are
    minimum images).  The first entry is the image nearest to the unwrapped difference of the positions, so that of the
    two slots of such a pair one points each way.  From the lattice's own row semantics: _positions and _lattice_vectors;
    a CubicLattice with D != 3 has neither, and its rows are +e_d (d < D) and -e_d by construction."""
    nb = np.asarray(l.neighs, dtype=np.int64) - 1
    z, N = nb.shape
    if isinstance(l, CubicLattice) and l.dim != 3:
        D = l.dim
        out = []
        for k in range(z):
            v = np.zeros(D)
            v[k % D] = 1.0 if k < D else -1.0
            out.append([[v.copy(), -v] if l.L == 2 else [v.copy()] for _ in range(N)])
        return out
    pos = np.array(_positions(l), dtype=np.float64)
    wrap = np.array(generate_combinations(_lattice_vectors(l)), dtype=np.float64)
    out = []
    for k in range(z):
        raw = pos[nb[k]] - pos                              # [N][dim]
        cand = raw[None, :, :] + wrap[:, None, :]           # [images][N][dim]
        norms = np.linalg.norm(cand, axis=2)
        tied = norms <= norms.min(axis=0)[None, :] + eps
        row = []
        for i in range(N):
            c = cand[tied[:, i], i]
            if len(c) > 1:  # nearest to the unwrapped difference first (stable), duplicates dropped
                c = c[np.argsort(np.linalg.norm(c - raw[i], axis=1), kind="stable")]
                uniq = []
                for v in c:
                    if not any(np.linalg.norm(v - u) <= eps for u in uniq):
                        uniq.append(v)
                c = uniq
            row.append(list(c))
        out.append(row)
    return out


def bond_classes(l, directions=True, eps=1e-9):
    """-> (slot_class int8 [z, N], class vectors [n_c, dim], x [n_dir, n_c]): the bond displacement classes of a lattice
    for the helicity modulus (include/dqmc_hip.h, "Stiffness" of the q-state section; QStateMC.set_stiffness).

    A directed slot is (i, k) with j = neighs[k, i]; its displacement is r_j - r_i at minimum image.  A class is a
    displacement vector in its canonical orientation of +-v, the one whose first non-zero component is positive; a slot
    is counted (slot_class >= 0) iff its displacement is the canonical one, so that every undirected neighbour pair is
    counted once; the other slots hold -1.  Classes are numbered in the order they first appear, rows of neighs first.
    `directions`: 1 to 4 unit vectors of the lattice's dimension, or True for its cartesian axes (at most 4; on a
    BilayerSquareLattice the two in-plane axes: the layer index has period 2 and carries no twist);
    x[mu][c] = directions[mu] . v_c.  Where the lattice has a period of 2 along a bond, +v and -v are both minimum
    images: fine while every requested direction sees the same projection, a ValueError otherwise (SquareLattice(2)
    along x).  TriangularLattice: the rows of neighs only, not the two-step bonds of ext_neighs."""
    images = _slot_displacements(l, eps)
    z, N = len(images), len(images[0])
    dim = len(images[0][0][0])
    if directions is True:
        n_axes = 2 if isinstance(l, BilayerSquareLattice) else min(dim, 4)
        dirs = np.eye(dim)[:n_axes]
    else:
        dirs = np.array(directions, dtype=np.float64)
        if dirs.ndim != 2 or dirs.shape[1] != dim or not 1 <= dirs.shape[0] <= 4:
            raise ValueError("bond_classes: 1 to 4 direction vectors of dimension %d, got an array of shape %r"
                             % (dim, dirs.shape))
        if not np.all(np.isfinite(dirs)) or np.any(np.abs(np.linalg.norm(dirs, axis=1) - 1.0) > 1e-9):
            raise ValueError("bond_classes: the directions must be finite unit vectors")
    slot_class = -np.ones((z, N), dtype=np.int8)
    vectors = []
    for k in range(z):
        for i in range(N):
            v = images[k][i][0]
            lead = next((c for c in v if abs(c) > eps), 0.0)
            if lead <= 0.0:
                continue  # the reverse slot is the counted one
            for other in images[k][i][1:]:
                if np.any(np.abs(dirs @ (other - v)) > eps):
                    raise ValueError("bond_classes: the displacement of the bond (%d, %d) (1-based) is ambiguous along a "
                                     "requested direction: the lattice has a period of 2 there" % (i + 1, l.neighs[k, i]))
            c = next((n for n, u in enumerate(vectors) if np.linalg.norm(u - v) <= eps), None)
            if c is None:
                vectors.append(np.array(v, dtype=np.float64))
                c = len(vectors) - 1
            slot_class[k, i] = c
    if not 1 <= len(vectors) <= 8:
        raise ValueError("bond_classes: %d displacement classes (the engine takes 1 to 8)" % len(vectors))
    vectors = np.array(vectors, dtype=np.float64)
    return slot_class, vectors, np.ascontiguousarray(dirs @ vectors.T)


def momentum_grid(l):
    """-> (q [N, dim], labels [N, dim]): the N wave vectors a periodic lattice of N sites allows, cartesian, and their
    integer labels.  With A_i = _lattice_vectors(l), the vectors the lattice is periodic under, the reciprocal basis is
    G_j with A_i . G_j = 2 pi delta_ij, and q = sum_j m_j G_j, m_j = 0 .. L_j - 1 (L_j the number of sites along A_j);
    the first label runs fastest.  Chain, SquareLattice, RectangularLattice (counts (Lx, Ly)), CubicLattice (D = 3),
    TriangularLattice and BilayerSquareLattice (counts (L, L, 2): q_z = 0 and pi are the bonding and antibonding combinations of the layers); on a HoneycombLattice
    the L^2 cell momenta (counts (L, L), A = L v1, L v2), N = sites / 2."""
    A = np.array(_lattice_vectors(l), dtype=np.float64)  # rows A_i
    if isinstance(l, (TriangularLattice, RectangularLattice)):
        counts = (l.Lx, l.Ly)
    elif isinstance(l, BilayerSquareLattice):
        counts = (l.L, l.L, 2)
    elif isinstance(l, HoneycombLattice):  # the L^2 cell momenta: the two sublattice sites share them
        counts = (l.L, l.L)
    elif isinstance(l, (SquareLattice, CubicLattice)):
        counts = (l.L,) * A.shape[0]
    else:
        counts = (l.sites,)
    G = 2.0 * np.pi * np.linalg.inv(A).T  # rows G_j
    labels = np.array([m[::-1] for m in np.ndindex(*counts[::-1])], dtype=np.int64).reshape(-1, len(counts))
    return labels.astype(np.float64) @ G, labels


def default_pair_channels(lattice, directions, K):
    """-> {name: weights f[k], k < K} over the K shortest directions (`directions[k]` the displacement, k = 0 on-site):
    s = e_0; s* = 1/2 on every nearest neighbour (the shortest non-zero directions among the K; the same 1/2 on every
    lattice, no 1/sqrt(z)); on a SquareLattice or RectangularLattice also d = +1/2 on the bonds along x and -1/2 on those along y.  On a
    BilayerSquareLattice the five nearest neighbours all have length 1 and are told apart by their z component: s* and d
    take the four in-plane ones, and s_perp = 1 on the interlayer direction, which is its own inverse on the two-layer torus
    (the 1 stands for the 1/2 + 1/2 of a +- pair).  On a HoneycombLattice with K = 7 the six shortest non-zero directions
    are the three A -> B and the three B -> A bonds: s* is 1/2 on all six, so every site sees weight 1/2 on each of its
    three bonds (its other three directions have no target); s and s* only."""
    r = np.asarray(directions, dtype=np.float64)[:K]
    nrm = np.linalg.norm(r, axis=1)
    if K < 1 or nrm[0] > 1e-9:
        raise ValueError("direction 0 must be the on-site one")
    s = np.zeros(K)
    s[0] = 1.0
    res = {"s": s}
    if isinstance(lattice, BilayerSquareLattice):
        nn = np.isclose(nrm, 1.0)
        perp = nn & (np.abs(r[:, 2]) > 0.5)
        inplane = nn & ~perp
        if inplane.sum() != 4 or perp.sum() != 1:
            raise ValueError("the bilayer channels need the four in-plane nearest neighbours and the interlayer one among the K directions")
        res["s*"] = np.where(inplane, 0.5, 0.0)
        res["d"] = np.where(inplane, np.where(np.abs(r[:, 0]) > np.abs(r[:, 1]), 0.5, -0.5), 0.0)
        res["s_perp"] = np.where(perp, 1.0, 0.0)
        return res
    if K > 1:
        nn = np.isclose(nrm, nrm[1:].min())
        res["s*"] = np.where(nn, 0.5, 0.0)
        if isinstance(lattice, (SquareLattice, RectangularLattice)):
            if nn.sum() != 4:
                raise ValueError("the d channel needs the four nearest neighbours among the K directions")
            res["d"] = np.where(nn, np.where(np.abs(r[:, 0]) > np.abs(r[:, 1]), 0.5, -0.5), 0.0)
    return res


def generate_combinations(vs):
    """lattice_iterators.jl:137-143: all periodic images, in the reference's order"""
    out = [np.zeros(len(vs[0]))]
    for v in vs:
        out = [e - v for e in out] + out + [e + v for e in out]
    return out


def directed_norm(v, eps):
    """norm + eps * angle(v, e_x) (lattice_iterators.jl:146-155)"""
    ln = float(np.linalg.norm(v))
    if len(v) == 2 and ln > eps:
        angle = float(np.arccos(v[0] / ln))
        if v[1] < 0:
            angle = 2 * np.pi - angle
        return ln + eps * angle
    return ln


class EachSitePairByDistance:
    """Triplets (direction index, source, target) sorted by distance.  `pairs[d]` lists the 1-based
    (src, trg) pairs of direction d in the reference's order; `dir_of[src-1, trg-1]` is the 0-based
    direction index of a pair; `directions[d]` the displacement vector."""

    def __init__(self, lattice, eps=1e-6):
        pos = _positions(lattice)
        wrap = generate_combinations(_lattice_vectors(lattice))
        directions, bonds = [], []
        for origin in range(len(lattice)):
            for trg, p in enumerate(pos):
                d = pos[origin] - p + wrap[0]
                for v in wrap[1:]:
                    new_d = pos[origin] - p + v
                    if directed_norm(new_d, eps) + eps < directed_norm(d, eps):
                        d = new_d
                idx = next((k for k, dd in enumerate(directions) if np.linalg.norm(dd - d) <= eps), None)
                if idx is None:
                    directions.append(d.copy())
                    bonds.append([])
                    idx = len(directions) - 1
                bonds[idx].append((origin + 1, trg + 1))
        order = sorted(range(len(directions)), key=lambda k: directed_norm(directions[k], eps))  # stable
        self.directions = [directions[k] for k in order]
        self.pairs = [bonds[k] for k in order]
        self.N = len(lattice) ** 2
        n = len(lattice)
        self.dir_of = np.zeros((n, n), dtype=np.int32)
        for d, prs in enumerate(self.pairs):
            for s, t in prs:
                self.dir_of[s - 1, t - 1] = d

    def __len__(self):
        return self.N

    def ndirections(self):
        return len(self.pairs)

    def __iter__(self):
        for d, prs in enumerate(self.pairs):
            for s, t in prs:
                yield d + 1, s, t


def _default_K(lattice):
    """the default K of the quad iterators: on-site plus one direction per neighbour row.  On a HoneycombLattice the
    three A -> B and the three B -> A nearest directions are distinct, so K = 1 + 2 * 3: every source then has its three
    neighbours among its targets (and no target in the other three directions: trg_of == -1 there)."""
    if isinstance(lattice, HoneycombLattice):
        return 1 + 2 * lattice.neighs.shape[0]
    return 1 + lattice.neighs.shape[0]


def sublattice_sign(iterator, lattice):
    """-> [n_dirs] of +1.0 / -1.0 over the directions of an EachSitePairByDistance (or anything with dir_of and
    ndirections()): +1 where a direction joins sites of the same sublattice, -1 where it joins A and B.  The q = 0
    transform with these signs is the staggered (antiferromagnetic) one.  Needs a lattice with a `sublattice` array
    (HoneycombLattice); a direction that mixed both kinds of pair would be an error of the table."""
    sub = getattr(lattice, "sublattice", None)
    if sub is None:
        raise TypeError("sublattice_sign: %s has no sublattice array" % type(lattice).__name__)
    sub = np.asarray(sub)
    dir_of = np.asarray(iterator.dir_of)
    nd = int(iterator.ndirections())
    pair_sign = np.where(sub[:, None] == sub[None, :], 1.0, -1.0)
    sign = np.zeros(nd)
    for s in (1.0, -1.0):
        hit = np.unique(dir_of[pair_sign == s])
        if np.any(sign[hit] != 0.0):
            raise ValueError("sublattice_sign: a direction joins both kinds of pair")
        sign[hit] = s
    if np.any(sign == 0.0):
        raise ValueError("sublattice_sign: a direction without pairs")
    return sign


class EachLocalQuadByDistance:
    """EachLocalQuadByDistance{K}(lattice) (src/lattices/lattice_iterators.jl:258-353): quadruples
    (src1, trg1, src2, trg2) where trg_k is reached from src_k in one of the K shortest directions,
    grouped by (dir12, dir1, dir2) with dir12 the direction index of the pair (src1, src2).
    `trg_from_src[src-1]` lists the 1-based (dir, trg) of a source in the reference's order;
    `trg_of[src-1, k]` is the 0-based target in direction k (-1 if the site has none; sites of a
    Bravais lattice have exactly one per direction)."""

    def __init__(self, lattice, K=None, pairs=None):
        self.pairs_by_dir = pairs if pairs is not None else EachSitePairByDistance(lattice)
        n = len(lattice)
        if K is None:  # pairing(): K = 1 + length(neighbors(lattice, 1)) (measurements.jl:199-204)
            K = _default_K(lattice)
        if K > self.pairs_by_dir.ndirections():
            raise ValueError("K exceeds the number of directions of the lattice")
        self.K = K
        self.trg_from_src = [[] for _ in range(n)]
        for d in range(K):
            for src, trg in self.pairs_by_dir.pairs[d]:
                self.trg_from_src[src - 1].append((d + 1, trg))
        self.N = sum(len(x) for x in self.trg_from_src) ** 2
        self.trg_of = -np.ones((n, K), dtype=np.int32)
        for src, lst in enumerate(self.trg_from_src):
            for d, trg in lst:
                if self.trg_of[src, d - 1] >= 0:
                    raise ValueError("more than one target per direction: lattice with a basis is not supported")
                self.trg_of[src, d - 1] = trg - 1

    def __len__(self):
        return self.N

    def ndirections(self):
        return (self.pairs_by_dir.ndirections(), self.K, self.K)

    def __iter__(self):
        """(lin, src1, trg1, src2, trg2), lin the 1-based linear index of (dir12, dir1, dir2)"""
        nd, K = self.pairs_by_dir.ndirections(), self.K
        for d2 in range(K):
            for d1 in range(K):
                for d12 in range(nd):
                    lin = 1 + d12 + nd * (d1 + K * d2)
                    for src1, src2 in self.pairs_by_dir.pairs[d12]:
                        for dir1, trg1 in self.trg_from_src[src1 - 1]:
                            if dir1 != d1 + 1:
                                continue
                            for dir2, trg2 in self.trg_from_src[src2 - 1]:
                                if dir2 == d2 + 1:
                                    yield lin, src1, trg1, src2, trg2


class EachLocalQuadBySyncedDistance:
    """EachLocalQuadBySyncedDistance{K}(lattice) (src/lattices/lattice_iterators.jl:360-467): quadruples
    (src1, trg1, src2, trg2) whose two targets are reached in the same direction dir_ii, one of the K
    shortest, grouped by (dir12, dir_ii) with dir12 the direction index of the pair (src1, src2).
    `trg_from_src` and `trg_of` as in EachLocalQuadByDistance; `implied[d12][k]` lists the 1-based quads
    of one cell in the order the reference's `while` loop pushes them (built on first use)."""

    def __init__(self, lattice, K=None, pairs=None):
        self.pairs_by_dir = pairs if pairs is not None else EachSitePairByDistance(lattice)
        n = len(lattice)
        if K is None:  # current_current_susceptibility(): K = 1 + length(neighbors(lattice, 1)) (measurements.jl:257-263)
            K = _default_K(lattice)
        if K > self.pairs_by_dir.ndirections():
            raise ValueError("K exceeds the number of directions of the lattice")
        self.K = K
        self.trg_from_src = [[] for _ in range(n)]
        for d in range(K):
            for src, trg in self.pairs_by_dir.pairs[d]:
                self.trg_from_src[src - 1].append((d + 1, trg))
        self.trg_of = -np.ones((n, K), dtype=np.int32)
        for src, lst in enumerate(self.trg_from_src):
            for d, trg in lst:
                if self.trg_of[src, d - 1] >= 0:
                    raise ValueError("more than one target per direction: lattice with a basis is not supported")
                self.trg_of[src, d - 1] = trg - 1
        # every pair (src1, src2) contributes one quad per direction both sources have a target in
        have = (self.trg_of >= 0).sum(axis=0)
        self.N = int((have.astype(np.int64) ** 2).sum())
        self._implied = None

    @property
    def implied(self):
        """implied[dir12][dir_ii] (0-based indices into lists of 1-based (src1, trg1, src2, trg2)), as the
        reference's `while` loop fills it: pair index, then the target i of src1, then the target j of src2"""
        if self._implied is None:
            nd = self.pairs_by_dir.ndirections()
            implied = [[[] for _ in range(self.K)] for _ in range(nd)]
            for d12, prs in enumerate(self.pairs_by_dir.pairs):
                cell = implied[d12]
                for src1, src2 in prs:
                    for dir1, trg1 in self.trg_from_src[src1 - 1]:
                        for dir2, trg2 in self.trg_from_src[src2 - 1]:
                            if dir1 == dir2:
                                cell[dir1 - 1].append((src1, trg1, src2, trg2))
            self._implied = implied
        return self._implied

    def __len__(self):
        return self.N

    def ndirections(self):
        return (self.pairs_by_dir.ndirections(), self.K)

    def __iter__(self):
        """(lin, src1, trg1, src2, trg2), lin the 1-based column-major linear index of (dir12, dir_ii)"""
        nd, implied = self.pairs_by_dir.ndirections(), self.implied
        for k in range(self.K):
            for d12 in range(nd):
                lin = 1 + d12 + nd * k
                for quad in implied[d12][k]:
                    yield (lin,) + quad
