"""Adversarial lattices for the three general clustering implementations behind vofod_cluster (launch_cluster, vofod_hip.hip):
voxel level (k_union<2> + k_flatten<0>), brick masks (k_brick_conn + k_brick_link_tr) and the fused brick union (k_brick_union<1>).
vofod_cluster takes lattice keys and a vofod_grid_desc directly, so every case here is drawn in numpy as integer cells, with no
voxeliser in front.  No GPU and no native library in this module (the ctypes structures and the statement are imported where a
function needs them): tests/test_cluster_lattice_cpu.py holds the cases to what they claim (and the oracle to scipy) on any machine,
tests/test_gpu_cluster_lattice.py runs them through the HIP library.

A case is (ijk, div_b, leaf[3], offset[3], tol) plus
  expect  what statements.euclidean_components must find: an int (number of components), "one", "singletons", or None where the
          float32 expression on the actual centres decides and nothing is known by construction (boundary pairs off the origin,
          random fills);
  family  the kernels the plan reaches with no switch set: "voxel" (tol / leaf <= 3 sqrt(3): a 4x4x4 brick is no clique),
          "masks" (at most 64 brick offsets in the half stencil) or "union" (more).  Which ratio lands where: a brick offset b
          belongs to the stencil when its nearest voxel pair, max(4|b| - 3, 0) cells apart per axis, is within the tolerance or on it.
          Ratios 5.2, 6 and 7 keep |b| <= 2 on one axis only (40 offsets), ratio 8 all of |b| <= 2 but the eight corners (58), ratio 9
          takes the corners and, on the boundary, (+-3, 0, 0) and its kin (65), ratios 15 and 30 hundreds.

Ratios are built from leaves and tolerances that are exact in float32 (0.5, 0.25; 1.25, 1.5, 1.75, 2.0, 2.25, 2.5) wherever a case claims
a structure by construction: centres at offset 0 and their differences are then exact, and so is `d2 < tol * tol`."""
import itertools
from dataclasses import dataclass, field

import numpy as np

F = np.float32


@dataclass(frozen=True)
class Case:
    name: str
    ijk: np.ndarray = field(repr=False, compare=False)
    div_b: tuple
    leaf: tuple
    offset: tuple
    tol: float
    expect: object  # int | "one" | "singletons" | None
    family: str     # "voxel" | "masks" | "union"
    label_rank: object = None  # interleaved serpentines: the labels the reference must hand out (ranks of the two smallest keys)

    def __post_init__(self):
        a = np.asarray(self.ijk, dtype=np.int64).reshape(-1, 3)
        assert len(a) and (a >= 0).all() and (a < np.array(self.div_b)).all(), self.name
        assert len(np.unique(a, axis=0)) == len(a), self.name  # no cell twice
        assert len(a) <= 8192, (self.name, len(a))


def lattice_inputs(case):
    """what cluster() takes: (points [n] POINT_XYZR, keys [n] uint32 strictly ascending, GridDesc, P [n, 3] float32 centres).
    key = i + j*dx + k*dx*dy; centre = (ijk + 0.5) * leaf + offset with every operation rounded to float32 in that order
    (include/vofod.h vofod_grid_desc, k_flatten); range = 1; min_b = 0."""
    from vofod_amd import capi

    dx, dy, dz = (int(v) for v in case.div_b)
    assert dx * dy * dz <= 0x7FFFFFFF
    a = np.asarray(case.ijk, dtype=np.int64).reshape(-1, 3)
    keys = a[:, 0] + a[:, 1] * dx + a[:, 2] * dx * dy
    order = np.argsort(keys, kind="stable")
    a, keys = a[order], keys[order]
    assert (np.diff(keys) > 0).all()
    leaf, off = np.array(case.leaf, dtype=F), np.array(case.offset, dtype=F)
    P = np.empty((len(a), 3), dtype=F)
    for c in range(3):
        P[:, c] = ((a[:, c].astype(F) + F(0.5)) * leaf[c]) + off[c]
    assert P.dtype == F
    pts = np.zeros(len(a), dtype=capi.POINT_XYZR)
    pts["x"], pts["y"], pts["z"], pts["range"] = P[:, 0], P[:, 1], P[:, 2], 1
    grid = capi.GridDesc()
    for c in range(3):
        grid.leaf[c], grid.offset[c], grid.min_b[c], grid.div_b[c] = float(leaf[c]), float(off[c]), 0, case.div_b[c]
    return pts, keys.astype(np.uint32), grid, P


_reference = {}


def reference(case):
    """(labels, number of components) of the plain statement for a case, computed once and shared by the tests: scipy's connected
    components over FLANN's float32 `d2 < tol * tol` (statements.euclidean_components), label = smallest member"""
    if case.name not in _reference:
        import statements

        _, _, _, P = lattice_inputs(case)
        comp, first, _, _ = statements.euclidean_components(P, F(case.tol))
        labels = first[comp].astype(np.uint32)
        labels.setflags(write=False)
        _reference[case.name] = (labels, int(comp.max()) + 1)
    return _reference[case.name]


def expected_components(case, n_components):
    """does the reference's count satisfy what the case claims?"""
    n = len(case.ijk)
    if case.expect is None:
        return 1 <= n_components <= n
    want = {"one": 1, "singletons": n}.get(case.expect, case.expect)
    return n_components == want


# ------------------------------------------------------------------------------------------------------------------ ratios
# (leaf, tol, largest gap in cells that still links along an axis, family)
R2_5 = (0.5, 1.25, 2, "voxel")
R6 = (0.25, 1.5, 5, "masks")
R8 = (0.25, 2.0, 7, "masks")
R9 = (0.25, 2.25, 8, "union")
R15 = (0.1, 1.5, 14, "union")


def _fit(cells, pad=(0, 0, 0)):
    """(cells, div_b): the smallest lattice holding the cells, plus `pad` empty cells on the far faces"""
    a = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    return a, tuple(int(a[:, c].max()) + 1 + pad[c] for c in range(3))


def _case(name, cells, ratio, expect, div_b=None, offset=(0.0, 0.0, 0.0), tol=None, family=None, leaf=None, **kw):
    a, fit = _fit(cells)
    lf = leaf if leaf is not None else (ratio[0],) * 3
    return Case(name, a, tuple(div_b or fit), tuple(lf), tuple(offset), ratio[1] if tol is None else tol, expect, family or ratio[3], **kw)


# -------------------------------------------------------------------------------------------------------- 1, 2 serpentines
def _run(a, b, g):
    """integers strictly between a and b, stepping at most g from a towards b (the far end then within g of b)"""
    out, s = [], 1 if b > a else -1
    x = a
    while abs(b - x) > g:
        x += s * g
        out.append(x)
    return out


def _layer_path(g, nx, ny):
    """one layer of a serpentine as an ordered path of (x, y): rows g + 1 apart (the smallest distance that does not link), cells g
    apart (the largest that does), one turn-around cell between consecutive rows at alternating ends.  ny even: the path starts at
    (0, 0) and ends at (0, last row)."""
    s, L, path = g + 1, g * (nx - 1), []
    for r in range(ny):
        xs = [g * t for t in range(nx)]
        if r % 2:
            xs.reverse()
        path += [(x, s * r) for x in xs]
        if r + 1 < ny:
            path += [(L if r % 2 == 0 else 0, y) for y in _run(s * r, s * (r + 1), g)]
    return path, L


def _serpentine(g, nx, ny, zs, mirror=False, x0=0):
    """a chain through the layers `zs` (each 2D path walked forth and back alternately, vertical runs at the joints); mirror: x
    reflected, so both ends of every layer's path lie at the right edge"""
    path, L = _layer_path(g, nx, ny)
    if mirror:
        path = [(L - x, y) for x, y in path]
    cells = []
    for n, z in enumerate(zs):
        p = path if n % 2 == 0 else path[::-1]
        cells += [(x + x0, y, z) for x, y in p]
        if n + 1 < len(zs):
            ex, ey = p[-1]
            cells += [(ex + x0, ey, zz) for zz in _run(z, zs[n + 1], g)]
    return cells, L


def _serpentine_cases():
    out = []
    for tag, ratio, nx, ny, nl in (("r2.5", R2_5, 32, 10, 5), ("r6", R6, 13, 6, 3)):
        g = ratio[2]
        zs = [(g + 1) * n for n in range(nl)]
        cells, _ = _serpentine(g, nx, ny, zs)
        out.append(_case(f"serpentine_{tag}", cells, ratio, "one"))
        # without the voxel of the smallest key (the chain's first cell): the label starts one link further in
        a, _ = _fit(cells)
        first = np.lexsort((a[:, 0], a[:, 1], a[:, 2]))[0]
        out.append(_case(f"serpentine_{tag}_without_first", np.delete(a, first, axis=0), ratio, "one"))
        # z reflected: the smallest key is the first cell of the LAST layer, (nl - 1) / nl along the chain - the label travels both ways
        zmax = max(c[2] for c in cells)
        out.append(_case(f"serpentine_{tag}_label_inside", [(x, y, zmax - z) for x, y, z in cells], ratio, "one"))
    return out


def _interleaved(ratio, nx, ny):
    """two serpentines that never come within the tolerance of each other.  s = g + 1 cells do not link.  B lies in the layers z = s, 3s
    with its joints in the column x = 0 and a tail down to (0, 0, 0); A lies in the layers z = 0, 2s, shifted s cells in x, mirrored, with
    its joints at its right edge - s cells past B's footprint.  So layers of A and B are s apart in z, every joint and the tail s apart
    in x from the other chain.  The two smallest keys are B's tail cell (0, 0, 0) and A's (s, 0, 0)."""
    g = ratio[2]
    s = g + 1
    assert ny % 2 == 0
    b, L = _serpentine(g, nx, ny, [s, 3 * s])
    b += [(0, 0, 0)] + [(0, 0, z) for z in _run(0, s, g)]
    a, _ = _serpentine(g, nx, ny, [0, 2 * s], mirror=True, x0=s)
    return a + b


def _interleaved_cases():
    return [
        _case("interleaved_r2.5", _interleaved(R2_5, 16, 6), R2_5, 2, label_rank=(0, 1)),
        _case("interleaved_r6", _interleaved(R6, 9, 4), R6, 2, label_rank=(0, 1)),
    ]


# ------------------------------------------------------------------------------------------------------- 3 on the boundary
def _half_space(v):
    """the sign / permutation images of an offset in the forward half space (dz > 0, or dz == 0 and dy > 0, or dy == dz == 0 and dx > 0)"""
    out = set()
    for p in set(itertools.permutations(v)):
        for sg in itertools.product((1, -1), repeat=3):
            o = tuple(a * b for a, b in zip(p, sg))
            if (o[2], o[1], o[0]) > (0, 0, 0):
                out.add(o)
    return sorted(out)


def _pairs_on_grid(offsets, reach, per_row=5):
    """one pair (anchor, anchor + o) per offset, anchors on a square grid so far apart that voxels of different pairs are more than
    `reach` cells from each other"""
    pitch = 3 * reach + 2
    cells = []
    for n, o in enumerate(offsets):
        ax, ay = pitch * (n % per_row) + reach, pitch * (n // per_row) + reach
        cells += [(ax, ay, 0), (ax + o[0], ay + o[1], o[2])]
    return cells


def _shorter(o):
    """the offset one cell shorter along its longest axis: inside the tolerance when `o` is on it"""
    c = int(np.argmax(np.abs(o)))
    return tuple(v - (np.sign(v) if k == c else 0) for k, v in enumerate(o))


BOUNDARY = (
    # (tag, leaf, tol, cells per tolerance m, integer vectors of length exactly m, family)
    ("r3", 0.5, 1.5, 3, [(3, 0, 0)], "voxel"),
    ("r5", 0.5, 2.5, 5, [(5, 0, 0), (3, 4, 0)], "voxel"),
    ("r7", 0.25, 1.75, 7, [(7, 0, 0), (2, 3, 6)], "masks"),
    ("r8", 0.25, 2.0, 8, [(8, 0, 0)], "masks"),
    ("r9", 0.25, 2.25, 9, [(9, 0, 0), (1, 4, 8)], "union"),
    ("r30", 0.1, 3.0, 30, [(30, 0, 0), (18, 24, 0)], "union"),
    # a leaf that is no float at the two lower families as well (a leaf of 0.5 or 0.25 is a whole number of ulps at any offset: the
    # centres move, their differences stay exact)
    ("r5_leaf0.1", 0.1, 0.5, 5, [(5, 0, 0), (3, 4, 0)], "voxel"),
    ("r7_leaf0.1", 0.1, 0.7, 7, [(7, 0, 0), (2, 3, 6)], "masks"),
)
FAR_OFFSETS = (("at90", (90.37, -90.11, 90.73)), ("at1000", (-1000.7, 1000.3, 1000.9)), ("at8000", (8000.1, 8000.7, -8000.3)))


def _boundary_cases():
    out = []
    for tag, leaf, tol, m, vecs, family in BOUNDARY:
        on = [o for v in vecs for o in _half_space(v)]
        offs = on + [_shorter(o) for o in on]  # a pair exactly on the tolerance and, as the control, one a cell inside it
        cells = _pairs_on_grid(offs, m)
        a, fit = _fit(cells, pad=(1, 2, 3))
        exact = leaf in (0.5, 0.25)  # 0.1 is no float: the centres are inexact at the origin already, scipy decides
        for otag, off in (("origin", (0.0, 0.0, 0.0)),) + FAR_OFFSETS:
            expect = 2 * len(on) + len(on) if (otag == "origin" and exact) else None
            out.append(Case(f"boundary_{tag}_{otag}", a, fit, (leaf,) * 3, off, tol, expect, family))
    return out


# --------------------------------------------------------------------------------------------------------- 4 word boundaries
def _word_boundary_cases():
    """ratio 6: the row (dj, dk) = (1, 0) reaches 5 cells in x (sqrt(25 + 1) < 6 <= sqrt(36 + 1)), so the window of voxel (i, j, k) over the
    next row starts at cell i - 5: L = (k*dy + j + 1)*dx + i - 5.  One group per start bit 63, 0 and 1: the voxel with one partner in the
    window's first cell and one in its last (bit L + 10: the next word for the starts 63 ... 54), linked through it alone.  A last
    group has its partner in the lattice's very last cell.  Groups lie 8 layers apart.  (dx = 64: rows are words, no window can start
    at bit 63 or straddle; the third group's window ends in the word's last bit instead.)"""
    out = []
    rx, dy = 5, 5
    for dx in (61, 64, 67, 127):
        cells, k = [], 0
        for sh in (63, 0, 1) if dx != 64 else (53, 0, 1):
            hits = [(i, j, kk) for kk in range(k, k + 64) for j in range(dy - 1) for i in range(rx, dx - rx) if ((kk * dy + j + 1) * dx + i - rx) % 64 == sh]
            i, j, k = hits[0]
            cells += [(i, j, k), (i - rx, j + 1, k), (i + rx, j + 1, k)]
            k += 8
        dz = k + 1
        cells += [(dx - 1 - rx, dy - 2, dz - 1), (dx - 1, dy - 1, dz - 1)]
        out.append(_case(f"words_dx{dx}", cells, R6, 4, div_b=(dx, dy, dz)))
    return out


# ----------------------------------------------------------------------------------------------- 5 faces, degenerate lattices
def _shell(dx, dy, dz):
    g = np.stack(np.meshgrid(np.arange(dx), np.arange(dy), np.arange(dz), indexing="ij"), axis=-1).reshape(-1, 3)
    on = ((g == 0) | (g == np.array([dx - 1, dy - 1, dz - 1]))).any(axis=1)
    return g[on]


def _corners_and_face_centres(dx, dy, dz):
    c = [(x, y, z) for x in (0, dx - 1) for y in (0, dy - 1) for z in (0, dz - 1)]
    mx, my, mz = dx // 2, dy // 2, dz // 2
    return c + [(0, my, mz), (dx - 1, my, mz), (mx, 0, mz), (mx, dy - 1, mz), (mx, my, 0), (mx, my, dz - 1)]


def _line(g, n_gaps):
    """positions along a line: gaps of g cells (link) and g + 1 (do not) in a fixed pattern; (positions, components)"""
    pos, comps = [0], 1
    for n in range(n_gaps):
        wide = n % 4 == 2
        pos.append(pos[-1] + g + (1 if wide else 0))
        comps += wide
    return pos, comps


def _face_cases():
    out = []
    for tag, ratio in (("r2.5", R2_5), ("r6", R6)):
        # 15 x 11 x 9: no extent a multiple of 4 (partial last bricks).  Every cell of the six faces: one component.  The eight
        # corners and six face centres: more than 6 cells from each other, all singletons at both ratios.
        out.append(_case(f"shell_{tag}", _shell(15, 11, 9), ratio, "one", div_b=(15, 11, 9)))
        out.append(_case(f"corners_{tag}", _corners_and_face_centres(15, 11, 9), ratio, "singletons", div_b=(15, 11, 9)))
        pos, comps = _line(ratio[2], 22)
        for axis, name in enumerate(("x", "y", "z")):
            cells = np.zeros((len(pos), 3), dtype=np.int64)
            cells[:, axis] = pos
            div = [1, 1, 1]
            div[axis] = pos[-1] + 1
            out.append(_case(f"line_{name}_{tag}", cells, ratio, comps, div_b=tuple(div)))
        out.append(_case(f"single_cell_{tag}", [(0, 0, 0)], ratio, "one", div_b=(1, 1, 1)))
    return out


# ----------------------------------------------------------------------------------------------------------- 6 dense block
def _box(dx, dy, dz):
    return np.stack(np.meshgrid(np.arange(dx), np.arange(dy), np.arange(dz), indexing="ij"), axis=-1).reshape(-1, 3)


def _dense_cases():
    out = [_case(f"dense_{tag}", _box(11, 10, 9), ratio, "one") for tag, ratio in (("r2.5", R2_5), ("r6", R6), ("r15", R15))]
    b = _box(11, 10, 9)
    checker = b[b.sum(axis=1) % 2 == 0]
    # nearest neighbours of the checkerboard: sqrt(2) * 0.5 m, d2 = 0.5 exactly; 0.7071f^2 < 0.5 < 0.7072f^2
    assert F(0.7071) * F(0.7071) < F(0.5) < F(0.7072) * F(0.7072)
    out.append(_case("checker_below", checker, (0.5, 0.7071, 1, "voxel"), "singletons", div_b=(11, 10, 9)))
    out.append(_case("checker_above", checker, (0.5, 0.7072, 1, "voxel"), "one", div_b=(11, 10, 9)))
    return out


# ------------------------------------------------------------------------------------------------------ 7 brick-corner links
HALF_DIRS = [d for d in itertools.product((-1, 0, 1), repeat=3) if (d[2], d[1], d[0]) > (0, 0, 0)]  # (dx, dy, dz): the 13 forward directions


def _longest_link(d, m):
    """the longest offset along direction d (per-axis steps in cells, equal at first, then the first axis stretched) that is still
    shorter than m cells, and the one a cell longer on that axis, which is not"""
    nz = [c for c in range(3) if d[c]]
    a = 1
    while (a + 1) ** 2 * len(nz) < m * m:
        a += 1
    v = [a * abs(d[c]) for c in range(3)]
    while sum(x * x for x in v) + 2 * v[nz[0]] + 1 < m * m:
        v[nz[0]] += 1
    beyond = list(v)
    beyond[nz[0]] += 1
    assert sum(x * x for x in v) < m * m <= sum(x * x for x in beyond)
    return tuple(x * s for x, s in zip(v, d)), tuple(x * s for x, s in zip(beyond, d))


def _brick_corner_cells(offsets):
    """per (direction, offset): a voxel in the corner of its brick that faces the direction (local 3 where d > 0, 0 where d < 0, 1 on the
    axes the direction does not move along) and its partner `offset` away - in the brick next door for |offset| <= 4, two bricks
    away for 5 ... 8.  Pairs sit in regions of 32 cells, more than 9 cells from each other."""
    cells = []
    for n, (d, o) in enumerate(offsets):
        base = (32 * (n % 6) + 12, 32 * (n // 6) + 12, 12)
        a = tuple(base[c] + (3 if d[c] > 0 else 0 if d[c] < 0 else 1) for c in range(3))
        cells += [a, tuple(a[c] + o[c] for c in range(3))]
    return cells


def _brick_corner_cases():
    out = []
    for tag, ratio, m in (("r8", R8, 8), ("r9", R9, 9)):
        reach1 = [(d, d) for d in HALF_DIRS]  # facing corners of neighbouring bricks: one cell apart on every moving axis
        reach2 = [(d, _longest_link(d, m)[0]) for d in HALF_DIRS]
        beyond = [(d, _longest_link(d, m)[1]) for d in HALF_DIRS]
        assert all(max(abs(x) for x in o) >= 5 for _, o in reach2)  # two bricks apart on the stretched axis
        cells = _brick_corner_cells(reach1 + reach2)
        out.append(_case(f"brick_corners_{tag}_link", cells, ratio, 26, div_b=_fit(cells, pad=(1, 2, 3))[1]))
        cells = _brick_corner_cells(beyond)
        out.append(_case(f"brick_corners_{tag}_beyond", cells, ratio, "singletons", div_b=_fit(cells, pad=(1, 2, 3))[1]))
    return out


# ---------------------------------------------------------------------------------------------------- 8 the clique threshold
def _clique_cases():
    """the same lattice at tolerance 1.29 and 1.30 over leaf 0.25: ratio 5.16 and 5.2, either side of 3 sqrt(3) = 5.196.  Four pairs
    (+-3, +-3, 3) apart - the diagonal of a brick, 1.299 m - and a full 4x4x4 brick: the pairs are apart below the threshold and
    joined above it, the brick is one component both times (below through its inner cells)."""
    offs = [(3, 3, 3), (-3, 3, 3), (3, -3, 3), (-3, -3, 3)]
    cells = _pairs_on_grid(offs, 6, per_row=2)
    top = max(c[1] for c in cells) + 12
    cells += [(x, top + y, z) for x in range(4) for y in range(4) for z in range(4)]
    a, fit = _fit(cells, pad=(2, 1, 3))
    return [
        Case("clique_below", a, fit, (0.25,) * 3, (0.0,) * 3, 1.29, 9, "voxel"),
        Case("clique_above", a, fit, (0.25,) * 3, (0.0,) * 3, 1.30, 5, "masks"),
    ]


def _clique_ambiguous_case():
    """8 km from the origin a centre is only known to a millimetre and the class of the brick diagonal (3, 3, 3) turns ambiguous for
    tolerances around 1.3 m: D = 1.6875, the classifier's margin there is about 0.009.  Tolerance 1.299 (r2 = 1.6874) lies inside it,
    and the float expression - a leaf of 0.25 is a whole number of ulps, the differences stay exact - says NOT within.  A brick is no
    certain clique, so the voxel level has to run, and two voxels in opposite corners of one brick stay apart."""
    cells = [(4, 4, 4), (7, 7, 7), (7, 4, 12), (4, 7, 15)]
    return [Case("clique_ambiguous_at8000", np.array(cells), (13, 11, 18), (0.25,) * 3, (8000.1, 8000.7, -8000.3), 1.299, "singletons", "voxel")]


def _quantised_cases():
    """the nominal class is sure, the real float32 centres disagree: leaf 0.1 at 8 km, where a centre is a multiple of q = 2^-11 m
    (0.49 mm).  Pairs 4, 7 and 16 cells apart along an axis are nominally 819.2, 1433.6 and 3276.8 q apart, in float32 the whole number
    below or above: 0.39990 / 0.40039, 0.69971 / 0.70020, 1.59961 / 1.60010 m.  A tolerance between the lower value and the nominal distance
    links the pairs that rounded down though the nominal distance is beyond it; one between the nominal distance and the upper value
    leaves the pairs that rounded up apart though the nominal distance is within it.  Either tolerance is 5e-5 m or more from the
    nominal distance, a hundred times the classifier's margin without the centres' own error (its `delta`): only a classifier that
    counts the centres' rounding leaves these pairs to the float expression.  24 pairs at different cells, so both roundings
    occur; scipy's float32 evaluation decides, test_cluster_lattice_cpu.py requires that it links some pairs and not others."""
    out = []
    for tag, m, family, below, above in (("r4", 4, "voxel", 0.39995, 0.4002), ("r7", 7, "masks", 0.6999, 0.7001), ("r16", 16, "union", 1.5998, 1.60005)):
        cells = _pairs_on_grid([(m, 0, 0), (0, m, 0), (0, 0, m)] * 8, m + 1)  # (anchors 3 m + 5 cells apart: no whole number of q)
        a, fit = _fit(cells, pad=(3, 2, 1))
        for side, tol in (("below", below), ("above", above)):
            out.append(Case(f"quantised_{tag}_{side}", a, fit, (0.1,) * 3, (8000.1, 8000.7, -8000.3), tol, None, family))
    return out


# ------------------------------------------------------------------------------------ the in-row shortcuts of the voxel level
def _row_reach(dj, dk, m):
    """largest |di| with di^2 + dj^2 + dk^2 < m^2, or -1"""
    r = -1
    while (r + 1) ** 2 + dj * dj + dk * dk < m * m:
        r += 1
    return r


def _shortcut_cases():
    """k_union skips cells that a voxel's left neighbour in its own row has already examined, and cells within the sure in-row gap g of
    a neighbour it has just linked.  Both are right only up to one exact cell.  Per row (dj, dk) of the half stencil with reach r:
      - u, v = u + d in one row (d = 1 and d = g) and w in the row (dj, dk) at u + r + 1: one cell past what u reached, linked to v alone;
      - v with w1 = v - r and w2 = w1 + g + 1 in the row (dj, dk): both linked to v, one cell too far apart to link each other.
    Every group is one component, more than the tolerance from the next."""
    out = []
    for tag, ratio, m in (("r2.5", R2_5, 2.5), ("r6", R6, 6)):
        g = ratio[2]
        R = int(np.ceil(m))
        groups = []
        for dk in range(0, R + 1):
            for dj in range(-R if dk else 1, R + 1):
                r = _row_reach(dj, dk, m)
                if r < 1:
                    continue
                for d in sorted(d for d in {1, g} if d <= 2 * r + 1):  # (w within r of v on either side)
                    groups.append([(0, 0, 0), (d, 0, 0), (r + 1, dj, dk)])
                if g + 1 <= 2 * r:
                    groups.append([(0, 0, 0), (-r, dj, dk), (-r + g + 1, dj, dk)])
        pitch, per_row, cells = 3 * R + 2, 12, []
        for n, grp in enumerate(groups):
            ax, ay = pitch * (n % per_row) + R, pitch * (n // per_row) + R
            cells += [(ax + x, ay + y, z) for x, y, z in grp]
        out.append(_case(f"row_shortcuts_{tag}", cells, ratio, len(groups), div_b=_fit(cells, pad=(2, 1, 1))[1]))
    return out


# -------------------------------------------------------------------------------------------------------- 9 the window limit
WINDOW_LIMIT = dict(leaf=0.1, tol=3.0, refused_tol=3.05)  # R = ceil(tol / leaf) + 1 = 31 = MAX_R; 3.05 gives 32


def _window_cases():
    """leaf 0.1, tolerance 3.0: the 63-bit window.  Offsets at least 0.15 cells inside or 0.03 cells outside 30 cells (1.5 cm, 3 mm:
    float rounding of centres a few metres from the origin is below a micrometre), so the structure holds by construction: 29 cells
    along x with the pair in two different bitmap words, and the longest diagonals with the next lattice point outside.  The pair
    exactly 30 cells apart is a case of its own: 0.1 is no float, scipy's float32 expression decides."""
    inside = [(29, 0, 0), (21, 21, 0), (-21, 21, 0), (0, 21, 21), (21, 0, 21), (17, 17, 17), (-17, 17, 17), (17, -17, 17), (-17, -17, 17), (29, 7, 0), (7, 29, 0),
              (0, -7, 29), (-29, 7, 0)]
    outside = [(21, 22, 0), (-22, 21, 0), (0, 22, 21), (17, 17, 18), (-17, 18, 17), (29, 8, 0), (8, 29, 0), (0, -8, 29), (-29, 8, 0)]
    assert all(29.85 ** 2 > sum(x * x for x in o) for o in inside) and all(30.03 ** 2 < sum(x * x for x in o) for o in outside)
    cells = _pairs_on_grid(inside + outside, 30)
    def straddles(pad):
        """with `pad` empty cells past the last pair, is dx no multiple of 4 and does the 29-cell pair (the first one) lie in two words?"""
        a, fit = _fit(cells, pad=(pad, 1, 2))
        k0, k1 = (int(a[n, 0] + a[n, 1] * fit[0] + a[n, 2] * fit[0] * fit[1]) for n in (0, 1))
        return k1 - k0 == 29 and k0 // 64 != k1 // 64 and fit[0] % 4 != 0

    pad = next(p for p in range(1, 64) if straddles(p))  # (StopIteration: no row length in reach does it)
    a, fit = _fit(cells, pad=(pad, 1, 2))
    lf = (WINDOW_LIMIT["leaf"],) * 3
    out = [Case("window_limit", a, fit, lf, (0.0,) * 3, WINDOW_LIMIT["tol"], len(inside) + 2 * len(outside), "union")]
    # rows 34 cells apart: 30 cells across the first word boundary of a row, 29 across it, 30 further along
    cells = [(40, 0, 0), (70, 0, 0), (40, 34, 0), (69, 34, 0), (10, 68, 0), (40, 68, 0)]
    out.append(Case("window_limit_30_cells", np.array(cells), (97, 69, 1), lf, (0.0,) * 3, WINDOW_LIMIT["tol"], None, "union"))
    return out


# ------------------------------------------------------------------------------------------------------ 10 anisotropic leaf
def _anisotropic_cases():
    """leaf (0.5, 0.25, 1.0), tolerance 1.3: 2 cells link along x (1.0 m) and 3 do not (1.5), 5 / 6 along y (1.25 / 1.5), 1 / 2 along z.
    Axis pairs at those gaps with a known count, and a 30 % random fill for everything in between."""
    leaf, tol = (0.5, 0.25, 1.0), 1.3
    offs = [(2, 0, 0), (0, 5, 0), (0, 0, 1), (3, 0, 0), (0, 6, 0), (0, 0, 2)]
    cells = _pairs_on_grid(offs, 6, per_row=3)
    a, fit = _fit(cells, pad=(1, 1, 1))
    rng = np.random.default_rng(1010)
    b = _box(13, 22, 7)
    return [
        Case("anisotropic_axes", a, fit, leaf, (0.0,) * 3, tol, 3 + 6, "voxel"),
        Case("anisotropic_fill", b[rng.random(len(b)) < 0.3], (13, 22, 7), leaf, (0.0,) * 3, tol, None, "voxel"),
    ]


# ------------------------------------------------------------------------------------------------------------ 11 random fill
def _random_cases():
    """boxes filled to 2 %, 30 % and 90 % at ratios 1.4, 3, 6 and 15: the box shrinks with the ratio and the fill so that the
    statement's pair list stays around a million entries (a voxel has ~ 4/3 pi ratio^3 * fill neighbours)"""
    ratios = (("r1.4", (0.5, 0.7, 1, "voxel")), ("r3", (0.5, 1.5, 2, "voxel")), ("r6", R6), ("r15", R15))
    boxes = {  # (ratio, fill %) -> box
        ("r1.4", 2): (61, 37, 29), ("r1.4", 30): (31, 23, 18), ("r1.4", 90): (23, 19, 14),
        ("r3", 2): (61, 37, 29), ("r3", 30): (31, 23, 18), ("r3", 90): (23, 19, 14),
        ("r6", 2): (61, 37, 29), ("r6", 30): (27, 21, 14), ("r6", 90): (19, 14, 11),
        ("r15", 2): (67, 45, 38), ("r15", 30): (23, 18, 13), ("r15", 90): (15, 13, 10),
    }
    out = []
    for n, ((tag, ratio), fill) in enumerate(itertools.product(ratios, (2, 30, 90))):
        box = boxes[(tag, fill)]
        b = _box(*box)
        rng = np.random.default_rng(1100 + n)
        out.append(_case(f"fill{fill}_{tag}", b[rng.random(len(b)) < fill / 100.0], ratio, None, div_b=box, offset=(-7.3, 2.1, 0.4)))
    # the brick families percolate at 2 %: fills thin enough for hundreds of components (a voxel has about one neighbour)
    for tag, ratio, box, fill in (("r6", R6, (101, 83, 61), 0.002), ("r15", R15, (211, 163, 127), 0.00015)):
        n_cells = box[0] * box[1] * box[2]
        keys = np.flatnonzero(np.random.default_rng(1150).random(n_cells) < fill)
        cells = np.stack([keys % box[0], keys // box[0] % box[1], keys // (box[0] * box[1])], axis=1)
        out.append(_case(f"fill_thin_{tag}", cells, ratio, None, div_b=box, offset=(-7.3, 2.1, 0.4)))
    return out


def _all_cases():
    out = []
    for make in (_serpentine_cases, _interleaved_cases, _boundary_cases, _word_boundary_cases, _face_cases, _dense_cases, _brick_corner_cases, _clique_cases,
                 _clique_ambiguous_case, _quantised_cases, _shortcut_cases, _window_cases, _anisotropic_cases, _random_cases):
        out += make()
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _all_cases()
BY_NAME = {c.name: c for c in CASES}
# three (leaf, tolerance) pairs, one per family, for the sequences on one handle that caches the tables of two: CACHE_SEQUENCE indexes them -
# A, B, A (a hit), C (evicts B's slot), A (still cached: its neighbour was rebuilt), B (evicts), then round and round, every call a rebuild
ALTERNATING = ("interleaved_r2.5", "brick_corners_r8_link", "brick_corners_r9_link")
CACHE_SEQUENCE = (0, 1, 0, 2, 0, 1, 2, 0, 1, 2)
