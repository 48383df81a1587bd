"""Hand-placed scenes for tests/test_gpu_tail_edges.py: lattice clusters above an apriori background sheet, built so that a
frame meets exactly one capacity or gate of the device classification tail (kernels_tail.h).  Everything here is host
arithmetic on map cells; the numbers a scene claims (candidate clusters, candidate members, detections) follow from the placed
geometry alone and are checked against the oracle's debug view by the tests."""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field

import numpy as np

VS = 0.25
SENSOR_CELL = np.array([350.5, 200.0, 20.5])  # sensor position in cell units (cell i spans [i, i + 1)): x, z on a cell centre, y on a cell boundary
SHEET_LAYER = 8
GAP = 11  # cells between the members of different clusters (tolerance 1.5 m / 0.25 m = 6 cells: none join)


@dataclass
class Shape:
    name: str
    cells: np.ndarray        # [n, 3] map cells
    kind: str                # "sym": position = centroid of the cells; "skew": position inside the AABB; "none": no position statement
    det: object              # True / False: a detection or not, from the placed geometry alone; None: the oracle decides
    cand: bool               # a candidate cluster (far, >= min_points voxels, lattice extents within the prefilter)


@dataclass
class Scene:
    frames: list             # four lists of Shape; frame 0 is the frame at the edge
    dyn: dict = field(default_factory=dict)          # dynamic parameters that differ from the defaults
    unknown: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), dtype=np.int64))  # map cells written to scores/unknown
    trips: object = None     # which capacity frame 0 exceeds: None, "clusters", "members", "dets", "radius"; "open": not asserted
    R: object = None         # Manhattan radius of the 2-voxel clusters' fills, where the case is about it
    scan_frames: tuple = (0, 1)  # the frames that also run as single map-updating scans


# ------------------------------------------------------------------------------------------------------------------ shapes
def _norm(cells):
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    return c - c.min(0)


def line(n, axis):
    c = np.zeros((n, 3), dtype=np.int64)
    c[:, axis] = np.arange(n)
    return c


def diag_line(n, d):
    return _norm(np.arange(n)[:, None] * np.asarray(d, dtype=np.int64)[None, :])


def block(a, b, c):
    return np.array(list(itertools.product(range(a), range(b), range(c))), dtype=np.int64)


PAIRS = {"pair x": line(2, 0), "pair y": line(2, 1), "pair z": line(2, 2), "pair xy": diag_line(2, (1, 1, 0)), "pair x-y": diag_line(2, (1, -1, 0)),
         "pair yz": diag_line(2, (0, 1, 1)), "pair xyz": diag_line(2, (1, 1, 1))}
FLAT_PAIRS = ["pair x", "pair y", "pair z", "pair xy", "pair x-y", "pair yz"]  # OBB diagonal <= 0.354 m
ALIGNED = {
    "2 points along x": [(0, 0, 0), (1, 0, 0)],
    "3 collinear": [(0, 0, 0), (1, 0, 0), (2, 0, 0)],
    "2x2 square": [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)],
    "2x2 square xz": [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1)],
    "2x2x2 cube": list(itertools.product((0, 1), repeat=3)),
    "3x3 square": [(i, j, 0) for i in range(3) for j in range(3)],
    "plus": [(1, 0, 0), (0, 1, 0), (1, 1, 0), (2, 1, 0), (1, 2, 0)],
}
DIAGONALS = {"diagonal pair xy": [(0, 0, 0), (1, 1, 0)], "diagonal pair xyz": [(0, 0, 0), (1, 1, 1)], "diagonal triple xy": [(0, 0, 0), (1, 1, 0), (2, 2, 0)]}
TETRAHEDRA = {f"tetrahedron {s}": _norm([(0, 0, 0), (s[0], 0, 0), (0, s[1], 0), (0, 0, s[2])]) for s in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1))}
L_TRIPLE = _norm([(0, 0, 0), (1, 0, 0), (0, 1, 0)])


def random_subblocks(n, seed=9):
    """subsets of a 3 x 3 x 3 block as test_obb_gates_on_degenerate_lattice_clusters draws them (at least two cells)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        cells = np.unique(rng.integers(0, 3, size=(int(rng.integers(2, 10)), 3)), axis=0)
        if len(cells) >= 2:
            out.append(_norm(cells))
    return out


# --------------------------------------------------------------------------------------------------------------- placement
def dist_m(cells):
    """distance of the cells' centroid from the sensor, metres"""
    return float(np.linalg.norm((np.asarray(cells, dtype=np.float64) + 0.5).mean(0) - SENSOR_CELL) * VS)


class Placer:
    """deals lattice positions of one frame: bases on a grid of `pitch` cells, nearest to the sensor first; a shape is put on
    the first base where it keeps GAP cells from everything placed or reserved before and its centroid lies in [dmin, dmax] m"""

    def __init__(self, pitch=20, x=(250, 450), y=(60, 340), z=(30, 84), skip=0, reserved=(), keepout=()):
        b = np.array(list(itertools.product(range(x[0], x[1] + 1, pitch), range(y[0], y[1] + 1, pitch), range(z[0], z[1] + 1, pitch))), dtype=np.int64)
        order = np.argsort(np.linalg.norm(b + 0.5 - SENSOR_CELL, axis=1), kind="stable")
        self.bases = [tuple(v) for v in b[order]]
        self.bases = self.bases[skip:] + self.bases[:skip]
        self.placed = [np.asarray(r, dtype=np.int64).reshape(-1, 3) for r in reserved if len(r)]
        self.keepout = list(keepout)  # (centre cell, radius in cells): pockets of unknown voxels
        self.lim = (x, y, z)

    def fits(self, cells):
        if cells.min() < 12 or (cells.max(0) > np.array([468, 388, 95])).any() or cells[:, 2].min() < SHEET_LAYER + 20:
            return False
        for c, r in self.keepout:
            if np.linalg.norm(cells - np.asarray(c), axis=1).min() < r + GAP:
                return False
        for p in self.placed:
            d = cells[:, None, :] - p[None, :, :]
            if (d * d).sum(-1).min() < GAP * GAP:
                return False
        return True

    def put(self, cells):
        cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
        assert self.fits(cells), cells
        self.placed.append(cells)
        return cells

    def take(self, rel, dmin=3.0, dmax=45.0):
        rel = np.asarray(rel, dtype=np.int64).reshape(-1, 3)
        for i, b in enumerate(self.bases):
            cells = rel + np.asarray(b)
            if dmin <= dist_m(cells) <= dmax and self.fits(cells):
                del self.bases[i]
                self.placed.append(cells)
                return cells
        raise AssertionError("no room left for a shape")


def diamond(c, r):
    """the cells within Manhattan distance r of cell c"""
    g = np.arange(-r, r + 1)
    d = np.array(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1).T
    return d[np.abs(d).sum(1) <= r] + np.asarray(c, dtype=np.int64)


def ordinary_frame(k, names=("pair x", "2x2x2 cube", "plus", "pair xyz", "2x2 square", "3 collinear"), dmax=45.0, **placer):
    """an everyday frame: 3 + k floating symmetric shapes, placed differently from frame to frame"""
    pl = Placer(skip=9 * (k + 1), **placer)
    shapes = {**PAIRS, **{n: _norm(c) for n, c in ALIGNED.items()}}
    return [Shape(n, pl.take(shapes[n], dmax=dmax), "sym", True, True) for n in (names * 2)[: 3 + k]]


def _with_ordinary(frame0, dmax=45.0, **kw):
    return [frame0] + [ordinary_frame(k, dmax=dmax, **kw) for k in (0, 1, 2)]


# ------------------------------------------------------------------------------------------------------------------- cases
def scene_candidate_clusters(n):
    """case 1: n candidate clusters in frame 0 - 8 floating 2-voxel clusters, 30 diagonal lines of 8 / 9 / 10 voxels along (1, 1, 1)
    or (1, -1, 1) (every AABB extent <= 2.25 m, length 1.75 * sqrt(3) = 3.03 m or more: past the prefilter, over max_size) and n - 38
    lines of 2 / 3 / 4 voxels beyond classification__max_distance (lowered to 20 m).  Sizes repeat: the canonical order has ties."""
    dmax_gate = 20.0
    pl = Placer()
    f = []
    for i, name in enumerate(list(PAIRS)[:7] + ["pair x"]):
        f.append(Shape(name, pl.take(PAIRS[name], dmax=dmax_gate - 1.5), "sym", True, True))
    for i in range(30):
        f.append(Shape(f"diagonal line {8 + i % 3}", pl.take(diag_line(8 + i % 3, (1, 1, 1) if i % 2 else (1, -1, 1)), dmax=dmax_gate - 1.5), "none", False, True))
    for i in range(n - 38):
        f.append(Shape(f"distant line {2 + i % 3}", pl.take(line(2 + i % 3, i % 2), dmin=dmax_gate + 1.5), "none", False, True))
    return Scene(_with_ordinary(f, dmax=dmax_gate - 1.5), dyn=dict(classification__max_distance=dmax_gate), trips="clusters" if n > 64 else None)


def scene_candidate_members(n):
    """case 2: n candidate members in 16 candidate clusters of frame 0 - fifteen 4 x 4 x 4 blocks (seven of them within
    classification__max_distance = 20 m, eight beyond it: candidates all the same) and a remainder of n - 960 voxels (a block less
    a corner, a block, a block with one voxel more), within reach: 8 detections"""
    dmax_gate = 20.0
    pl = Placer()
    b = block(4, 4, 4)
    rem = {63: b[1:], 64: b, 65: np.vstack([b, [[4, 0, 0]]])}[n - 960]
    f = [Shape(f"remainder {len(rem)}", pl.take(rem, dmax=dmax_gate - 1.5), "sym" if len(rem) == 64 else "skew", True, True)]
    for i in range(7):
        f.append(Shape("block", pl.take(b, dmax=dmax_gate - 1.5), "sym", True, True))
    for i in range(8):
        f.append(Shape("distant block", pl.take(b, dmin=dmax_gate + 1.5), "none", False, True))
    return Scene(_with_ordinary(f, dmax=dmax_gate - 1.5), dyn=dict(classification__max_distance=dmax_gate), trips="members" if n > 1024 else None)


def scene_member_512():
    """case 2, the staging area: a 4 x 4 x 5 block (80 voxels: first in the canonical order) and ten 4 x 4 x 4 blocks, 720 candidate
    members, all under the gates - the seventh 64-voxel block takes list positions 464 .. 527, across member 512"""
    pl = Placer()
    f = [Shape("block 4x4x5", pl.take(block(4, 4, 5)), "sym", True, True)] + [Shape("block", pl.take(block(4, 4, 4)), "sym", True, True) for _ in range(10)]
    return Scene(_with_ordinary(f))


def scene_detections(n):
    """case 3: n floating 2-voxel clusters of all orientations in frame 0 plus six diagonal-line fillers (n + 6 < 64 candidates);
    the map holds pockets of unknown voxels around the first six clusters (the members' own cells included: a fill starts there)
    - boxes, bars and an L of cells, nowhere near a fill's rim or the background - so these fills write frontier voxels"""
    pl = Placer()
    f, unknown = [], []
    names = list(PAIRS)
    for i in range(n):
        cells = pl.take(PAIRS[names[i % len(names)]])
        f.append(Shape(names[i % len(names)], cells, "sym", True, True))
        c = cells[0]
        if i < 6:
            if i % 3 == 0:  # a 3 x 3 x 3 box around the first member, the second one included or touched
                unknown.append(block(3, 3, 3) - 1 + c)
            elif i % 3 == 1:  # a bar through both members and four cells on
                unknown.append(np.vstack([cells, line(5, i % 2) + cells[1]]))
            else:  # the first member alone and an L of cells behind it
                unknown.append(np.vstack([c[None, :], c - line(4, 0), c - line(4, 0)[-1] + line(3, 2)]))
    for i in range(6):
        f.append(Shape(f"diagonal line {8 + i % 3}", pl.take(diag_line(8 + i % 3, (1, 1, 1))), "none", False, True))
    unknown = np.unique(np.vstack(unknown), axis=0)
    frames = [f] + [ordinary_frame(k, reserved=[unknown]) for k in (0, 1, 2)]
    return Scene(frames, unknown=unknown, trips="dets" if n > 16 else None)


POCKET_RIM = (np.array([300, 200, 62]), 34)   # every voxel unknown out to Manhattan radius 34: a fill of R = 32 / 33 reaches its rim
POCKET_FULL = (np.array([400, 200, 62]), 29)  # ... out to radius 29: a fill of R = 32 explores all of it (37 k voxels) and finds no rim


def scene_radius(max_explore, R, open_):
    """case 4: every cluster of the scene is a 2-voxel cluster with an OBB diagonal of 0.25 m or 0.354 m, so that
    R = int((obb_size + max_explore) / 0.25) is the same for all of them.  Frame 0: five plain ones, one in the middle of a
    pocket that is unknown out to Manhattan radius 34 (the fill meets its rim: no detection), one in a pocket unknown out to
    radius 29 (the fill explores the whole pocket - the largest work list a fill of R = 32 can have without meeting its rim - writes
    it to the map as frontier voxels and the cluster is a detection)."""
    keep = [POCKET_RIM, POCKET_FULL]
    pl = Placer(keepout=keep)
    det = None if open_ else True
    f = [Shape(n, pl.take(PAIRS[n]), "sym", det, True) for n in FLAT_PAIRS[:5]]
    f.append(Shape("pair x in rim pocket", np.array(POCKET_RIM[0]) + line(2, 0), "none", None if open_ else False, True))
    f.append(Shape("pair x in full pocket", np.array(POCKET_FULL[0]) + line(2, 0), "sym", det, True))
    unknown = np.vstack([diamond(*POCKET_RIM), diamond(*POCKET_FULL)])
    frames = [f] + [ordinary_frame(k, names=tuple(FLAT_PAIRS), keepout=keep) for k in (0, 1, 2)]
    return Scene(frames, dyn=dict(classification__max_explore_distance=max_explore), unknown=unknown, trips="open" if open_ else ("radius" if R > 32 else None), R=R)


def scene_gates():
    """case 5, min_points = 2, max_size = 3.0, max_distance lowered to 25 m: lines of 12 / 13 / 14 voxels along x, y, z (OBB diagonal
    2.75 / 3.00 / 3.25 m: detection / the oracle decides / not even a candidate, its extent 3.25 m fails the prefilter), the
    diagonal lines of case 1 (candidates over max_size), single voxels (min_points - 1) and pairs (min_points), and two identical
    pairs along y 24.49 m and 25.50 m from the sensor (0.51 m inside and 0.50 m outside max_distance)."""
    gate = 25.0
    pl = Placer(pitch=28)
    s = SENSOR_CELL
    inside = np.array([[350 + 88, 199, 20 + 43], [350 + 88, 200, 20 + 43]])
    outside = np.array([[350 - 92, 199, 20 + 44], [350 - 92, 200, 20 + 44]])
    assert abs(dist_m(inside) - (gate - 0.5)) < 0.02 and abs(dist_m(outside) - (gate + 0.5)) < 0.02, (dist_m(inside), dist_m(outside), s)
    f = [Shape("pair y inside max_distance", pl.put(inside), "sym", True, True), Shape("pair y outside max_distance", pl.put(outside), "none", False, True)]
    for axis in range(3):
        f.append(Shape(f"line 12 axis {axis}", pl.take(line(12, axis), dmax=gate - 1.5), "sym", True, True))
        f.append(Shape(f"line 13 axis {axis}", pl.take(line(13, axis), dmax=gate - 1.5), "none", None, True))  # exactly max_size: held to the oracle only
        f.append(Shape(f"line 14 axis {axis}", pl.take(line(14, axis), dmax=gate - 1.5), "none", False, False))
    for i in range(6):
        f.append(Shape(f"diagonal line {8 + i % 3}", pl.take(diag_line(8 + i % 3, (1, 1, 1) if i % 2 else (1, -1, 1)), dmax=gate - 1.5), "none", False, True))
    for i in range(3):
        f.append(Shape("single voxel", pl.take(line(1, 0), dmax=gate - 1.5), "none", False, False))
        f.append(Shape(list(PAIRS)[i], pl.take(PAIRS[list(PAIRS)[i]], dmax=gate - 1.5), "sym", True, True))
    return Scene(_with_ordinary(f, dmax=gate - 1.5), dyn=dict(classification__max_distance=gate))


def scene_min_points_4():
    """case 5, min_points = 4: clusters of 3 voxels (a line, an L) and of 2 are no candidates, clusters of 4 (a line, a square, the
    tetrahedron) are detections"""
    pl = Placer()
    f = []
    for rep in range(2):
        f += [Shape("line 3", pl.take(line(3, rep)), "none", False, False), Shape("L triple", pl.take(L_TRIPLE), "none", False, False),
              Shape("pair", pl.take(line(2, 2 - rep)), "none", False, False), Shape("line 4", pl.take(line(4, rep)), "sym", True, True),
              Shape("2x2 square", pl.take(_norm(ALIGNED["2x2 square"])), "sym", True, True), Shape("tetrahedron", pl.take(TETRAHEDRA["tetrahedron (1, 1, 1)"]), "skew", True, True)]
    names = ("2x2x2 cube", "plus", "2x2 square", "3x3 square")
    return Scene([f] + [ordinary_frame(k, names=names) for k in (0, 1, 2)], dyn=dict(classification__min_points=4))


def scene_degenerate():
    """case 6: the shapes of test_obb_gates_on_degenerate_lattice_clusters - the aligned ones, the diagonal pairs / triples, the
    tetrahedron in four orientations, an L triple and 40 random sub-blocks of 3 x 3 x 3 (seed 9) - at map x above 62 m.  All 55 are
    floating.  One frame cannot hold them on the device routes: beyond 16 detections a batch is redone by the host tail, whose boxes
    are the host's.  They are dealt over the four frames of a batch, 14 / 14 / 14 / 13, and every frame also runs as a single scan."""
    frames = [[] for _ in range(4)]
    pls = [Placer(pitch=14, x=(330, 456), skip=5 * k) for k in range(4)]
    for i, (n, c, kind) in enumerate(_degenerate_shapes()):
        frames[i % 4].append(Shape(n, pls[i % 4].take(c), kind, True, True))
    return Scene(frames, scan_frames=(0, 1, 2, 3))


def scene_degenerate_one_scan():
    """case 6 as the issue words it, one frame with all 55 shapes - for the single map-updating scan only: 55 detections are more
    than the record slots hold, the records are rebuilt from the clusters on the device and carry the device's boxes"""
    pl = Placer(pitch=14, x=(330, 456))
    return Scene([[Shape(n, pl.take(c), kind, True, True) for n, c, kind in _degenerate_shapes()]], trips="dets", scan_frames=(0,))


def _degenerate_shapes():
    todo = [(n, _norm(c), "sym") for n, c in ALIGNED.items()] + [(n, _norm(c), "sym") for n, c in DIAGONALS.items()] + [(n, c, "skew") for n, c in TETRAHEDRA.items()]
    todo += [("L triple", L_TRIPLE, "skew")] + [(f"random sub-block {i}", c, "skew") for i, c in enumerate(random_subblocks(40))]
    return todo
