"""vofod_map_distance and vofod_map_match_field: the numpy statement of include/vofod.h, MAP DISTANCE, and the fixtures
test_map_distance_cpu.py and test_gpu_map_distance.py share.  The distance is a brute-force minimum over ALL occupied voxels in
int64 - no window, no separation by axes: nothing of how the device computes it.  The field match takes the scan's point and
SKIPPED from map_match_cases (imported, not copied) and the transform written out as that file's `classes` writes it (held equal to
it in test_map_distance_cpu.py); behind them it is a gather, a bincount and an int64 sum.  Nothing comes from the product."""
from types import SimpleNamespace

import numpy as np

import map_match_cases as mm
import map_render_cases as mrc

F = np.float32
SKIPPED, OUTSIDE, FAR, NEAR = range(4)
MAX_RADIUS = 255


# ------------------------------------------------------------------------------------------------ the statement: the distance
def occupied(m, threshold):
    """bool [sz, sy, sx]: map > threshold as floats - a NaN voxel is free, +inf occupied, one equal to the threshold free"""
    with np.errstate(invalid="ignore"):
        return np.asarray(m, F) > F(threshold)


def nearest2(occ):
    """int64 [sz, sy, sx]: the squared distance, in voxels, to the nearest True voxel of `occ`, by brute force over all of them;
    where there is none, a value above every clamp"""
    occ = np.asarray(occ, bool)
    out = np.full(occ.size, np.iinfo(np.int64).max, np.int64)
    u = np.argwhere(occ).astype(np.int64)  # (z, y, x) of every occupied voxel
    if len(u):
        v = np.argwhere(np.ones(occ.shape, bool)).astype(np.int64)  # ... of every voxel, in the order of v = (z * sy + y) * sx + x
        step = max(1, (1 << 22) // len(u))
        for a in range(0, len(v), step):
            d = v[a : a + step, None, :] - u[None, :, :]
            out[a : a + step] = (d * d).sum(axis=2).min(axis=1)
    return out.reshape(occ.shape)


def clamp(full, radius):
    return np.minimum(full, np.int64(radius) * radius).astype(np.uint16)


def distance(m, threshold, radius):
    """vofod_map_distance: uint16 [sz, sy, sx]"""
    return clamp(nearest2(occupied(m, threshold)), radius)


def distance_edt(m, threshold, radius):
    """the same from scipy's exact Euclidean transform - an independent statement: the distance to the nearest zero of ~occ, squared
    and rounded back to the integer it is.  (A map with nothing occupied has no zero to measure to: R * R by the definition.)"""
    from scipy import ndimage

    occ = occupied(m, threshold)
    if not occ.any():
        return np.full(occ.shape, radius * radius, np.uint16)
    return np.minimum(np.rint(ndimage.distance_transform_edt(~occ) ** 2), radius * radius).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ the statement: the field match
def voxel_of(g, p, tf):
    """(inside bool [n], v int64 [n]): MAP MATCH's candidate, float bounds test and v, as map_match_cases.classes writes them;
    v is 0 where the point is not inside"""
    tf = np.asarray(tf, dtype=F).reshape(3, 4)
    sx, sy, sz = g.size
    inv = F(1.0) / F(g.vs)
    inside = np.ones(len(p), dtype=bool)
    f = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            w = (tf[a, 0] * p[:, 0]) + ((tf[a, 1] * p[:, 1]) + ((tf[a, 2] * p[:, 2]) + tf[a, 3]))
            fa = np.floor((w - F(g.off[a])) * inv)
            assert w.dtype == F and fa.dtype == F
            inside &= (fa >= F(0.0)) & (fa < F(g.size[a]))
            f.append(fa)
    c = [np.where(inside, fa, F(0.0)).astype(np.int64) for fa in f]
    return inside, (c[2] * sy + c[1]) * sx + c[0]


def field_statement(g, d2, scan, tfs, near2, outside_cost, lo=(0.0, 0.0, 0.0), hi=(0.0, 0.0, 0.0), shift_by_row=None):
    """vofod_map_match_field: SimpleNamespace(counts uint32 [K, 4], cost uint64 [K], best)"""
    tfs = np.asarray(tfs, dtype=F).reshape(-1, 3, 4)
    field = np.ascontiguousarray(d2, np.uint16).reshape(-1).astype(np.int64)
    p, zero = mm.scan_points(g, scan, lo, hi, shift_by_row)
    skip = mm.skipped(p, zero, lo, hi)
    counts, cost = [], []
    for tf in tfs:
        inside, v = voxel_of(g, p, tf)
        d = field[v]  # the gather
        cls = np.where(skip, SKIPPED, np.where(~inside, OUTSIDE, np.where(d <= int(near2), NEAR, FAR)))
        c = np.bincount(cls, minlength=4)
        counts.append(c)
        cost.append(int(d[~skip & inside].sum()) + int(outside_cost) * int(c[OUTSIDE]))
    cost = np.array(cost, dtype=np.uint64)
    return SimpleNamespace(counts=np.stack(counts).astype(np.uint32), cost=cost, best=int(np.argmin(cost)))


# ------------------------------------------------------------------------------------------------ the maps of the distance tests
# name -> (size in voxels, operation area at 0.25 m: VoxelMap::resize gives ceil(area / vs) + 1 voxels per axis)
VS = 0.25
MAPS = {
    "9x9x9": (9, 9, 9),        # 729 voxels: a ragged last bit word
    "21x13x9": (21, 13, 9),
    "130x3x2": (130, 3, 2),    # a row crosses two word boundaries, rows start mid-word
    "300x5x3": (300, 5, 3),    # an axis longer than 255 and than a block of 256 threads
    "3x70x2": (3, 70, 2),      # the long axis is the one the y pass walks: three tiles of 32 rows
    "3x2x70": (3, 2, 70),      # ... the z pass
}
RADII = (1, 2, 3, 8, 64, 65, 255)
THRESHOLD = 0.5
CORNERS = tuple((ix, iy, iz) for iz in (0, 1) for iy in (0, 1) for ix in (0, 1))
CONTENTS = ("empty", "solid") + tuple(f"corner{k}" for k in range(8)) + ("random0.2", "random5", "random50")


def area_of(size):
    return tuple((s - 1) * VS for s in size)


def make_det(lib, name, w=2, h=2, max_batch=1):
    """a handle whose map is MAPS[name], under the smallest sensor a handle takes"""
    dev = mrc.make_det(lib, w, h, area_of(MAPS[name]), VS, mrc.sim_lut(w, h), max_batch=max_batch)
    assert tuple(dev.map_size) == MAPS[name], (dev.map_size, name)
    return dev


def random_map(size, seed, threshold, frac):
    """`frac` of the voxels above the threshold; one or a few voxels each of NaN, +inf (occupied), -0.0, the threshold itself (free)
    and -inf put in"""
    rs = np.random.default_rng(seed)
    sx, sy, sz = size
    m = rs.uniform(-10.0, float(threshold) - 0.5, size=(sz, sy, sx)).astype(F)
    m[rs.random(m.shape) < frac] = F(threshold) + F(rs.uniform(0.5, 5.0))
    flat = m.reshape(-1)
    k = max(flat.size // 400, 1)
    at = rs.choice(flat.size, size=5 * k, replace=False)  # (distinct voxels: no special value overwrites another)
    for i, val in enumerate((np.nan, np.inf, -0.0, threshold, -np.inf)):
        flat[at[i * k : (i + 1) * k]] = F(val)
    return m


def content(name, kind, threshold=THRESHOLD):
    """float32 [sz, sy, sx]"""
    size = MAPS[name]
    sx, sy, sz = size
    if kind == "empty":
        return np.full((sz, sy, sx), threshold, F)  # (equal to the threshold: free)
    if kind == "solid":
        return np.full((sz, sy, sx), threshold + 1.0, F)
    if kind.startswith("corner"):
        cx, cy, cz = CORNERS[int(kind[6:])]
        m = np.full((sz, sy, sx), np.nan, F)  # (NaN: free)
        m[cz * (sz - 1), cy * (sy - 1), cx * (sx - 1)] = np.inf
        return m
    return random_map(size, sum(size) + len(kind), threshold, float(kind[6:]) / 100.0)


_FULL = {}


def shared_full(name, kind, threshold=THRESHOLD):
    """(map, unclamped squared distances) of one test map and content, computed once per process and left unchanged"""
    key = (name, kind, threshold)
    if key not in _FULL:
        m = content(name, kind, threshold)
        full = nearest2(occupied(m, threshold))
        m.setflags(write=False)
        full.setflags(write=False)
        _FULL[key] = (m, full)
    return _FULL[key]


def random_field(n, seed):
    """an arbitrary field: any uint16 values, 0 and 65535 among them"""
    f = np.random.default_rng(seed).integers(0, 65536, n).astype(np.uint16)
    f[:2] = (0, 65535)
    return f


# ------------------------------------------------------------------------------------------------ the end-to-end scene
# map_match_cases.e2e_case() - the scan rendered from pose P in the asymmetric 21 x 13 x 9 scene, and its 5 x 5 x 3 lattice with
# three yaws, one voxel apart: two steps either side of the centre along x and y, which is the ring the slope is asked on
E2E_RADIUS, E2E_NEAR2 = 8, 0
E2E_OUTSIDE_COST = E2E_RADIUS * E2E_RADIUS  # a return outside the map costs what one beyond the radius costs


def e2e_field_case():
    e = mm.e2e_case()
    d2 = distance(e.map, mm.E2E_THRESHOLD, E2E_RADIUS)
    scan = SimpleNamespace(range=e.range.reshape(-1), col_tfs=None, xyz=None)
    exp = field_statement(e.g, d2, scan, e.tfs, E2E_NEAR2, E2E_OUTSIDE_COST)
    return SimpleNamespace(e=e, d2=d2, scan=scan, exp=exp)
