"""vofod_map_match and vofod_pose_lattice: the numpy statement of include/vofod.h, MAP MATCH - written from the header's text in
float32 with every operation rounded once, one candidate at a time - the lattice in float64, and the fixtures
test_map_match_cpu.py and test_gpu_map_match.py share.  The beam and the decode are range_motion_cases' (beam_points,
motion_definition) - imported, not copied; the transform, the float bounds test and the counts are written out here.  Nothing comes
from the product."""
from types import SimpleNamespace

import numpy as np

import map_render_cases as mrc
import map_render_scans_cases as sc
import range_motion_cases as rm
from vofod_amd.detector import VoFOD, default_params

F = np.float32
SKIPPED, OUTSIDE, FREE, OCCUPIED = range(4)
NAMES = ("SKIPPED", "OUTSIDE", "FREE", "OCCUPIED")


# ------------------------------------------------------------------------------------------------ the statement
def scan_points(g, scan, lo, hi, shift_by_row=None):
    """(p [n, 3] float32, zero [n] bool): the scan's point of every pixel and the pixels without a return.  scan: an object with
    either `xyz` ([n, 3] float32: a point scan) or `range` (n uint32) and `col_tfs` ([w, 3, 4] float32 or None)."""
    if getattr(scan, "xyz", None) is not None:
        p = np.ascontiguousarray(scan.xyz, dtype=F).reshape(-1, 3)
        return p, (p == 0).all(axis=1)  # (either sign of zero)
    rng = np.ascontiguousarray(scan.range, dtype=np.uint32).reshape(-1)
    if scan.col_tfs is None:
        q = np.stack(rm.beam_points(rng, g.dirs, g.offs), axis=1)
        return np.where((rng == 0)[:, None], F(0.0), q).astype(F), rng == 0
    x, y, z, _ = rm.motion_definition(rng, g.dirs, g.offs, scan.col_tfs, g.w, lo, hi, shift_by_row)
    return np.stack([x, y, z], axis=1).astype(F), rng == 0


def skipped(p, zero, lo, hi):
    """SKIPPED of the header: no return, a coordinate that is not finite, or inside the closed exclude box"""
    finite = np.isfinite(p).all(axis=1)
    with np.errstate(invalid="ignore"):
        box = ((p >= np.asarray(lo, F)[None]) & (p <= np.asarray(hi, F)[None])).all(axis=1)
    return zero | ~finite | box


def classes(g, m, p, skip, tf, threshold):
    """the class of every pixel under ONE candidate: uint8 [n]"""
    tf = np.asarray(tf, dtype=F).reshape(3, 4)
    flat = np.ascontiguousarray(m, dtype=F).reshape(-1)
    sx, sy, sz = g.size
    inv = F(1.0) / F(g.vs)
    inside = np.ones(len(p), dtype=bool)
    f = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            w = (tf[a, 0] * p[:, 0]) + ((tf[a, 1] * p[:, 1]) + ((tf[a, 2] * p[:, 2]) + tf[a, 3]))
            assert w.dtype == F
            fa = np.floor((w - F(g.off[a])) * inv)
            assert fa.dtype == F
            inside &= (fa >= F(0.0)) & (fa < F(g.size[a]))  # (compared as floats: a NaN or an infinity is outside)
            f.append(fa)
    c = [np.where(inside, fa, F(0.0)).astype(np.int64) for fa in f]  # (only floats of [0, size) are converted)
    v = (c[2] * sy + c[1]) * sx + c[0]
    with np.errstate(invalid="ignore"):
        occ = flat[v] > F(threshold)  # (a NaN voxel is FREE, +inf OCCUPIED, an equal one FREE)
    cls = np.where(skip, SKIPPED, np.where(~inside, OUTSIDE, np.where(occ, OCCUPIED, FREE)))
    return cls.astype(np.uint8)


def statement(g, m, scan, tfs, threshold, lo=(0.0, 0.0, 0.0), hi=(0.0, 0.0, 0.0), shift_by_row=None):
    """The whole call: SimpleNamespace(counts uint32 [K, 4], best, skipped bool [n], classes uint8 [K, n])"""
    tfs = np.asarray(tfs, dtype=F).reshape(-1, 3, 4)
    p, zero = scan_points(g, scan, lo, hi, shift_by_row)
    skip = skipped(p, zero, lo, hi)
    cls = np.stack([classes(g, m, p, skip, tf, threshold) for tf in tfs])
    counts = np.stack([np.bincount(c, minlength=4) for c in cls]).astype(np.uint32)
    return SimpleNamespace(counts=counts, best=int(np.argmax(counts[:, OCCUPIED])), skipped=skip, classes=cls)


def lattice(tf, step, n, yaw_step=0.0, n_yaw=1):
    """vofod_pose_lattice in float64: [n0 * n1 * n2 * n_yaw, 3, 4], rounded to float32 once per entry by the caller's astype"""
    tf = np.asarray(tf, dtype=F).reshape(3, 4).astype(np.float64)
    step = np.asarray(step, dtype=F).astype(np.float64)
    out = []
    for iyaw in range(n_yaw):
        psi = (iyaw - (n_yaw - 1) / 2.0) * float(F(yaw_step))
        c, s = np.cos(psi), np.sin(psi)
        for iz in range(n[2]):
            for iy in range(n[1]):
                for ix in range(n[0]):
                    k = np.empty((3, 4))
                    k[0, :3] = c * tf[0, :3] - s * tf[1, :3]
                    k[1, :3] = s * tf[0, :3] + c * tf[1, :3]
                    k[2, :3] = tf[2, :3]
                    for a, i in enumerate((ix, iy, iz)):
                        k[a, 3] = tf[a, 3] + (i - (n[a] - 1) / 2.0) * step[a]
                    out.append(k)
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ handles and geometry
# the sensors of map_render_scans_cases (two waves; a ragged wave under an Ouster LUT with offsets; a second block of 8 lanes) and
# one of eight blocks
SENSORS = dict(sc.SENSORS, **{"64x32": (64, 32, (5.0, 3.0, 2.0), 0.25, False)})
THRESHOLD = 0.5
# an exclude box that removes the nearest returns: (size, offset) of vofod_static_params; the z offset is the box's bottom
EXCLUDE = ((1.2, 1.0, 0.6), (0.1, 0.0, -0.3))


def exclude_bounds(exclude):
    if exclude is None:
        return np.zeros(3, F), np.zeros(3, F)
    return rm.exclude_bounds(SimpleNamespace(exclude_size=exclude[0], exclude_offset=exclude[1]))


def make_det(lib, name, dirs, offs=None, exclude=None, max_batch=1, area_offset=(0.0, 0.0, 0.0)):
    w, h, area, vs, _ = SENSORS[name]
    sp, dp = default_params(lib)
    sp.voxel_size = vs
    sp.sensor_hrays, sp.sensor_vrays = w, h
    sp.sensor_vfov = F(np.deg2rad(45.0))
    sp.max_batch_frames = max_batch
    for a in range(3):
        sp.oparea_size[a], sp.oparea_offset[a] = area[a], area_offset[a]
        sp.exclude_size[a], sp.exclude_offset[a] = (0.0, 0.0) if exclude is None else (exclude[0][a], exclude[1][a])
    return VoFOD(lib, sp, dp, lut_directions=dirs, lut_offsets=offs)


def lut_of(name, lib=None):
    if name in sc.SENSORS:
        return sc.lut_of(name, lib)
    w, h = SENSORS[name][:2]
    return mrc.sim_lut(w, h), None


def geometry(name, dirs, offs):
    """the geometry of the handle make_det builds (VoxelMap::resize: ceil(area / vs) + 1 voxels, centred in x and y, z from the bottom)"""
    w, h, area, vs, _ = SENSORS[name]
    size = tuple(int(np.ceil(a / vs)) + 1 for a in area)
    off = np.array([-area[0] / 2.0, -area[1] / 2.0, 0.0], dtype=F)
    return SimpleNamespace(size=size, off=off, vs=F(vs), dirs=np.asarray(dirs, F).reshape(-1, 3), offs=None if offs is None else np.asarray(offs, F).reshape(-1, 3), h=h, w=w)


def centre_pose(g):
    sx, sy, sz = g.size
    return mrc.pose(mrc.voxel_centre(g, sx // 2, sy // 2, sz // 2) + 0.03)


def candidates(g, n_poses, seed=0):
    """n_poses candidates [n, 3, 4]: the centre; a general rotation; the four quarter turns about z; a NaN entry; an infinite
    entry; one that pushes every point out through each of the six faces; then small random motions around the centre.  With
    fewer than 14 asked for, the head of that list."""
    rs = np.random.default_rng(seed + 23)
    c = centre_pose(g)
    t = c[:, 3].astype(np.float64)
    out = [c, mrc.pose(t + 0.11, yaw=0.7, pitch=-0.4, roll=0.2)]
    out += [mrc.pose(t, yaw=k * np.pi / 2) for k in range(1, 4)]
    for k in range(1, 4):  # (an exact quarter turn: entries 0 and +-1)
        out[1 + k][:, :3] = np.rint(out[1 + k][:, :3])
    bad = c.copy()
    bad[1, 2] = np.nan
    out.append(bad)
    bad = c.copy()
    bad[0, 3] = np.inf
    out.append(bad)
    extent = [float(g.vs) * s for s in g.size]
    for a in range(3):
        for sign in (-1.0, 1.0):
            far = c.copy()
            far[a, 3] += F(sign * 2.0 * extent[a])
            out.append(far)
    while len(out) < n_poses:
        out.append(mrc.pose(t + rs.uniform(-0.6, 0.6, 3), yaw=rs.uniform(-0.5, 0.5), pitch=rs.uniform(-0.1, 0.1), roll=rs.uniform(-0.1, 0.1)))
    return np.stack(out[:n_poses]).astype(F)


def ranges_of(g, seed=0):
    """uint32 millimetres: an eighth without a return, the others up to beyond the map's half extent"""
    rs = np.random.default_rng(seed + 29)
    r = rs.integers(150, 3600, g.w * g.h).astype(np.uint32)
    r[rs.random(r.size) < 0.125] = 0
    return r


def keep_live(rng_or_xyz, skip, n_live):
    """the input with every live pixel behind the first n_live of them turned into 'no return'"""
    out = np.array(rng_or_xyz)
    live = np.flatnonzero(~skip)
    out[live[n_live:]] = 0
    return out


def device_case(lib, name, kind="range", n_poses=300, map_kind="random", exclude=None, seed=0):
    """Everything one device case needs but the handle.  kind: "range" (a range image), "motion" (with a table, under column
    shifts), "points" (a point scan: the decoded points, with a NaN, an infinity and signed zeros put in)."""
    w, h = SENSORS[name][:2]
    dirs, offs = lut_of(name, lib)
    g = geometry(name, dirs, offs)
    m = {"random": lambda: mrc.random_map(g.size, seed + 11, THRESHOLD, frac=0.15), "empty": lambda: np.full(g.size[::-1], -1.0, F), "solid": lambda: np.full(g.size[::-1], 3.0, F)}[map_kind]()
    lo, hi = exclude_bounds(exclude)
    rng = ranges_of(g, seed)
    shifts = sc.column_shifts(w, h, seed) if kind == "motion" else None
    table = np.ascontiguousarray(sc.small_table(lib, w, seed), F) if kind == "motion" else None
    scan = SimpleNamespace(range=rng, col_tfs=table, xyz=None)
    if kind == "points":
        p, _ = scan_points(g, scan, lo, hi)
        p = p.copy()
        p[3], p[5, 1], p[7, 2] = (-0.0, 0.0, -0.0), np.nan, np.inf
        scan = SimpleNamespace(range=None, col_tfs=None, xyz=p)
    tfs = candidates(g, n_poses, seed)
    exp = statement(g, m, scan, tfs, THRESHOLD, lo, hi, shifts)
    return SimpleNamespace(name=name, kind=kind, w=w, h=h, dirs=dirs, offs=offs, g=g, m=m, lo=lo, hi=hi, exclude=exclude, shifts=shifts, table=table, scan=scan, tfs=tfs, exp=exp,
                           threshold=THRESHOLD)


_CASES = {}


def shared_case(lib, name, kind="range", n_poses=300, map_kind="random", exclude=None):
    """device_case, computed once per process and left unchanged"""
    key = (name, kind, n_poses, map_kind, exclude)
    if key not in _CASES:
        _CASES[key] = device_case(lib, name, kind, n_poses, map_kind, exclude)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ the hand map
def hand_geometry(points):
    """map_render_cases' 5 x 4 x 3 hand map at 0.5 m, origin (-1, -0.75, 0), under a 'sensor' whose n pixels decode to `points` at a
    range of 1000 mm (1000 * 0.001f == 1.0f): directions = points, no offsets"""
    p = np.asarray(points, F).reshape(-1, 3)
    return SimpleNamespace(size=mrc.HAND_SIZE, off=np.asarray(mrc.HAND_OFF, F), vs=F(mrc.HAND_VS), dirs=p, offs=None, h=1, w=len(p))


# ------------------------------------------------------------------------------------------------ the end-to-end scene
# A 48 x 24 sensor with a 90 degree field of view in a 21 x 13 x 9 map at 0.25 m.  The map is asymmetric: a floor one voxel thick,
# a wall one voxel thick across +x that ends before the -y side, and a box of 2 x 2 x 3 voxels off the centre on the +y side.  The
# scan is rendered from pose P; the returns lie in the middle of the pieces of the hit voxels, so under P every return is OCCUPIED,
# and a candidate a voxel or a few degrees off loses the returns of the surfaces that face the motion.
E2E_NAME = "48x24"
SENSORS[E2E_NAME] = (48, 24, (5.0, 3.0, 2.0), 0.25, False)
E2E_LATTICE = ((5, 5, 3), 3, 0.06)  # counts, n_yaw, yaw_step; the step is the voxel size
E2E_THRESHOLD, E2E_LENGTH = 0.0, 8.0


def e2e_case():
    w, h = SENSORS[E2E_NAME][:2]
    dirs = mrc.sim_lut(w, h, 90.0)
    g = geometry(E2E_NAME, dirs, None)
    m = np.full(g.size[::-1], -1.0, F)  # [z, y, x]
    m[0, :, :] = 3.0          # the floor
    m[1:, 3:, 17] = 3.0       # the wall across +x, open on the -y side
    m[1:4, 9:11, 5:7] = 3.0   # the box, behind the sensor on the +y side
    P = mrc.pose(mrc.voxel_centre(g, 10, 6, 4) + np.array([0.02, -0.03, 0.01]), yaw=0.2)
    seen = mrc.render(g, m, P[None], E2E_THRESHOLD, E2E_LENGTH)
    n, n_yaw, yaw_step = E2E_LATTICE
    tfs = lattice(P, (g.vs,) * 3, n, yaw_step, n_yaw).astype(F)
    centre = (n[0] * n[1] * n[2] * n_yaw) // 2
    scan = SimpleNamespace(range=seen.range[0].reshape(-1), col_tfs=None, xyz=None)
    exp = statement(g, m, scan, tfs, E2E_THRESHOLD)
    return SimpleNamespace(g=g, dirs=dirs, w=w, h=h, map=m, P=P, range=seen.range[0], tfs=tfs, centre=centre, exp=exp, lattice=E2E_LATTICE)
