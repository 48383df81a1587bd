"""vofod_map_render: the numpy statement of include/vofod.h, MAP RENDER - written from the header's text, one ray at a time in
float32 with every operation rounded once - and the case builders test_map_render_cpu.py and test_gpu_map_render.py share."""
from types import SimpleNamespace

import numpy as np

from vofod_amd import capi
from vofod_amd.detector import VoFOD, default_params

F = np.float32
NOT_CAST, HIT, END, LEFT = capi.RENDER_NOT_CAST, capi.RENDER_HIT, capi.RENDER_END, capi.RENDER_LEFT
NO_VOXEL = 0xFFFFFFFF
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the statement
def rays(tf, dirs, offs):
    """dir = R d, start = (R o) + t for every pixel: [n, 3] float32 each, in the header's association (numpy fuses nothing)"""
    tf = np.asarray(tf, dtype=F).reshape(3, 4)
    d = np.asarray(dirs, dtype=F).reshape(-1, 3)
    o = np.zeros_like(d) if offs is None else np.asarray(offs, dtype=F).reshape(-1, 3)
    dir_ = np.stack([((tf[k, 0] * d[:, 0]) + (tf[k, 1] * d[:, 1])) + (tf[k, 2] * d[:, 2]) for k in range(3)], axis=1)
    start = np.stack([(((tf[k, 0] * o[:, 0]) + (tf[k, 1] * o[:, 1])) + (tf[k, 2] * o[:, 2])) + tf[k, 3] for k in range(3)], axis=1)
    assert dir_.dtype == F and start.dtype == F
    return dir_, start


def walk(start, dir_, m, off, vs, threshold, length):
    """One ray through the map `m` ([sz, sy, sx] float32).  Returns (what, voxel, t_in, t_out, visited): visited lists every voxel
    the loop looked at as (linear index, ddist) with ddist = min(dist, length) - prev, the piece forEachRay would hand out."""
    vs, length, threshold = F(vs), F(length), F(threshold)
    size = (m.shape[2], m.shape[1], m.shape[0])
    flat = m.reshape(-1)
    inv, half = F(1.0) / vs, vs / F(2.0)
    cur, step, last, tdelta, tmax = [0] * 3, [0] * 3, [0] * 3, [F(0)] * 3, [F(0)] * 3
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            cur[a] = int(np.floor((F(start[a]) - F(off[a])) * inv))
        if any(cur[a] < 0 or cur[a] >= size[a] for a in range(3)):
            return NOT_CAST, NO_VOXEL, F(0), F(0), []
        for a in range(3):
            d = F(dir_[a])
            ad = np.abs(d)
            step[a] = int(d > 0) - int(d < 0)
            last[a] = size[a] - 1 if step[a] > 0 else 0
            tdelta[a] = (F(1.0) / ad) * vs
            ctr = ((F(cur[a]) + F(0.5)) * vs) + F(off[a])
            tmax[a] = (half + (F(step[a]) * (ctr - F(start[a])))) / ad
        prev = F(0)
        visited = []
        while True:
            a = 0
            if tmax[1] < tmax[a]:
                a = 1
            if tmax[2] < tmax[a]:
                a = 2
            dist = tmax[a]
            t_out = dist if dist < length else length  # min(dist, length); a NaN dist cannot arise from finite inputs
            lin = (cur[2] * size[1] + cur[1]) * size[0] + cur[0]
            visited.append((lin, F(t_out - prev)))
            if flat[lin] > threshold:
                return HIT, lin, prev, t_out, visited
            if not (dist < length):
                return END, NO_VOXEL, prev, t_out, visited
            if cur[a] == last[a]:
                return LEFT, NO_VOXEL, prev, t_out, visited
            cur[a] += step[a]
            tmax[a] = tmax[a] + tdelta[a]
            prev = dist


def range_mm(t_in, t_out):
    """the header's range of a HIT: the middle of the piece in millimetres, ties to even, at least 1"""
    mm = np.rint(((F(t_in) + F(t_out)) * F(0.5)) * F(1000.0))
    return max(1, int(min(max(mm, F(0)), F(4294967040.0))))


def render(g, m, tfs, threshold, length, want_visited=False, pixels=None):
    """The statement for a whole call (`pixels`: only these pixel indices are walked - the others stay NOT_CAST - for sensors too
    large to walk in Python; sample() cuts the same pixels out of a device answer).  g: geometry (size (sx, sy, sz), off, vs, dirs, offs, h, w); m: the voxel map [sz, sy, sx].
    Returns SimpleNamespace(range, voxel, what, tio[, visited]) shaped like VoFOD.map_render's result."""
    tfs = np.asarray(tfs, dtype=F).reshape(-1, 3, 4)
    n = g.h * g.w
    out = SimpleNamespace(range=np.zeros((len(tfs), n), np.uint32), voxel=np.full((len(tfs), n), NO_VOXEL, np.uint32), what=np.zeros((len(tfs), n), np.uint8),
                          tio=np.zeros((len(tfs), n, 2), F), visited=[])
    m = np.ascontiguousarray(m, dtype=F)
    for v, tf in enumerate(tfs):
        dir_, start = rays(tf, g.dirs, g.offs)
        vis = []
        for i in (range(n) if pixels is None else pixels):
            what, vox, t_in, t_out, visited = walk(start[i], dir_[i], m, g.off, g.vs, threshold, length)
            out.what[v, i], out.voxel[v, i], out.tio[v, i] = what, vox, (t_in, t_out)
            out.range[v, i] = range_mm(t_in, t_out) if what == HIT else 0
            vis.append(visited)  # (in the order walked)
        out.visited.append(vis)
    for k in ("range", "voxel", "what"):
        setattr(out, k, getattr(out, k).reshape(len(tfs), g.h, g.w))
    out.tio = out.tio.reshape(len(tfs), g.h, g.w, 2)
    if not want_visited:
        del out.visited
    return out


def assert_same(got, exp, case="", pixels=None):
    """bit for bit: the four arrays of VoFOD.map_render against the statement's (on `pixels` only, where given)"""
    rng, vox, what, tio = got
    if pixels is not None:
        nv = what.shape[0]
        cut = lambda a, k: a.reshape(nv, -1, *([2] if k else []))[:, pixels]
        rng, vox, what, tio = cut(rng, 0), cut(vox, 0), cut(what, 0), cut(tio, 1)
        exp = SimpleNamespace(range=cut(exp.range, 0), voxel=cut(exp.voxel, 0), what=cut(exp.what, 0), tio=cut(exp.tio, 1))
    np.testing.assert_array_equal(what, exp.what, err_msg=f"{case}: what")
    np.testing.assert_array_equal(vox, exp.voxel, err_msg=f"{case}: voxel")
    np.testing.assert_array_equal(tio.view(np.uint32), exp.tio.view(np.uint32), err_msg=f"{case}: t_in_out")
    np.testing.assert_array_equal(rng, exp.range, err_msg=f"{case}: range")


# ------------------------------------------------------------------------------------------------ handles and geometry
def make_det(lib, w, h, area_size, vs, dirs, offs=None, area_offset=(0.0, 0.0, 0.0), max_batch=1, **dyn):
    """a detector whose map has ceil(area_size / vs) + 1 voxels per axis (VoxelMap::resize) under the given LUT"""
    sp, dp = default_params(lib)
    sp.voxel_size = vs
    sp.sensor_hrays, sp.sensor_vrays = w, h
    sp.sensor_vfov = F(np.deg2rad(45.0))
    sp.max_batch_frames = max_batch
    for a in range(3):
        sp.oparea_size[a], sp.oparea_offset[a] = area_size[a], area_offset[a]
        sp.exclude_size[a], sp.exclude_offset[a] = 0.0, 0.0
    for k, v in dyn.items():
        setattr(dp, k, v)
    return VoFOD(lib, sp, dp, lut_directions=dirs, lut_offsets=offs)


def geom(det, dirs, offs=None):
    return SimpleNamespace(size=det.map_size, off=np.asarray(det.map_offset, dtype=F), vs=F(det.sp.voxel_size), dirs=np.asarray(dirs, F).reshape(-1, 3),
                           offs=None if offs is None else np.asarray(offs, F).reshape(-1, 3), h=int(det.sp.sensor_vrays), w=int(det.sp.sensor_hrays))


def sim_lut(w, h, vfov_deg=45.0):
    from vofod_amd import synth

    return synth.sim_lut(w, h, float(F(np.deg2rad(vfov_deg))))


def pose(xyz, yaw=0.0, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return np.hstack([R, np.asarray(xyz, dtype=np.float64).reshape(3, 1)]).astype(F)


def voxel_centre(g, ix, iy, iz):
    return np.array([(i + 0.5) * float(g.vs) + float(g.off[a]) for a, i in enumerate((ix, iy, iz))])


def random_map(size, seed, threshold, special=True, frac=0.2):
    """a fifth (`frac`) of the voxels over the threshold; NaN, +inf, -0.0 and threshold-equal values sprinkled in"""
    rng = np.random.default_rng(seed)
    sx, sy, sz = size
    m = rng.uniform(-10.0, float(threshold) - 0.5, size=(sz, sy, sx)).astype(F)
    m[rng.random(m.shape) < frac] = F(threshold) + F(rng.uniform(0.5, 5.0))
    if special:
        flat = m.reshape(-1)
        for val in (np.nan, np.inf, -0.0, threshold, -np.inf):
            flat[rng.integers(0, flat.size, size=max(flat.size // 40, 2))] = F(val)
    return m


# ------------------------------------------------------------------------------------------------ the hand cases
# a 5 x 4 x 3 map at 0.5 m: area (2.0, 1.5, 1.0) at offset 0 -> origin (-1, -0.75, 0); voxel ix spans x in [-1 + 0.5 ix, -0.5 + 0.5 ix]
HAND_AREA, HAND_VS, HAND_SIZE, HAND_OFF = (2.0, 1.5, 1.0), 0.5, (5, 4, 3), (-1.0, -0.75, 0.0)
BG = -1.0  # the map's value elsewhere; threshold 0


def _lin(ix, iy, iz):
    return (iz * 4 + iy) * 5 + ix


def _tf(x, y, z):
    return pose((x, y, z))


def hand_cases():
    """(name, lut direction, tf, {voxel: value}, threshold, max_distance, expected what, voxel, t_in, t_out, range) - every number
    worked out by hand on the grid above; all of them are exact in float32"""
    X, NY, DG, TIE = (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.5, 0.25, 0.0), (0.5, 0.5, 0.0)
    c = []
    # +x from the centre of voxel (0, 1, 0): faces at t = 0.25, 0.75, 1.25, 1.75, 2.25
    c.append(("+x hit", X, _tf(-0.75, 0.0, 0.25), {(3, 1, 0): 1.0}, 0.0, 10.0, HIT, _lin(3, 1, 0), 1.25, 1.75, 1500))
    # -y from the centre of voxel (2, 3, 1): faces at 0.25, 0.75, 1.25, 1.75
    c.append(("-y hit", NY, _tf(0.25, 1.0, 0.75), {(2, 1, 1): 1.0}, 0.0, 10.0, HIT, _lin(2, 1, 1), 0.75, 1.25, 1000))
    # dir (0.5, 0.25, 0) from the centre of (0, 0, 0): tmax = (0.5, 1.0), tdelta = (1, 2): x .5, y 1., x 1.5 -> (2, 1) until x 2.5
    c.append(("diagonal hit", DG, _tf(-0.75, -0.5, 0.25), {(2, 1, 0): 1.0}, 0.0, 10.0, HIT, _lin(2, 1, 0), 1.5, 2.5, 2000))
    # dir (0.5, 0.5, 0) from a centre: tmax x == tmax y == 0.5, the first minimum (x) steps first; (1, 0) is crossed in a piece of length 0
    c.append(("tie: x first", TIE, _tf(-0.75, -0.5, 0.25), {(1, 0, 0): 1.0, (0, 1, 0): 5.0}, 0.0, 10.0, HIT, _lin(1, 0, 0), 0.5, 0.5, 500))
    c.append(("threshold equal is no hit", X, _tf(-0.75, 0.0, 0.25), {(2, 1, 0): 0.5, (4, 1, 0): 0.75}, 0.5, 10.0, HIT, _lin(4, 1, 0), 1.75, 2.25, 2000))
    c.append(("NaN in front of a hit", X, _tf(-0.75, 0.0, 0.25), {(1, 1, 0): np.nan, (2, 1, 0): 1.0}, 0.0, 10.0, HIT, _lin(2, 1, 0), 0.75, 1.25, 1000))
    c.append(("+inf is a hit", X, _tf(-0.75, 0.0, 0.25), {(1, 1, 0): np.inf}, 0.0, 10.0, HIT, _lin(1, 1, 0), 0.25, 0.75, 500))
    # the start voxel itself: [0, 0.25], middle 0.125 m = 125 mm; from 0.0005 m before the face: [0, 0.0005] -> rint(0.25) = 0 -> 1
    c.append(("start voxel is a hit", X, _tf(-0.75, 0.0, 0.25), {(0, 1, 0): 1.0}, 0.0, 10.0, HIT, _lin(0, 1, 0), 0.0, 0.25, 125))
    c.append(("END inside the second voxel", X, _tf(-0.75, 0.0, 0.25), {(3, 1, 0): 1.0}, 0.0, 0.5, END, NO_VOXEL, 0.25, 0.5, 0))
    c.append(("END: length on a face", X, _tf(-0.75, 0.0, 0.25), {}, 0.0, 0.25, END, NO_VOXEL, 0.0, 0.25, 0))
    # LEFT at each of the six faces, from the centre of voxel (2, 1, 1) = (0.25, 0.0, 0.75)
    for name, d, t_in, t_out in (("+x", (1, 0, 0), 0.75, 1.25), ("-x", (-1, 0, 0), 0.75, 1.25), ("+y", (0, 1, 0), 0.75, 1.25), ("-y", (0, -1, 0), 0.25, 0.75),
                                 ("+z", (0, 0, 1), 0.25, 0.75), ("-z", (0, 0, -1), 0.25, 0.75)):
        c.append((f"LEFT at the {name} face", tuple(float(x) for x in d), _tf(0.25, 0.0, 0.75), {}, 0.0, 10.0, LEFT, NO_VOXEL, t_in, t_out, 0))
    # a start exactly on the face x = -0.5: floor((-0.5 + 1) * 2) = 1, the voxel on the far side; its centre is 0.25 ahead: faces at 0.5, 1.0
    c.append(("start on a face", X, _tf(-0.5, 0.0, 0.25), {(1, 1, 0): 1.0}, 0.0, 10.0, HIT, _lin(1, 1, 0), 0.0, 0.5, 250))
    c.append(("start on a face, looking back", (-1.0, 0.0, 0.0), _tf(-0.5, 0.0, 0.25), {(0, 1, 0): 1.0}, 0.0, 10.0, HIT, _lin(0, 1, 0), 0.0, 0.5, 250))
    return c


def hand_map(cells):
    m = np.full((3, 4, 5), BG, dtype=F)
    for (ix, iy, iz), v in cells.items():
        m[iz, iy, ix] = v
    return m


def hand_det(lib, direction, offs=None):
    """the hand map under a 2 x 2 sensor (the smallest a handle takes) whose four pixels carry the one direction"""
    tile = lambda a: None if a is None else np.tile(np.asarray(a, F).reshape(1, 3), (4, 1))
    return make_det(lib, 2, 2, HAND_AREA, HAND_VS, tile(direction), tile(offs))


# ------------------------------------------------------------------------------------------------ decode and scenes
def decode_point(g, tf, range_img):
    """the points of a range image by the RANGE IMAGES definition, transformed with tf in the pipeline's (pcl) association - float32"""
    r = range_img.reshape(-1).astype(F) * F(0.001)
    o = np.zeros_like(g.dirs) if g.offs is None else g.offs
    p = (g.dirs * r[:, None]) + o
    tf = np.asarray(tf, F).reshape(3, 4)
    return np.stack([((tf[k, 0] * p[:, 0]) + (tf[k, 1] * p[:, 1])) + ((tf[k, 2] * p[:, 2]) + tf[k, 3]) for k in range(3)], axis=1)


def cell_of(g, q):
    c = np.floor((q - g.off[None, :]) * (F(1.0) / g.vs)).astype(np.int64)
    sx, sy, sz = g.size
    inside = ((c >= 0) & (c < np.array([sx, sy, sz]))).all(axis=1)
    return np.where(inside, (c[:, 2] * sy + c[:, 1]) * sx + c[:, 0], -1)


# the end-to-end scene: a 41 x 41 x 21 map at 0.5 m under a 64 x 16 sensor with a 90 degree field of view.  A ground slab loaded as
# a-priori points (+inf: above every threshold; it also sets both background latches), every other voxel carved to scores/ray (free
# air the pipeline is sure of), and a floating box of 2 x 2 x 2 voxels at scores/point, 3.3 m in front of the sensor at its height:
# nine of its rays hit the box, the lower rings hit the slab.  With the box erased from the detector's map, the rendered scan shows
# the pipeline a cluster in known-free air, far from any background: one detection, inside the box.
E2E_W, E2E_H, E2E_VFOV, E2E_AREA, E2E_AREA_OFFSET, E2E_VS = 64, 16, 90.0, (20.0, 20.0, 10.0), (0.0, 0.0, -1.0), 0.5
E2E_BOX = (slice(10, 12), slice(24, 26), slice(26, 28))  # [z, y, x]: x in [3, 4], y in [2, 3], z in [4, 5] metres
E2E_BOX_MIN, E2E_BOX_MAX = (3.0, 2.0, 4.0), (4.0, 3.0, 5.0)


def e2e_det(lib):
    dirs = sim_lut(E2E_W, E2E_H, E2E_VFOV)
    det = make_det(lib, E2E_W, E2E_H, E2E_AREA, E2E_VS, dirs, area_offset=E2E_AREA_OFFSET)
    assert det.map_size == (41, 41, 21)
    return det, geom(det, dirs)


def e2e_scene(det, g):
    """(the map with the box, the map without it, the pose); leaves the detector holding the map WITH the box"""
    vs = E2E_VS
    gx, gy = np.meshgrid(np.arange(-10 + vs / 2, 10, vs), np.arange(-10 + vs / 2, 10, vs), indexing="ij")
    det.load_apriori(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -0.8)], axis=1).astype(F))
    m = det.read_map()
    slab = m > F(det.dp.voxel_map__thresholds__new_obstacles)
    assert slab.sum() == 1600 and slab[0].sum() == 1600
    m[~slab] = det.dp.voxel_map__scores__ray
    free = m.copy()
    m[E2E_BOX] = det.dp.voxel_map__scores__point
    det.write_map(capi.MAP_VOXELS, m)
    return m, free, pose(voxel_centre(g, 20, 20, 10))


def points_of_range(g, range_img):
    """the sensor-frame points of a range image by the RANGE IMAGES definition (zeros where there is no return), for an
    implementation that takes point scans only"""
    from vofod_amd.detector import ScanData

    rr = np.ascontiguousarray(range_img, dtype=np.uint32).reshape(-1)
    o = np.zeros_like(g.dirs) if g.offs is None else g.offs
    p = ((g.dirs * (rr.astype(F) * F(0.001))[:, None]) + o).astype(F)
    p[rr == 0] = 0
    return ScanData(x=p[:, 0].copy(), y=p[:, 1].copy(), z=p[:, 2].copy(), width=g.w, height=g.h, intensity=np.full(rr.size, 100.0, F), range=rr.copy())
