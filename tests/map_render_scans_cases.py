"""vofod_map_render_scans: the numpy statement of include/vofod.h, SCANS AGAINST THE MAP - written from the header's text in float32
with every operation rounded once - and the fixtures test_map_render_scans_cpu.py and test_gpu_map_render_scans.py share.  The beam
is raycast_motion_cases.ray_definition, the front map_render_cases.rays, the walk map_render_cases.walk - imported, not copied; the
verdict and the counts are written out here.  Nothing comes from the product."""
from types import SimpleNamespace

import numpy as np

import map_render_cases as mrc
import raycast_motion_cases as rmc
from vofod_amd import capi
from vofod_amd.detector import VoFOD, default_params

F = np.float32
NOT_CAST, HIT, END, LEFT = mrc.NOT_CAST, mrc.HIT, mrc.END, mrc.LEFT
NONE, AGREES, EMPTY, NEARER, THROUGH, MISSING, BEYOND = range(7)
NAMES = ("NONE", "AGREES", "EMPTY", "NEARER", "THROUGH", "MISSING", "BEYOND")


# ------------------------------------------------------------------------------------------------ the statement
def view_rays(g, tf, col_tfs=None, shift_by_row=None):
    """(dir, start) [n, 3] float32 of every pixel of one view: the rigid ray without a table; with one, d', o' of
    MOTION-COMPENSATED RAYS in place of the LUT entries, then MAP RENDER's front"""
    if col_tfs is None:
        return mrc.rays(tf, g.dirs, g.offs)
    dm, om = rmc.ray_definition(g.dirs, g.offs, col_tfs, g.w, shift_by_row)
    return mrc.rays(tf, dm, om)


def verdict(what, t_in, t_out, r, mask, tol):
    """the header's table, for arrays of one shape: what uint8, t_in / t_out float32, r uint32 millimetres, mask uint8"""
    what, r, mask = np.asarray(what), np.asarray(r, dtype=np.uint32), np.asarray(mask)
    t_in, t_out, tol = np.asarray(t_in, dtype=F), np.asarray(t_out, dtype=F), F(tol)
    rm = (r.astype(F) * F(0.001)).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        near = (rm + tol).astype(F)
        far = (t_out + tol).astype(F)
        hit = np.where(near < t_in, NEARER, np.where(rm > far, THROUGH, AGREES))
        open_ = np.where(near < t_out, NEARER, BEYOND)
    v = np.where(what == HIT, hit, open_)
    v = np.where(r == 0, np.where(what == HIT, MISSING, EMPTY), v)
    v = np.where((r == 0) & (mask == 0), NONE, v)
    v = np.where(what == NOT_CAST, NONE, v)
    return v.astype(np.uint8)


def statement(g, m, scans, tfs, threshold, length, tolerance=0.0, mask=None, shift_by_row=None, render=None, pixels=None):
    """The whole call.  scans: objects with `col_tfs` ([w, 3, 4] float32 or None) and `range` (w * h uint32 in pixel order, or
    None: no verdict for that call).  `render`: an earlier answer for the same views whose walks are taken over, not walked again.
    `pixels`: only these pixel indices are walked, for sensors too large to walk in Python - the others stay NOT_CAST, their
    verdict NONE, and the counts are of no use.  Returns SimpleNamespace(range, voxel, what, tio, verdict, counts) shaped like
    VoFOD.map_render_scans' result (tio: its t_in_out)."""
    tfs = np.asarray(tfs, dtype=F).reshape(-1, 3, 4)
    assert len(tfs) == len(scans)
    nv, n = len(scans), g.h * g.w
    m = np.ascontiguousarray(m, dtype=F)
    mask = np.ones(n, np.uint8) if mask is None else np.asarray(mask, np.uint8).reshape(n)
    out = SimpleNamespace(range=np.zeros((nv, n), np.uint32), voxel=np.full((nv, n), mrc.NO_VOXEL, np.uint32), what=np.zeros((nv, n), np.uint8), tio=np.zeros((nv, n, 2), F),
                          verdict=np.zeros((nv, n), np.uint8), counts=np.zeros((nv, 8), np.uint32))
    compare = all(s.range is not None for s in scans)
    for v, (s, tf) in enumerate(zip(scans, tfs)):
        if render is not None:
            for k in ("range", "voxel", "what", "tio"):
                getattr(out, k)[v] = getattr(render, k)[v].reshape(getattr(out, k)[v].shape)
        dir_, start = (None, None) if render is not None else view_rays(g, tf, s.col_tfs, shift_by_row)
        for i in ([] if render is not None else range(n) if pixels is None else pixels):
            what, vox, t_in, t_out, _ = mrc.walk(start[i], dir_[i], m, g.off, g.vs, threshold, length)
            out.what[v, i], out.voxel[v, i], out.tio[v, i] = what, vox, (t_in, t_out)
            out.range[v, i] = mrc.range_mm(t_in, t_out) if what == HIT else 0
        if compare:
            out.verdict[v] = verdict(out.what[v], out.tio[v, :, 0], out.tio[v, :, 1], np.asarray(s.range, np.uint32).reshape(n), mask, tolerance)
            out.counts[v] = np.bincount(out.verdict[v], minlength=8)
    for k in ("range", "voxel", "what", "verdict"):
        setattr(out, k, getattr(out, k).reshape(nv, g.h, g.w))
    out.tio = out.tio.reshape(nv, g.h, g.w, 2)
    if not compare:
        out.verdict = out.counts = None
    return out


def assert_same(got, exp, case=""):
    """bit for bit: the six arrays of VoFOD.map_render_scans against the statement's"""
    mrc.assert_same((got.range, got.voxel, got.what, got.t_in_out), exp, case)
    if exp.verdict is not None:
        np.testing.assert_array_equal(got.verdict, exp.verdict, err_msg=f"{case}: verdict")
        np.testing.assert_array_equal(got.counts, exp.counts, err_msg=f"{case}: counts")


# ------------------------------------------------------------------------------------------------ handles, tables, measured ranges
def make_det(lib, w, h, area_size, vs, dirs, offs=None, mask=None, max_batch=1, **dyn):
    """map_render_cases.make_det with a mask"""
    sp, dp = default_params(lib)
    sp.voxel_size = vs
    sp.sensor_hrays, sp.sensor_vrays = w, h
    sp.sensor_vfov = F(np.deg2rad(45.0))
    sp.max_batch_frames = max_batch
    for a in range(3):
        sp.oparea_size[a], sp.oparea_offset[a] = area_size[a], 0.0
        sp.exclude_size[a], sp.exclude_offset[a] = 0.0, 0.0
    for k, v in dyn.items():
        setattr(dp, k, v)
    return VoFOD(lib, sp, dp, lut_directions=dirs, lut_offsets=offs, mask=mask)


def sensor_mask(w, h, seed=0):
    """an eighth of the pixels masked out"""
    return (np.random.default_rng(seed + 91).random(w * h) >= 0.125).astype(np.uint8)


def column_shifts(w, h, seed=0):
    """non-zero shifts, negative ones and ones >= width included"""
    sh = np.random.default_rng(seed + 17).integers(-2 * w, 3 * w, h).astype(np.int32)
    sh[0], sh[1], sh[-1] = -1, w + 3, 0
    return sh


def small_table(lib, w, seed=0):
    """a random small rigid table: the sensor moves a few centimetres and turns a few degrees while the scan is taken"""
    from vofod_amd.detector import column_poses

    rs = np.random.default_rng(seed + 5)
    a = mrc.pose(rs.uniform(-0.05, 0.05, 3), yaw=rs.uniform(-0.1, 0.1), pitch=rs.uniform(-0.05, 0.05))
    b = mrc.pose(rs.uniform(-0.05, 0.05, 3), yaw=rs.uniform(-0.1, 0.1), roll=rs.uniform(-0.05, 0.05))
    return column_poses(lib, a, b, mrc.IDENT, w)


def identity_table(w):
    return np.tile(mrc.IDENT[None], (w, 1, 1)).astype(F)


def measured_ranges(render, length, seed=0):
    """The ranges a sensor could have delivered for every view of a statement's own render, so that every verdict occurs: on HIT
    pixels the rendered range itself, one far nearer, one far behind, or no return; on END / LEFT pixels a return below and one
    above the piece's end, or none.  [views, n] uint32."""
    rs = np.random.default_rng(seed + 3)
    nv = render.what.shape[0]
    what, rng = render.what.reshape(nv, -1), render.range.reshape(nv, -1)
    t_out = render.tio.reshape(nv, -1, 2)[..., 1]
    pick = rs.integers(0, 4, what.shape)
    hit = np.select([pick == 0, pick == 1, pick == 2], [rng, np.maximum(rng.astype(np.int64) - 1500, 1), rng.astype(np.int64) + 3000], 0)
    end_mm = np.rint(t_out.astype(np.float64) * 1000.0).astype(np.int64)
    open_ = np.select([pick == 0, pick == 1, pick == 2], [np.maximum(end_mm - 400, 1), end_mm + 700, end_mm + 5], 0)
    return np.where(what == HIT, hit, open_).astype(np.uint32)


def scan_of(rng, w, h, col_tfs=None):
    """a host range image as ScanData, contiguous"""
    from vofod_amd.detector import ScanData

    return ScanData.range_image(np.ascontiguousarray(rng, np.uint32).reshape(-1), w, h, col_tfs=None if col_tfs is None else np.ascontiguousarray(col_tfs, F))


# ------------------------------------------------------------------------------------------------ the shapes of the device tests
# (w, h, area, voxel size, Ouster LUT with beam offsets?): 128 rays - two waves; 140 - a ragged last wave; 264 - a second block of 8 live lanes
SENSORS = {
    "16x8": (16, 8, (4.0, 4.0, 4.0), 0.5, False),    # map 9 x 9 x 9
    "20x7": (20, 7, (5.0, 3.0, 2.0), 0.25, True),    # map 21 x 13 x 9
    "24x11": (24, 11, (5.0, 3.0, 2.0), 0.25, False),  # map 21 x 13 x 9
}
MAP_SIZE = {"16x8": (9, 9, 9), "20x7": (21, 13, 9), "24x11": (21, 13, 9)}
THRESHOLD, LENGTH, TOLERANCE = 0.5, {"16x8": 2.6, "20x7": 1.6, "24x11": 1.6}, 0.05


def lut_of(name, lib=None):
    w, h, _, _, ouster = SENSORS[name]
    if not ouster:
        return mrc.sim_lut(w, h), None
    from vofod_amd.detector import ouster_lut

    dirs, offs = ouster_lut(lib, w, h, np.linspace(360.0, 0.0, w, endpoint=False), np.linspace(20.0, -20.0, h), origin_mm=27.67)
    return dirs, (offs + F(0.01)).astype(F)


def geometry(name, dirs, offs):
    """the geometry of the handle make_det builds for a sensor, without a handle (VoxelMap::resize: ceil(area / vs) + 1 voxels,
    centred on the area's offset in x and y, z from the bottom; map_render_cases.HAND_OFF states the same rule)"""
    w, h, area, vs, _ = SENSORS[name]
    size = tuple(int(np.ceil(a / vs)) + 1 for a in area)
    assert size == MAP_SIZE[name]
    off = np.array([-area[0] / 2.0, -area[1] / 2.0, 0.0], dtype=F)
    return SimpleNamespace(size=size, off=off, vs=F(vs), dirs=np.asarray(dirs, F).reshape(-1, 3), offs=None if offs is None else np.asarray(offs, F).reshape(-1, 3), h=h, w=w)


def view_poses(g, n_views):
    """poses inside the map: the middle, rotated, near corners"""
    sx, sy, sz = g.size
    c = mrc.voxel_centre(g, sx // 2, sy // 2, sz // 2)
    out = [mrc.pose(c), mrc.pose(c + 0.07, yaw=0.7, pitch=-0.4, roll=0.2), mrc.pose(mrc.voxel_centre(g, 1, 1, 1) + 0.03, yaw=0.4)]
    for k, (ix, iy, iz) in enumerate([(x, y, z) for x in (1, sx - 2) for y in (1, sy - 2) for z in (1, sz - 2)]):
        out.append(mrc.pose(mrc.voxel_centre(g, ix, iy, iz) - 0.02, yaw=0.5 * k, pitch=0.1 * k))
    return np.stack(out[:n_views])


def view_tables(lib, w, n_views, seed=0):
    """a table, or None, per view: rigid, quarter turns, a small rigid motion, in turns; [(kind, table)]"""
    out = []
    for v in range(n_views):
        kind = ("rigid", "quarter", "small")[v % 3] if n_views > 1 else "small"
        tab = None if kind == "rigid" else rmc.quarter_table(w, seed + v)[1] if kind == "quarter" else small_table(lib, w, seed + v)
        out.append((kind, None if tab is None else np.ascontiguousarray(tab, F)))
    return out


def device_case(lib, name, n_views, map_kind="random", seed=0):
    """Everything one device case needs but the handle: geometry, map, mask, shifts, poses, tables, measured ranges and the
    statement's answer.  Built once per (sensor, views, map) and left unchanged."""
    w, h, _, _, _ = SENSORS[name]
    dirs, offs = lut_of(name, lib)
    g = geometry(name, dirs, offs)
    m = {"random": lambda: mrc.random_map(g.size, seed + 11, THRESHOLD, frac=0.08), "empty": lambda: np.full(g.size[::-1], -1.0, F), "solid": lambda: np.full(g.size[::-1], 3.0, F)}[map_kind]()
    mask, shifts = sensor_mask(w, h, seed), column_shifts(w, h, seed)
    tfs = view_poses(g, n_views)
    tabs = view_tables(lib, w, n_views, seed)
    bare = [SimpleNamespace(col_tfs=t, range=None) for _, t in tabs]
    render = statement(g, m, bare, tfs, THRESHOLD, LENGTH[name], mask=mask, shift_by_row=shifts)
    ranges = measured_ranges(render, LENGTH[name], seed)
    scans = [SimpleNamespace(col_tfs=t, range=ranges[v]) for v, (_, t) in enumerate(tabs)]
    exp = statement(g, m, scans, tfs, THRESHOLD, LENGTH[name], TOLERANCE, mask, shifts, render=render)
    return SimpleNamespace(name=name, w=w, h=h, dirs=dirs, offs=offs, g=g, m=m, mask=mask, shifts=shifts, tfs=tfs, tabs=tabs, ranges=ranges, scans=scans, exp=exp,
                           threshold=THRESHOLD, length=LENGTH[name], tolerance=TOLERANCE)


_CASES = {}


def shared_case(lib, name, n_views, map_kind="random"):
    """device_case, computed once per process"""
    key = (name, n_views, map_kind)
    if key not in _CASES:
        _CASES[key] = device_case(lib, name, n_views, map_kind)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ the end-to-end scene
# the 24 x 11 sensor in the middle of its 21 x 13 x 9 map at 0.25 m: free air (-1) in front of a wall seven voxels thick (x >= 14).
# BOX_FREE: 2 x 2 x 2 voxels of free air in front of the wall; BOX_WALL: 2 x 2 x 2 voxels of the wall's first two layers.
E2E_NAME, E2E_LENGTH = "24x11", 8.0
BOX_FREE = (slice(4, 6), slice(6, 8), slice(12, 14))  # [z, y, x]
BOX_WALL = (slice(4, 6), slice(6, 8), slice(14, 16))


def _box_voxels(g, box):
    sx, sy, _ = g.size
    return {(z * sy + y) * sx + x for z in range(box[0].start, box[0].stop) for y in range(box[1].start, box[1].stop) for x in range(box[2].start, box[2].stop)}


def e2e_case(kind):
    """kind "added": the scan is rendered from the map WITH a box in the free air, the handle holds the map without it - the returns
    from the box lie in space the map holds free.  kind "erased": the scan is rendered from the map with a box ERASED from the
    wall, the handle holds the whole wall - those returns lie behind the surface the map expects.  Returns (geometry, the handle's
    map, tf, the scan's ranges [h, w], the statement's answer, the pixels whose ray - in the scan's scene or the handle's - meets
    the box)."""
    w, h = SENSORS[E2E_NAME][:2]
    dirs, _ = lut_of(E2E_NAME)
    g = geometry(E2E_NAME, dirs, None)
    base = np.full(g.size[::-1], -1.0, F)
    base[:, :, 14:] = 3.0
    scene = base.copy()
    box = BOX_FREE if kind == "added" else BOX_WALL
    scene[box] = 3.0 if kind == "added" else -1.0
    tf = mrc.pose(mrc.voxel_centre(g, 10, 6, 4) + 0.01)
    seen = mrc.render(g, scene, tf[None], 0.0, E2E_LENGTH)  # what the sensor delivers
    rigid = mrc.render(g, base, tf[None], 0.0, E2E_LENGTH)  # what the handle's map says
    vox = _box_voxels(g, box)
    on_box = np.isin((seen if kind == "added" else rigid).voxel[0], list(vox))
    scan = SimpleNamespace(col_tfs=None, range=seen.range[0].reshape(-1))
    exp = statement(g, base, [scan], tf[None], 0.0, E2E_LENGTH, render=rigid)
    return SimpleNamespace(g=g, dirs=dirs, w=w, h=h, map=base, tf=tf, range=seen.range[0], exp=exp, on_box=on_box)


# ------------------------------------------------------------------------------------------------ the verdict's edges, by hand
def hand_verdicts():
    """(name, tf, {voxel: value}, max_distance, tolerance, four ranges, the four verdicts) on map_render_cases' hand map, +x from the
    centre of voxel (0, 1, 0): a hit in voxel (3, 1, 0) is the piece [1.25, 1.75], a max_distance of 0.5 ends inside [0.25, 0.5].
    125, 250, 1000 and 2000 mm times 0.001f are 0.125, 0.25, 1 and 2 exactly, so the equalities below are equalities."""
    tf, hit = mrc.pose((-0.75, 0.0, 0.25)), {(3, 1, 0): 1.0}
    return [
        ("HIT: rm + tol == t_in is not NEARER, rm == t_out + tol is not THROUGH", tf, hit, 10.0, 0.25, [1000, 999, 2000, 2001], [AGREES, NEARER, AGREES, THROUGH]),
        ("HIT: no return, and the middle of the piece", tf, hit, 10.0, 0.0, [0, 1500, 1249, 1751], [MISSING, AGREES, NEARER, THROUGH]),
        ("END: rm + tol == t_out is not NEARER", tf, hit, 0.5, 0.25, [125, 250, 900, 0], [NEARER, BEYOND, BEYOND, EMPTY]),
        ("LEFT at the +x face", mrc.pose((0.25, 0.0, 0.75)), {}, 10.0, 0.0, [1000, 1300, 0, 1], [NEARER, BEYOND, EMPTY, NEARER]),
    ]
