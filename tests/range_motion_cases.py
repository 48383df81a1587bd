"""Motion-compensated range images (include/vofod.h, MOTION COMPENSATION): the numpy float32 statement of the definition that
tests/test_gpu_range_motion.py holds k_range_decode_motion to bit for bit, and the case tables both test modules share.  The
statement is this module's own code; nothing of it comes from the product.

Pixel i = row * width + col was measured in column m = (col + shift_by_row[row]) mod width, and (every operation IEEE float32,
each rounded once, nothing fused)
    r = float(range[i]) * 0.001f;   q[a] = (lut_directions[3i+a] * r) + lut_offsets[3i+a]
    p = (+0, +0, +0)                 when range[i] == 0
    p = (qNaN, qNaN, qNaN)           when lo[a] <= q[a] <= hi[a] on all three axes (the exclude box as the first crop takes it)
    p[k] = T[k][0]*q[0] + (T[k][1]*q[1] + (T[k][2]*q[2] + T[k][3]))   otherwise, T = col_tfs[m]"""
import numpy as np

from vofod_amd import synth

f32 = np.float32
QNAN = np.uint32(0x7FC00000).view(f32)

# ------------------------------------------------------------------------------------------------ the definition, in numpy


def exclude_bounds(sp):
    """(lo, hi) float32 of the closed exclude box in the expressions of the first crop (vofod_nodelet.cpp:204, :626-629): the yaml's
    z offset is the bottom of the box; as tests/statements.py states them"""
    o, sz = np.array(list(sp.exclude_offset), dtype=f32), np.array(list(sp.exclude_size), dtype=f32)
    c = o.copy()
    c[2] = o[2] + sz[2] / f32(2)
    return (c - sz / f32(2)).astype(f32), (c + sz / f32(2)).astype(f32)


def measurement_column(row, col, width, shift_by_row=None):
    """m of the definition for integer arrays / scalars: the mathematical mod, in Python's unbounded integers"""
    row, col = np.asarray(row, dtype=object), np.asarray(col, dtype=object)
    sh = 0 if shift_by_row is None else np.asarray([int(v) for v in shift_by_row], dtype=object)[row.astype(np.int64)]
    return np.asarray((col + sh) % int(width), dtype=object).astype(np.int64)


def beam_points(range_mm, lut_directions, lut_offsets=None):
    """q of the definition: the decode WITHOUT the zero rule (tests/test_range_image_cpu.py: decode_definition applies it)"""
    rng = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
    d = np.ascontiguousarray(lut_directions, dtype=f32).reshape(-1, 3)
    o = np.zeros_like(d) if lut_offsets is None else np.ascontiguousarray(lut_offsets, dtype=f32).reshape(-1, 3)
    r = (rng.astype(f32) * f32(0.001)).astype(f32)
    return [((d[:, a] * r).astype(f32) + o[:, a]).astype(f32) for a in range(3)]


def motion_definition(range_mm, lut_directions, lut_offsets, col_tfs, width, lo, hi, shift_by_row=None):
    """(x, y, z) float32 and the mask of the pixels the NaN rule took"""
    rng = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
    n = rng.size
    assert n % width == 0
    q = beam_points(rng, lut_directions, lut_offsets)
    i = np.arange(n, dtype=np.int64)
    m = measurement_column(i // width, i % width, width, shift_by_row)
    T = np.ascontiguousarray(col_tfs, dtype=f32).reshape(width, 3, 4)[m]
    inside = np.ones(n, dtype=bool)
    for a in range(3):
        inside &= (q[a] >= f32(lo[a])) & (q[a] <= f32(hi[a]))
    inside &= rng != 0
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            t2 = ((T[:, k, 2] * q[2]).astype(f32) + T[:, k, 3]).astype(f32)
            t1 = ((T[:, k, 1] * q[1]).astype(f32) + t2).astype(f32)
            p = ((T[:, k, 0] * q[0]).astype(f32) + t1).astype(f32)
            p = np.where(inside, QNAN, p)
            out.append(np.where(rng == 0, f32(0.0), p).astype(f32))
    return out[0], out[1], out[2], inside


# ------------------------------------------------------------------------------------------------ case tables
# (rows, columns, vfov_deg, max range): the shapes of the issue
SHAPES = {
    "5x20": (5, 20, 30.0, 120.0),      # n = 100: vector variant, quads inside rows
    "3x21": (3, 21, 30.0, 120.0),      # n = 63: the scalar variant
    "4x18": (4, 18, 30.0, 120.0),      # n = 72, n % 4 == 0 but 18 % 4 != 0: quads straddle row ends
    "os1_16": synth.SENSORS["os1-16"],
    "os1_128": synth.SENSORS["os1-128"],
}


def identity_poses(width):
    return np.tile(np.eye(3, 4, dtype=f32), (width, 1, 1))


def general_poses(width, seed=0):
    """random 3x4 matrices, NOT orthonormal and not symmetric: a transposed or a column-major read gives other numbers"""
    return np.random.default_rng(seed + 11).uniform(-2.0, 2.0, (width, 3, 4)).astype(f32)


def rigid_poses(width, seed=0, yaw_rate=1.0, v=(3.0, 0.0, 0.0), period=0.1):
    """a constant twist over one period, the last column being the reference: col_tfs[m] = exp((m / (w - 1) - 1) * period * twist)"""
    rng = np.random.default_rng(seed + 13)
    axis = rng.normal(size=3) * 0.1 + np.array([0.0, 0.0, 1.0])
    axis /= np.linalg.norm(axis)
    out = np.zeros((width, 3, 4))
    for m in range(width):
        s = (m / max(width - 1, 1) - 1.0) * period
        out[m, :, :3] = rotvec_matrix(axis * yaw_rate * s)
        out[m, :, 3] = np.asarray(v) * s
    return out.astype(f32)


def rotvec_matrix(w):
    """Rodrigues, double"""
    w = np.asarray(w, dtype=np.float64)
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if a < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / (a * a) * (K @ K)


POSES = {"general": general_poses, "rigid": rigid_poses, "identity": lambda w, seed=0: identity_poses(w)}


def shifts(kind, height, width, seed=0):
    if kind == "none":
        return None
    if kind == "all_width":
        return np.full(height, width, dtype=np.int32)
    return np.random.default_rng(seed + 17).integers(-3 * width, 3 * width + 1, height).astype(np.int32)


SHIFTS = ("none", "all_width", "random")


def near_ranges(range_mm, share=0.2, seed=0):
    """a share of the returns pulled in to 300..1 200 mm: inside the default exclude box (2.5 x 2.5 x 1.6 m around the sensor)"""
    rng = np.random.default_rng(seed + 19)
    r = np.array(range_mm, dtype=np.uint32)
    at = rng.random(r.size) < share
    r[at] = rng.integers(300, 1201, int(at.sum())).astype(np.uint32)
    return r


def with_face_pixels(lut, lo, hi, pixels):
    """LUT copy whose `pixels` have zero direction and an offset exactly ON a face of the box (even entries: inside, the box is
    closed) or one float outward of it (odd entries: outside); returns (directions, offsets, inside mask over `pixels`)"""
    d = np.array(lut[0], dtype=f32).reshape(-1, 3).copy()
    o = np.zeros_like(d) if lut[1] is None else np.array(lut[1], dtype=f32).reshape(-1, 3).copy()
    mid = ((lo.astype(np.float64) + hi) / 2).astype(f32)
    inside = []
    for k, px in enumerate(pixels):
        axis, upper, outward = (k // 4) % 3, (k // 2) % 2 == 1, k % 2 == 1
        p = mid.copy()
        face = hi[axis] if upper else lo[axis]
        p[axis] = np.nextafter(face, f32(np.inf if upper else -np.inf), dtype=f32) if outward else face
        d[px], o[px] = 0.0, p
        inside.append(not outward)
    return d, o, np.array(inside)


# ------------------------------------------------------------------------------------------------ the moving sensor of the issue's table
def twist_col_tfs(width, yaw_rate, v, period=0.1):
    """the sensor moves at a constant twist (body frame: yaw rate about z, velocity v) during the scan; the reference frame is the
    pose at the LAST column: col_tfs[m] = exp(-(1 - m / (w - 1)) * period * twist), double -> float32"""
    out = np.zeros((width, 3, 4))
    v = np.asarray(v, dtype=np.float64)
    for m in range(width):
        s = -(1.0 - m / (width - 1)) * period
        th = yaw_rate * s
        R = rotvec_matrix([0.0, 0.0, th])
        if abs(th) < 1e-12:
            V = np.eye(3)
        else:
            K = np.array([[0, -1.0, 0], [1.0, 0, 0], [0, 0, 0]])
            V = np.eye(3) + (1 - np.cos(th)) / th * K + (th - np.sin(th)) / th * (K @ K)
        out[m, :, :3] = R
        out[m, :, 3] = V @ (v * s)
    return out.astype(f32)


def table_shift(height):
    return (7 * np.arange(height) - 40).astype(np.int32)


def warm(dets, warm_scene, sensor_xy=(0.0, 0.0), shape=synth.SENSORS["os1-16"], n_scans=2, seed0=900):
    """the warm-up recipe of tests/test_gpu_frame_inputs.py (warm_both) for any number of detectors: surveyed background, the ground
    patch below the sensor, map-updating scans of the scene without targets, then every voxel still unknown becomes sure air"""
    from vofod_amd import capi

    ap = synth.apriori_points(warm_scene, float(dets[0].sp.voxel_size))
    for d in dets:
        d.load_apriori(ap)
        synth.seed_ground(d, xy=sensor_xy)
    for k in range(n_scans):
        s = synth.make_scan(warm_scene, synth.make_pose(seed0 + k, xy=sensor_xy), shape, seed=seed0 + k)
        for d in dets:
            d.process_scan(s.scan, s.tf)
    for d in dets:
        m = d.read_map(capi.MAP_VOXELS)
        m[m == f32(d.sp.score_init)] = f32(d.dp.voxel_map__thresholds__frontiers)
        d.write_map(capi.MAP_VOXELS, m)
    st = dets[0].status()
    assert st.background_pts_sufficient and st.sure_background_sufficient


DEFAULT_AREA = ((40.0, 20.0, -1.25), (120.0, 100.0, 25.0))


def moving_frames(n=4, yaw_rate=1.0, v=(3.0, 0.0, 0.0), shape=synth.SENSORS["os1-16"], scene_seed=3, seed0=40, n_targets=6):
    """the set-up of the issue's table: (warm scene, scene, frames, col_tfs, shift); frame k is seen from make_pose(seed0 + k) at its
    LAST column while the sensor moves at the twist, its rays cast one by one from the moving pose"""
    warm_scene = synth.make_scene(scene_seed, *DEFAULT_AREA, n_targets=0, sensor_xy=(0.0, 0.0))
    scene = synth.make_scene(scene_seed, *DEFAULT_AREA, n_targets=n_targets, sensor_xy=(0.0, 0.0))
    h, w = shape[:2]
    col_tfs = twist_col_tfs(w, yaw_rate, v)
    shift = table_shift(h)
    frames = [synth.make_moving_scan(scene, synth.make_pose(seed0 + k), col_tfs, shape, col_shift=shift, seed=seed0 + k) for k in range(n)]
    return warm_scene, scene, frames, col_tfs, shift


def target_centres(scene):
    b = scene.boxes[scene.n_static:]
    return (b[:, :3] + b[:, 3:]) / 2


def off_target(dets, scene, radius=0.6):
    """per detection: farther than `radius` from every target box's centre"""
    if len(dets) == 0:
        return np.zeros(0, dtype=bool)
    d = np.linalg.norm(np.asarray(dets["position"])[:, None, :] - target_centres(scene)[None, :, :], axis=2)
    return d.min(axis=1) > radius
