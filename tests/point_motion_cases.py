"""Motion-compensated point scans (include/vofod.h, MOTION COMPENSATION OF POINT SCANS): the numpy float32 statement of the definition
that tests/test_gpu_point_motion.py holds k_point_deskew to bit for bit, and the case tables both test modules share.  The statement
is this module's own code; nothing of it comes from the product.

Pixel i = row * width + col was measured in column m = (col + shift_by_row[row]) mod width, T = col_tfs[m], q = (x[i], y[i], z[i]) as
given, and (every operation IEEE float32, each rounded once, nothing fused; the rules in this order)
    p = (+0, +0, +0)                 when q[0] == 0 && q[1] == 0 && q[2] == 0 (either sign of zero)
    p = (qNaN, qNaN, qNaN)           when any q[a] is not finite
    p = (qNaN, qNaN, qNaN)           when lo[a] <= q[a] <= hi[a] on all three axes (the closed exclude box of the first crop)
    p[k] = T[k][0]*q[0] + (T[k][1]*q[1] + (T[k][2]*q[2] + T[k][3]))   otherwise"""
import numpy as np

from vofod_amd import synth

from range_motion_cases import POSES, SHAPES as RANGE_SHAPES, SHIFTS, exclude_bounds, measurement_column  # noqa: F401 (re-exported)

f32 = np.float32
QNAN = np.uint32(0x7FC00000).view(f32)

# (rows, columns, vfov_deg, max range)
SHAPES = {
    "5x20": RANGE_SHAPES["5x20"],      # n = 100: vector variant
    "3x21": RANGE_SHAPES["3x21"],      # n = 63: the scalar variant, less than one wave
    "4x18": RANGE_SHAPES["4x18"],      # quads straddle row ends, a wave spans all four rows
    "3x100": (3, 100, 30.0, 120.0),    # n = 300: a wave of 64 pixels straddles a row end, more than one wave (and, vector, more than one span)
    "2x70": (2, 70, 30.0, 120.0),      # width just over one wave
    "os1_16": synth.SENSORS["os1-16"],
}


def point_definition(x, y, z, col_tfs, width, lo, hi, shift_by_row=None):
    """(x, y, z) float32 of the definition and the mask of the pixels a NaN rule took"""
    q = [np.ascontiguousarray(v, dtype=f32).reshape(-1) for v in (x, y, z)]
    n = q[0].size
    assert n % width == 0 and q[1].size == n and q[2].size == n
    i = np.arange(n, dtype=np.int64)
    m = measurement_column(i // width, i % width, width, shift_by_row)
    T = np.ascontiguousarray(col_tfs, dtype=f32).reshape(width, 3, 4)[m]
    zero = (q[0] == 0) & (q[1] == 0) & (q[2] == 0)
    finite = np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2])
    inside = np.ones(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        for a in range(3):
            inside &= (q[a] >= f32(lo[a])) & (q[a] <= f32(hi[a]))
    nan = ~zero & (~finite | inside)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            t2 = ((T[:, k, 2] * q[2]).astype(f32) + T[:, k, 3]).astype(f32)
            t1 = ((T[:, k, 1] * q[1]).astype(f32) + t2).astype(f32)
            p = ((T[:, k, 0] * q[0]).astype(f32) + t1).astype(f32)
            p = np.where(nan, QNAN, p)
            out.append(np.where(zero, f32(0.0), p).astype(f32))
    return out[0], out[1], out[2], nan


def face_points(lo, hi):
    """24 points around the closed box: for every face one point exactly ON it (inside) and one a float outward (outside), twice over;
    returns ([24, 3] float32, inside mask) - the recipe of range_motion_cases.with_face_pixels on points"""
    lo, hi = np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32)
    mid = ((lo.astype(np.float64) + hi) / 2).astype(f32)
    pts, inside = [], []
    for k in range(24):
        axis, upper, outward = (k // 4) % 3, (k // 2) % 2 == 1, k % 2 == 1
        p = mid.copy()
        face = hi[axis] if upper else lo[axis]
        p[axis] = np.nextafter(face, f32(np.inf if upper else -np.inf), dtype=f32) if outward else face
        pts.append(p)
        inside.append(not outward)
    return np.array(pts, dtype=f32), np.array(inside)


SPECIALS = np.array(
    [[0.0, 0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, -0.0, -0.0], [-0.0, -0.0, -0.0],            # no return, either sign of zero
     [np.nan, 5.0, 1.0], [5.0, np.nan, 1.0], [5.0, 1.0, np.nan], [np.nan, np.nan, np.nan],  # not finite
     [np.inf, 5.0, 1.0], [5.0, -np.inf, 1.0], [5.0, 1.0, np.inf], [-np.inf, np.inf, 0.0],
     [0.0, np.nan, 0.0], [0.0, 0.0, -np.inf],                                               # a zero beside a non-finite coordinate: not "no return"
     [0.0, 0.0, 7.5], [-0.0, 30.0, 0.0]],                                                   # a zero coordinate of a real return
    dtype=f32)


def sample_points(shape, lo, hi, seed=0, near_share=0.2):
    """a cloud of `shape` for the kernel tests: returns out to the sensor's range, a share inside the exclude box, and - scattered over
    the image - SPECIALS and the face points; -> (x, y, z, index of the specials, index of the face points, inside mask of those)"""
    h_, w_ = shape[:2]
    n = h_ * w_
    rs = np.random.default_rng(seed + 23)
    p = rs.uniform(-60.0, 60.0, (n, 3)).astype(f32)
    p[:, 2] = rs.uniform(-3.0, 12.0, n).astype(f32)
    near = rs.random(n) < near_share
    p[near] = (lo + (hi - lo) * rs.random((int(near.sum()), 3))).astype(f32)
    faces, inside = face_points(lo, hi)
    k = min(n, len(SPECIALS) + len(faces))
    at = rs.choice(n, k, replace=False)
    special_at, face_at = at[: min(k, len(SPECIALS))], at[len(SPECIALS):]
    p[special_at] = SPECIALS[: len(special_at)]
    p[face_at] = faces[: len(face_at)]
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), special_at, face_at, inside[: len(face_at)]
