"""Exact raycast accumulation (include/vofod.h, EXACT RAYCAST ACCUMULATION): what tests/test_raycast_exact_cpu.py and
tests/test_gpu_raycast_exact.py share.  Nothing here comes from the product.

  scale_rule            S and QMAX of a handle, the rule of the header restated in Python integers and doubles
  units_of              q = min(rint(piece * 2^S), QMAX) in numpy integers
  single_ray_yardstick  the oracle, one ray at a time: with every pixel but i below the intensity gate the oracle's raycast_begin
                        leaves exactly the float pieces of ray i in its map (a ray visits a voxel once: nothing is summed), the pass is
                        abandoned (raycast_finish returns VOFOD_ERR_RAYCAST_NO_DETECTION);  U_want = the sum over i of units_of(pieces)
                        and c_v = the number of pieces per voxel.  Each ray may be cast under a pose of its own (the quarter-turn
                        tables of raycast_motion_cases: tf o T_k is exact)."""
from types import SimpleNamespace

import numpy as np

from vofod_amd import capi
from vofod_amd.detector import ScanData

import range_motion_cases as rm
import raycast_motion_cases as rc

f32 = np.float32
SHAPE_NAMES = ("5x20", "3x21", "os1_16")
VS = 0.5
# the S the header lists (sensor rows, columns, voxel size) -> S
S_TABLE = {(128, 1024, 0.25): 15, (128, 1024, 0.5): 14, (128, 2048, 0.1): 16, (16, 1024, 0.5): 17, (5, 20, 0.5): 24, (3, 21, 0.5): 24}


def scale_rule(n_pixels, voxel_size):
    """(S, QMAX): S the largest integer in [0, 24] with n_pixels * (floor(2 * vs * 2^S) + 1) <= 2^32 - 1, vs the float voxel size
    widened to double; QMAX = floor(2 * vs * 2^S).  The comparison is made in Python integers (exact: floor of a double is one)."""
    vs = float(f32(voxel_size))
    for s in range(24, -1, -1):
        q = int(np.floor(2.0 * vs * float(2 ** s)))
        if int(n_pixels) * (q + 1) <= 2 ** 32 - 1:
            return s, q
    raise ValueError("no S fits")


def units_of(pieces, s, qmax):
    """q of float32 pieces, int64: the product with 2^S is exact in double, np.rint rounds to nearest, ties to even"""
    p = np.asarray(pieces, dtype=f32).astype(np.float64) * float(2 ** s)
    return np.minimum(np.rint(p).astype(np.int64), int(qmax))


def float_view(units, s):
    """r = float32(U) * 2^-S: numpy's uint32 -> float32 conversion rounds to nearest even, the scaling is exact"""
    return (np.asarray(units, dtype=np.uint32).astype(f32) * f32(2.0 ** -s)).astype(f32)


def case(shape_name):
    """small_case of raycast_motion_cases for the shape (its masks and gates); on OS1-16 only rows 3 and 11 stay above the intensity
    gate: 2 x 1024 consecutive pixels - full waves and long merge runs - and few enough rays for the yardstick"""
    shape = rm.SHAPES[shape_name]
    h, w = shape[:2]
    c = rc.small_case(shape, seed=h * w + 3)
    if shape_name == "os1_16":
        keep = np.zeros(h * w, dtype=bool)
        keep[3 * w:4 * w] = keep[11 * w:12 * w] = True
        c.intensity = np.where(keep, c.intensity, f32(0.0)).astype(f32)
    c.shape, c.h, c.w = shape, h, w
    return c


def _scan(width, height, intensity, range_mm):
    z = np.zeros(width * height, dtype=f32)
    return ScanData(x=z, y=z, z=z, width=width, height=height, intensity=np.ascontiguousarray(intensity, dtype=f32), range=np.ascontiguousarray(range_mm, dtype=np.uint32))


def single_ray_yardstick(ref, c, pixels=None, tf_of_pixel=None):
    """`ref`: an oracle detector with the LUT, mask and parameters of the pass; `c`: a case.  Returns U (int64, flat), the per-voxel
    piece counts, the number of rays that laid a piece, the number of pieces of zero units, S and QMAX.  `pixels`: the rays of the
    pass (default: every pixel above the intensity gate); `tf_of_pixel(i)`: the pose ray i is cast under (default c.tf)."""
    n = c.h * c.w
    s, qmax = scale_rule(n, ref.sp.voxel_size)
    gate = f32(ref.dp.raycast__min_intensity)
    below = gate - f32(1.0)
    if pixels is None:
        pixels = np.flatnonzero(c.intensity >= gate)
    units = np.zeros(ref.n_voxels, dtype=np.int64)
    count = np.zeros(ref.n_voxels, dtype=np.int64)
    walked = zero_pieces = 0
    for i in pixels:
        assert c.intensity[i] >= gate
        it = np.full(n, below, dtype=f32)
        it[i] = c.intensity[i]
        assert ref.raycast_begin(_scan(c.w, c.h, it, c.range), c.tf if tf_of_pixel is None else tf_of_pixel(int(i))) == capi.OK
        pieces = ref.read_map(capi.MAP_RAYCAST).reshape(-1)
        assert ref.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
        at = np.flatnonzero(pieces)
        if at.size == 0:
            continue
        walked += 1
        q = units_of(pieces[at], s, qmax)
        zero_pieces += int((q == 0).sum())
        units[at] += q
        count[at] += q != 0
    assert units.max() <= 2 ** 32 - 1
    return SimpleNamespace(units=units, count=count, walked=walked, zero_pieces=zero_pieces, s=s, qmax=qmax)


def full_pass(ref, c, pixels=None):
    """the oracle's float pass over the same rays (float64, flat)"""
    it = c.intensity
    if pixels is not None:
        it = np.full(c.h * c.w, f32(ref.dp.raycast__min_intensity) - f32(1.0), dtype=f32)
        it[pixels] = c.intensity[pixels]
    assert ref.raycast_begin(_scan(c.w, c.h, it, c.range), c.tf) == capi.OK
    got = ref.read_map(capi.MAP_RAYCAST).astype(np.float64).reshape(-1)
    assert ref.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
    return got


def view_bound(y, want):
    """|U * 2^-S - float pass| <= c_v * 2^-(S+1) (one rounding of q per piece) + 2e-5 |want| + 2e-6 (the float pass's own summation, the
    raycast tolerance of the suite)"""
    return y.count * 2.0 ** -(y.s + 1) + 2e-5 * np.abs(want) + 2e-6


_CACHE = {}


def yardstick(oracle, shape_name, lut_kind, lut):
    """the rigid yardstick of a shape and LUT, computed once per process and shared (read only)"""
    key = (shape_name, lut_kind)
    if key not in _CACHE:
        c = case(shape_name)
        ref = rc.detector(oracle, c.shape, lut, mask=c.mask, vs=VS)
        try:
            y = single_ray_yardstick(ref, c)
            y.full = full_pass(ref, c)
        finally:
            ref.close()
        y.units.setflags(write=False)
        y.count.setflags(write=False)
        y.full.setflags(write=False)
        _CACHE[key] = (c, y)
    return _CACHE[key]
