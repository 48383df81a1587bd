"""The numpy statement of vofod_map_shift (include/vofod.h) and the scenes of its tests (test_map_shift_cpu.py,
test_gpu_map_shift.py).

Statement.  With s = shift_voxels and sizes S, x fastest as everywhere (arrays are [S2, S1, S0]):
    new[iz, iy, ix] = old[iz + s2, iy + s1, ix + s0]   where every i + s lies in [0, S)
    init_bits elsewhere.
Values are 32-bit patterns: the statement works on uint32 views, so +inf, -0.0f and NaN payloads are compared bit for bit.

Scenes.  A vehicle at the +x edge of the default operation area, a ground sheet that reaches beyond the area on every side and one
floating box that appears after the warm-up.  The continuation test shifts the area by SHIFT voxels; its box floats in the strip
100 m < x < 102 m, which the area only covers after the shift.  The hand-over test (no shift) has its box at x = 96.5 m."""
from __future__ import annotations

import numpy as np

from vofod_amd import capi, synth
from vofod_amd.detector import VoFOD, default_params

SENSOR = "os1-16"
VS = 0.5
SHIFT = (4, -2, 0)
N_WARM = 6   # scans of handle A with VOFOD_SCAN_AUTO_RAYCAST: an even count leaves no pass pending
N_CONT = 4   # scans both sides run after the hand-over
DECOY_FROM = 4  # (behind two raycast passes: upright and rolled)
VEHICLE_DIST = 3.0
TARGET_IN_AREA = (96.5, 22.0, 6.0)      # hand-over test: inside the default area (x up to 100 m)
TARGET_IN_NEW_STRIP = (101.0, 21.0, 6.0)  # continuation test: 100 m < x < 102 m exists only after SHIFT
TARGET_SIZE = 0.8


def shift_statement(arr_u32: np.ndarray, s, init_bits: int) -> np.ndarray:
    """arr_u32[S2, S1, S0] shifted by s = (s0, s1, s2) voxels; cells without a source hold init_bits"""
    a = np.asarray(arr_u32)
    assert a.dtype == np.uint32 and a.ndim == 3
    out = np.full_like(a, np.uint32(init_bits))
    dst, src = [], []
    for axis, sa in zip((2, 1, 0), (int(s[0]), int(s[1]), int(s[2]))):  # array axis 2 is x
        n = a.shape[axis]
        lo, hi = max(0, -sa), min(n, n - sa)  # destination indices i with 0 <= i + sa < n
        if hi <= lo:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo + sa, hi + sa))
    out[dst[2], dst[1], dst[0]] = a[src[2], src[1], src[0]]
    return out


def init_bits(det: VoFOD, which: int) -> int:
    v = np.float32(det.sp.score_init if which == capi.MAP_VOXELS else 0.0)
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def shifted_offset(offset, s, vs: float):
    """base + k * voxel_size from the integer k, rounded once (include/vofod.h: such offsets do not drift)"""
    return tuple(float(np.float32(float(o) + int(k) * float(vs))) for o, k in zip(offset, s))


def make_det(lib, sensor=SENSOR, voxel_size=VS, oparea_offset=None, oparea_size=None, max_batch=1, **dyn) -> VoFOD:
    """one detector with helpers.make_pair's parameters, optionally at another operation area"""
    h, w, vfov_deg, _ = synth.SENSORS[sensor]
    sp, dp = default_params(lib)
    sp.voxel_size = voxel_size
    sp.sensor_hrays, sp.sensor_vrays = w, h
    sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
    sp.max_batch_frames = max_batch
    for a in range(3):
        if oparea_offset is not None:
            sp.oparea_offset[a] = oparea_offset[a]
        if oparea_size is not None:
            sp.oparea_size[a] = oparea_size[a]
    for k, v in dyn.items():
        setattr(dp, k, v)
    return VoFOD(lib, sp, dp)


def random_bits(rng, shape) -> np.ndarray:
    """random 32-bit patterns with +inf, -inf, -0.0f, +0.0f and NaNs (payloads included) sprinkled in"""
    a = rng.integers(0, 2**32, size=shape, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7FC01234, 0xFFC00001, 0x7F800001], dtype=np.uint32)
    pick = rng.random(shape) < 0.2
    a[pick] = special[rng.integers(0, len(special), size=int(pick.sum()))]
    return a


def read_bits(det: VoFOD, which: int) -> np.ndarray:
    return det.read_map(which).view(np.uint32)


def write_bits(det: VoFOD, which: int, bits: np.ndarray):
    det.write_map(which, np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32))


MAPS = (capi.MAP_VOXELS, capi.MAP_FLAGS, capi.MAP_RAYCAST)


def status_tuple(det: VoFOD):
    s = det.status()
    return (s.detection_its, s.last_detection_id, s.background_pts_sufficient, s.sure_background_sufficient, s.raycast_pending, tuple(s.map_size),
            tuple(np.array(list(s.map_offset), dtype=np.float32).view(np.uint32).tolist()))


# ---------------------------------------------------------------------------- the continuation scene

def _box(c):
    h = TARGET_SIZE / 2
    return [c[0] - h, c[1] - h, c[2] - h, c[0] + h, c[1] + h, c[2] + h]


def scene(target, k: int) -> synth.Scene:
    """The world at scan k: a ground sheet beyond the area on every side (default area and the shifted one); from scan
    DECOY_FROM on a floating box behind the vehicle, inside the area - its detections during the warm-up move handle A's detection
    ids ahead of a fresh handle's; from scan N_WARM on the box at `target` in front of the vehicle."""
    boxes = np.zeros((0, 6))
    if k >= DECOY_FROM:
        boxes = np.vstack([boxes, _box((target[0] - 2 * VEHICLE_DIST, target[1], target[2]))])
    if k >= N_WARM:
        boxes = np.vstack([boxes, _box(target)])
    return synth.Scene((-30.0, 110.0, -40.0, 80.0), boxes, 0, 0)


def pose(k: int, target) -> np.ndarray:
    """The vehicle hovers VEHICLE_DIST in front of where the box appears, at its height.  16 rings leave a voxel enough ray length
    to become sure air in ONE raycast pass only at this range, where they span +-1 m: the passes (a pass takes the scan it begins
    with, every other one) alternate between the sensor upright - rings around the box's level - and rolled by 90 degrees - rings
    in the vertical plane through the box.  Together they clear every face neighbour of the box's voxels but the pocket right
    behind it, so that exploreToGround finds the box floating (vofod_nodelet.cpp:1648-1730)."""
    roll = (0.0, np.pi / 2)[(k // 2) % 2]
    yaw = 0.02 * (k % 2)
    rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(roll), -np.sin(roll)], [0, np.sin(roll), np.cos(roll)]])
    tf = np.zeros((3, 4), dtype=np.float64)
    tf[:, :3] = rz @ rx
    tf[:, 3] = (target[0] - VEHICLE_DIST, target[1], target[2])
    return tf.astype(np.float32)


def scans(target, first: int, n: int):
    """scans `first` .. `first + n - 1` of the sequence around `target`"""
    return [synth.make_scan(scene(target, k), pose(k, target), SENSOR, seed=500 + k) for k in range(first, first + n)]


def ground_apriori(vs: float = VS) -> np.ndarray:
    """the ground sheet inside the default area as a-priori points (sets both latches)"""
    gx, gy = np.meshgrid(np.arange(-20 + vs / 2, 100, vs), np.arange(-30 + vs / 2, 70, vs), indexing="ij")
    return np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, vs * 0.25)], axis=1).astype(np.float32)


def warm(det: VoFOD, target):
    """handle A: the ground plane, then N_WARM scans before the box at `target` appears, with the raycast role interleaved"""
    det.load_apriori(ground_apriori())
    out = []
    for s in scans(target, 0, N_WARM):
        out.append(det.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST))
    assert not det.status().raycast_pending
    return out


def continuation_scans(target):
    """the N_CONT scans after the hand-over: the box has appeared"""
    return scans(target, N_WARM, N_CONT)


def hand_over(lib, src_maps, oparea_offset=None, **kw) -> VoFOD:
    """handle B: fresh, the three maps through write_map, the latches through load_apriori with zero points"""
    b = make_det(lib, oparea_offset=oparea_offset, **kw)
    for which in MAPS:
        b.write_map(which, src_maps[which])
    b.load_apriori(np.zeros((0, 3), dtype=np.float32))
    return b


def assert_detections_equal_mod_id(a, b, id_shift: int):
    """helpers.assert_detections_equal with b's ids ahead of a's by one constant"""
    from helpers import assert_detections_equal

    b2 = b.copy()
    b2["id"] = (b2["id"].astype(np.int64) - id_shift).astype(np.uint32)
    assert_detections_equal(a, b2)
