"""The float accumulator of the one raycast walk (k_raycast_t in vofod_amd/csrc/kernels_raycast.h), ray by ray and bit for bit.

The units of the exact pass are held to the oracle one ray at a time (tests/test_gpu_raycast_exact.py); the float pass of a whole scan
can only be held to a tolerance, because the order of its atomics shows in the sums.  A LONE ray has no such freedom: it visits a
voxel once, so every atomic adds one piece onto zero and every merge run has length one - the raycast map after vofod_raycast_begin
IS the float pieces of the walk.  For every pixel above the intensity gate, one pass with only that pixel alive (all others below
the gate, as raycast_exact_cases.single_ray_yardstick does), the exact switch off:
  rigid            the motion switch off                          (launched as k_raycast)
  motion_identity  the motion switch on and the identity table    (launched as k_raycast_motion; d' == d, o' == o as values)
and vofod_read_map(VOFOD_MAP_RAYCAST) equals the oracle's map of the same single-ray pass as uint32 bit patterns.
Shapes 5x20 and 3x21 of range_motion_cases.SHAPES, LUT with beam offsets, 0.5 m voxels, the small operation area."""
import os

import numpy as np
import pytest

from vofod_amd import capi
from vofod_amd.detector import ScanData

import range_motion_cases as rm
import raycast_exact_cases as rx
import raycast_motion_cases as rc
from test_gpu_range_image import LUTS
from test_gpu_stream_route import profiled_calls

pytestmark = pytest.mark.gpu
if os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"):
    pytest.skip("oracle against oracle: the oracle has no profiler names, no motion switch and takes no range images", allow_module_level=True)

f32 = np.float32
SHAPE_NAMES = ("5x20", "3x21")
LUT_KIND = "offsets_28mm_36mm"
MIN_WALKED = 20  # single-ray passes that laid a piece, per shape (the oracle walks 65 / 35 rays of these cases)

_ORACLE = {}


def lone_ray_intensities(c):
    """{pixel: the case's intensities with every other pixel below the gate}, for every pixel above the gate"""
    gate = f32(rc.MIN_INTENSITY)
    out = {}
    for i in np.flatnonzero(c.intensity >= gate):
        it = np.full(c.h * c.w, gate - f32(1.0), dtype=f32)
        it[i] = c.intensity[i]
        out[int(i)] = it
    return out


def lone_ray_pass(det, sd, tf):
    """the raycast map (uint32 bit patterns, flat) of one vofod_raycast_begin; the pass is abandoned"""
    assert det.raycast_begin(sd, tf) == capi.OK
    bits = det.read_map(capi.MAP_RAYCAST).reshape(-1).view(np.uint32).copy()
    assert det.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
    return bits


def oracle_lone_rays(oracle, hip, shape_name):
    """(case, LUT, {pixel: (voxels, bit patterns)} of the oracle's single-ray passes), computed once per shape and shared (read only)"""
    if shape_name not in _ORACLE:
        c = rx.case(shape_name)
        lut = LUTS[LUT_KIND](hip, c.shape)
        z = np.zeros(c.h * c.w, dtype=f32)
        ref = rc.detector(oracle, c.shape, lut, mask=c.mask, vs=rx.VS)
        try:
            want = {}
            for i, it in lone_ray_intensities(c).items():
                bits = lone_ray_pass(ref, ScanData(x=z, y=z, z=z, width=c.w, height=c.h, intensity=it, range=c.range), c.tf)
                at = np.flatnonzero(bits)
                want[i] = (at, bits[at])
        finally:
            ref.close()
        _ORACLE[shape_name] = (c, lut, want)
    return _ORACLE[shape_name]


@pytest.mark.parametrize("variant", ("rigid", "motion_identity"))
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_lone_ray_float_pieces_are_the_oracles_bit_for_bit(oracle, hip, shape_name, variant):
    c, lut, want = oracle_lone_rays(oracle, hip, shape_name)
    n_walked = sum(at.size > 0 for at, _ in want.values())
    print(f"{shape_name}: {len(want)} pixels above the gate, {n_walked} single-ray passes of the oracle laid a piece")
    assert n_walked >= MIN_WALKED
    motion = variant == "motion_identity"
    table = rm.identity_poses(c.w) if motion else None
    dev = rc.detector(hip, c.shape, lut, mask=c.mask, vs=rx.VS)
    try:
        assert dev.set_raycast_motion(motion) == capi.OK
        dev.lib.profile_enable(dev.h, 1)
        n_laid = 0
        for i, it in lone_ray_intensities(c).items():
            got = lone_ray_pass(dev, ScanData.range_image(c.range, c.w, c.h, intensity=it, col_tfs=table), c.tf)
            at, bits = want[i]
            ref_bits = np.zeros_like(got)
            ref_bits[at] = bits
            np.testing.assert_array_equal(got, ref_bits, err_msg=f"{shape_name}/{variant}: pixel {i}")
            n_laid += bool(got.any())
        ran = profiled_calls(dev.lib, dev)
        dev.lib.profile_enable(dev.h, 0)
        assert n_laid >= MIN_WALKED
        mine, other = ("k_raycast_motion", "k_raycast") if motion else ("k_raycast", "k_raycast_motion")
        assert ran.get(mine, 0) == len(want) and other not in ran and "k_raycast_exact" not in ran, ran
    finally:
        dev.close()
