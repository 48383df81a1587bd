"""Range images (include/vofod.h: a vofod_scan with x == y == z == NULL) - what needs no GPU: the declared surface, the Python
mirror, the oracle's refusal, and the numpy float32 statement of the definition that tests/test_gpu_range_image.py holds
k_range_decode to bit for bit.  The statement is this module's own code; nothing of it comes from the product.

Per pixel i (every operation IEEE float32, each rounded once, nothing fused):
    r = float(range[i]) * 0.001f;   p[a] = (lut_directions[3i+a] * r) + lut_offsets[3i+a];   p = (+0, +0, +0) when range[i] == 0
It is held here to the three things it has to agree with: synth.make_scan under the simulated LUT (bit for bit), and the sensor
model of check_sensor_params (vofod_nodelet.cpp:1869-1917, the oracle's) under a LUT with beam offsets and under a
vofod_ouster_lut one."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from vofod_amd import capi, synth
from vofod_amd.detector import ScanData, VoFOD, check_sensor_params, default_params, ouster_lut

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the definition, in numpy
def decode_definition(range_mm, lut_directions, lut_offsets=None):
    """(x, y, z) float32 of a range image under the LUT; every intermediate is rounded to float32 once"""
    rng = np.ascontiguousarray(range_mm, dtype=np.uint32).reshape(-1)
    d = np.ascontiguousarray(lut_directions, dtype=f32).reshape(-1, 3)
    o = np.zeros_like(d) if lut_offsets is None else np.ascontiguousarray(lut_offsets, dtype=f32).reshape(-1, 3)
    r = (rng.astype(f32) * f32(0.001)).astype(f32)  # uint32 -> float32 is round-to-nearest-even in numpy as in v_cvt_f32_u32
    out = []
    for a in range(3):
        prod = (d[:, a] * r).astype(f32)
        p = (prod + o[:, a]).astype(f32)
        out.append(np.where(rng == 0, f32(0.0), p).astype(f32))
    return tuple(out)


def sim_directions(sensor):
    h, w, vfov_deg, _ = synth.SENSORS[sensor] if isinstance(sensor, str) else sensor
    return synth.sim_lut(w, h, float(f32(np.deg2rad(vfov_deg))))


def offset_lut(sensor):
    """the simulated directions with beam offsets of an Ouster's size: ~28 mm radially (along the beam's horizontal direction)
    and ~36 mm up"""
    d = sim_directions(sensor)
    horiz = d[:, :2] / np.maximum(np.linalg.norm(d[:, :2].astype(np.float64), axis=1, keepdims=True), 1e-9)
    o = np.concatenate([0.028 * horiz, np.full((d.shape[0], 1), 0.036)], axis=1).astype(f32)
    return d, o


def ouster_style_lut(lib, sensor, seed=2024):
    """a vofod_ouster_lut one: per-beam azimuth offsets, beam origin 15.806 mm off the axis, the OS1's lidar -> sensor transform"""
    h, w, vfov_deg, _ = synth.SENSORS[sensor] if isinstance(sensor, str) else sensor
    rng = np.random.default_rng(seed)
    altitude = np.linspace(vfov_deg / 2, -vfov_deg / 2, h)
    azimuth = rng.uniform(-3.2, 3.2, h)
    tf = np.eye(4)
    tf[:3, :3] = [[-1, 0, 0], [0, -1, 0], [0, 0, 1]]
    tf[:3, 3] = [0.0, 0.0, 36.18]
    return ouster_lut(lib, w, h, azimuth, altitude, origin_mm=15.806, tf=tf)


def sample_ranges(n, seed=0):
    """uint32 millimetres: plausible returns, pixels without one, and the ends of the conversion (1, 2^24 + 1: the first integer
    float32 cannot hold - a tie, rounded to even -, 0xFFFFFFFF: rounds up to 2^32)"""
    rng = np.random.default_rng(seed)
    r = rng.integers(300, 120_000, n).astype(np.uint32)
    r[rng.random(n) < 0.15] = 0
    special = np.array([0, 1, 2**24 + 1, 0xFFFFFFFF, 2**24 + 3, 2**31 + 129], dtype=np.uint32)
    at = rng.choice(n, 4 * special.size, replace=False)
    r[at] = np.tile(special, 4)
    return r



# ------------------------------------------------------------------------------------------------ surface
def test_header_declares_range_to_points_and_the_mirror_matches():
    names = capi.declared_entry_points()
    assert "range_to_points" in names
    assert set(names) == set(capi._SIGS)
    assert "range_to_points" in capi.PRODUCT_ONLY
    res, args = capi._SIGS["range_to_points"]
    assert res is C.c_int and len(args) == 6  # (handle, scan, x, y, z, out_memspace)
    text = capi.HEADER.read_text()
    assert "int vofod_range_to_points(vofod_handle* h, const vofod_scan* scan, float* x, float* y, float* z, int32_t out_memspace);" in text


def test_hip_library_exports_range_to_points():
    so = ROOT / "vofod_amd" / "csrc" / "libvofod_hip.so"
    if not so.exists():  # hipcc cross-compiles gfx950 without a GPU
        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    lib = capi.Library(so, "vofod_")
    assert hasattr(lib, "range_to_points")
    assert lib.range_to_points.argtypes == capi._SIGS["range_to_points"][1]


def test_range_image_scan_has_null_point_columns():
    r = np.arange(16 * 1024, dtype=np.uint32)
    it = np.ones(r.size, dtype=f32)
    sd = ScanData.range_image(r, 1024, 16, intensity=it, stamp=1.5)
    c = sd.as_c()
    assert c.x is None and c.y is None and c.z is None
    assert c.range == r.ctypes.data and c.intensity == it.ctypes.data
    assert (c.stride_bytes, c.width, c.height, c.memspace, c.stamp) == (4, 1024, 16, capi.MEM_HOST, 1.5)
    dev = ScanData.range_image(0x7F0000001000, 1024, 16, stride_bytes=48, memspace=capi.MEM_DEVICE).as_c()
    assert dev.range == 0x7F0000001000 and dev.intensity is None and dev.stride_bytes == 48 and dev.memspace == capi.MEM_DEVICE


def test_oracle_keeps_rejecting_range_only_scans(oracle):
    """the oracle has no range input (it is not touched): VOFOD_ERR_INVALID_ARG, and no vofod_oracle_range_to_points"""
    sp, dp = default_params(oracle)
    sp.sensor_hrays, sp.sensor_vrays = 1024, 16
    det = VoFOD(oracle, sp, dp)
    s = synth.make_scan(synth.make_scene(4, n_targets=1), synth.make_pose(1), "os1-16", seed=1)
    sd = ScanData.range_image(s.range, 1024, 16, intensity=s.intensity)
    cs = sd.as_c()
    tfa = np.ascontiguousarray(s.tf, dtype=f32).reshape(12)
    n_out = C.c_size_t(0)
    dets = np.zeros(4, dtype=capi.DETECTION)
    assert oracle.process_scan(det.h, C.byref(cs), capi.ptr(tfa), 0, capi.ptr(dets), 4, C.byref(n_out), None) == capi.ERR_INVALID_ARG
    assert not hasattr(oracle, "range_to_points")


# ------------------------------------------------------------------------------------------------ the definition
def test_definition_is_bit_equal_to_synth_under_the_simulated_lut():
    for sensor, seed in (("os1-16", 3), ("os1-128", 5)):
        s = synth.make_scan(synth.make_scene(seed, n_targets=3), synth.make_pose(seed), sensor, seed=seed)
        assert (s.range == 0).any() and (s.range > 0).sum() > s.range.size // 4
        x, y, z = decode_definition(s.range, sim_directions(sensor))
        hit = s.range > 0
        for got, want in ((x, s.x), (y, s.y), (z, s.z)):
            want = np.asarray(want, f32)
            np.testing.assert_array_equal(got[hit].view(np.uint32), want[hit].view(np.uint32))  # every return: the same bits
            # a pixel without a return: the definition says +0; synth multiplies the direction by 0 and keeps its sign (-0 == +0)
            np.testing.assert_array_equal(got, want)
            assert not np.signbit(got[~hit]).any() and (got[~hit] == 0).all()


def test_definition_at_the_ends_of_the_conversion():
    d = np.tile(f32([[1.0, -1.0, 0.5]]), (4, 1))
    o = np.tile(f32([[0.25, 0.0, -0.036]]), (4, 1))
    x, y, z = decode_definition(np.array([0, 1, 2**24 + 1, 0xFFFFFFFF], dtype=np.uint32), d, o)
    assert x[0] == 0 and y[0] == 0 and z[0] == 0 and not np.signbit([x[0], y[0], z[0]]).any()  # (+0, +0, +0), not the offset
    assert x[1] == f32(f32(0.001) + f32(0.25)) and y[1] == f32(-0.001)
    assert y[2] == -f32(f32(16777216.0) * f32(0.001))  # 2^24 + 1 is a tie: to even, 2^24
    assert y[3] == -f32(f32(4294967296.0) * f32(0.001))  # 0xFFFFFFFF rounds up to 2^32


def _accepted(oracle, sensor, x, y, z, rng_mm, dirs, offs, pixels):
    """check_sensor_params looks at the first valid pixel only: a mask with one pixel set puts each of `pixels` in front"""
    h, w = (synth.SENSORS[sensor] if isinstance(sensor, str) else sensor)[:2]
    sd = ScanData(x=x, y=y, z=z, width=w, height=h, range=rng_mm)
    verdicts = []
    for px in pixels:
        mask = np.zeros(h * w, dtype=np.uint8)
        mask[px] = 1
        ok, checked = check_sensor_params(oracle, sd, dirs, offs, mask)
        assert checked
        verdicts.append(ok)
    return np.array(verdicts)


def test_definition_fits_the_sensor_model_and_the_offsets_matter(oracle):
    sensor = "os1-16"
    s = synth.make_scan(synth.make_scene(3, n_targets=3), synth.make_pose(3), sensor, seed=3)
    valid = np.flatnonzero(s.range > 0)
    pixels = valid[np.random.default_rng(1).choice(valid.size, 200, replace=False)]
    for name, (dirs, offs) in (("offsets", offset_lut(sensor)), ("ouster", ouster_style_lut(oracle, sensor))):
        assert np.abs(offs).max() > 0.01, name
        x, y, z = decode_definition(s.range, dirs, offs)
        assert _accepted(oracle, sensor, x, y, z, s.range, dirs, offs, pixels).all(), name
    # the converse: synth's own points (no offsets) do not fit the offset LUT - 45 mm of beam offset against the check's 1e-3
    dirs, offs = offset_lut(sensor)
    assert not _accepted(oracle, sensor, s.x, s.y, s.z, s.range, dirs, offs, pixels).any()
