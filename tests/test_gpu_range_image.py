"""Range images on the GPU (include/vofod.h: a vofod_scan with x == y == z == NULL): the HIP detector is handed the sensor's
range column ONLY and rebuilds the points itself (k_range_decode, range_decode.h); the CPU oracle, which has no range input, is
handed the points of the numpy statement of the definition (tests/test_range_image_cpu.py: decode_definition).  Both sides hold
the same LUT (helpers.make_pair(..., lut=...)).

(a) vofod_range_to_points against the numpy statement, bit for bit (tolerance zero: the same IEEE operations on both sides);
(b) batches through the frame kernel, three views, on a LUT with beam offsets;  (c) the four input forms give identical results;
(d) the sensor stream from {range, intensity} alone;  (e) the error returns;  (f) (b) under each production fallback.
The warm-up recipe is that of tests/test_gpu_frame_inputs.py."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from vofod_amd import capi, synth
from vofod_amd.detector import ScanData, VoFOD, default_params

from helpers import make_pair
from test_gpu_frame_inputs import DEFAULT_AREA, DeviceBlocks, _profiled, scene_frames, three_views, warm_both
from test_gpu_stream_route import compare_cycle, profiled_calls
from test_range_image_cpu import decode_definition, offset_lut, ouster_style_lut, sample_ranges, sim_directions

pytestmark = pytest.mark.gpu
if os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"):
    pytest.skip("oracle against oracle: the oracle has no range input", allow_module_level=True)

f32 = np.float32
AOS48 = np.dtype({"names": ["x", "y", "z", "intensity", "range"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 16, 36], "itemsize": 48})  # ouster_ros::Point


# ------------------------------------------------------------------------------------------------ helpers
class DeviceMem(DeviceBlocks):
    """raw device buffers on top of DeviceBlocks' runtime binding"""

    def put(self, raw, shift=0):
        """`raw` (bytes as uint8) on the device, `shift` bytes behind a 16-byte boundary"""
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), raw.size + 16) == 0
        self.ptrs.append(p)
        assert p.value % 16 == 0
        assert self.rt.hipMemcpy(C.c_void_p(p.value + shift), raw.ctypes.data_as(C.c_void_p), raw.size, 1) == 0  # hipMemcpyHostToDevice
        return p.value + shift

    def empty(self, nbytes):
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), nbytes) == 0
        self.ptrs.append(p)
        return p.value

    def get(self, addr, n, dtype=f32):
        out = np.empty(n, dtype=dtype)
        assert self.rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(addr), out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out


def hip_detector(hip, shape, lut, vs=0.5, max_batch=1):
    sp, dp = default_params(hip)
    sp.voxel_size = vs
    sp.sensor_hrays, sp.sensor_vrays = shape[1], shape[0]
    sp.sensor_vfov = f32(np.deg2rad(shape[2]))
    sp.max_batch_frames = max_batch
    return VoFOD(hip, sp, dp, lut_directions=lut[0], lut_offsets=lut[1])


def aos48_of(rng_mm):
    a = np.zeros(rng_mm.size, dtype=AOS48)
    a["x"] = a["y"] = a["z"] = np.nan  # (never read: the scan hands over no point column)
    a["intensity"], a["range"] = 7.0, rng_mm
    return a


def ran_range_decode_and_packed_frame_kernel(names):
    assert names.get("k_range_decode", 0) >= 1, names
    fam = [n for n in names if n.startswith("k_frame_lds")]
    assert fam and not [n for n in fam if n.endswith("_strided")], names


def decoded_scans(frames, lut, shape):
    """what the oracle gets: the numpy statement's points as plain host columns (+ intensity and range for the raycast role)"""
    out = []
    for s in frames:
        x, y, z = decode_definition(s.range, *lut)
        out.append(ScanData(x=x, y=y, z=z, width=shape[1], height=shape[0], intensity=s.intensity, range=s.range))
    return out


def range_scans(frames, shape):
    return [ScanData.range_image(s.range, shape[1], shape[0], intensity=s.intensity) for s in frames]


# ------------------------------------------------------------------------------------------------ (a) the kernel against the definition
LUTS = {
    "simulated": lambda hip, shape: (sim_directions(shape), None),
    "offsets_28mm_36mm": lambda hip, shape: offset_lut(shape),
    "ouster": lambda hip, shape: ouster_style_lut(hip, shape),
}
OS1_16 = synth.SENSORS["os1-16"]
ODD = (15, 1021, 33.2, 120.0)  # w * h = 15 315 = 3 mod 4


@pytest.mark.parametrize("shape", [OS1_16, ODD], ids=["os1_16", "n_mod4_3"])
@pytest.mark.parametrize("lut_kind", list(LUTS))
def test_range_to_points_is_the_definition_bit_for_bit(hip, lut_kind, shape):
    """every layout of the issue on one handle: host / device input, host / device output, stride 4, stride 48 with range at +36
    (the ouster_ros::Point), a device base 4 bytes behind a 16-byte boundary; on a sensor of w * h % 4 == 0 and on one of
    w * h % 4 == 3; ranges include 0, 1, 2^24 + 1 and 0xFFFFFFFF."""
    lut = LUTS[lut_kind](hip, shape)
    n = shape[0] * shape[1]
    assert n % 4 == (0 if shape is OS1_16 else 3)
    dev = hip_detector(hip, shape, lut)
    rng = sample_ranges(n, seed=n)
    for v in (0, 1, 2**24 + 1, 0xFFFFFFFF):
        assert (rng == v).any()
    want = decode_definition(rng, *lut)
    assert all(np.isfinite(w).all() for w in want)
    if lut[1] is not None:
        assert sum(int((w[rng == 1] != 0).sum()) for w in want) > 0  # (the offsets are in: 1 mm along the beam is not the point)
    aos = aos48_of(rng)
    mem = DeviceMem()
    w_, h_ = shape[1], shape[0]
    try:
        inputs = {
            "host_stride4": ScanData.range_image(rng, w_, h_),
            "host_stride48": ScanData.range_image(aos.ctypes.data + 36, w_, h_, stride_bytes=48),
            "device_stride4": ScanData.range_image(mem.put(rng), w_, h_, memspace=capi.MEM_DEVICE),
            "device_stride4_plus4": ScanData.range_image(mem.put(rng, shift=4), w_, h_, memspace=capi.MEM_DEVICE),
            "device_stride48": ScanData.range_image(mem.put(aos.view(np.uint8)) + 36, w_, h_, stride_bytes=48, memspace=capi.MEM_DEVICE),
        }
        assert inputs["device_stride4"].range % 16 == 0 and inputs["device_stride4_plus4"].range % 16 == 4
        d_out = [mem.empty(4 * n) for _ in range(3)]
        dev.lib.profile_enable(dev.h, 1)
        for name, sd in inputs.items():
            got = dev.range_to_points(sd)
            for a, (g, w) in enumerate(zip(got, want)):
                np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=f"{lut_kind}/{name}: axis {a}, host output")
            for p in d_out:
                assert mem.rt.hipMemcpy(C.c_void_p(p), np.full(n, np.nan, dtype=f32).ctypes.data_as(C.c_void_p), 4 * n, 1) == 0
            assert dev.range_to_points(sd, out=d_out) is None
            for a, (p, w) in enumerate(zip(d_out, want)):
                np.testing.assert_array_equal(mem.get(p, n).view(np.uint32), w.view(np.uint32), err_msg=f"{lut_kind}/{name}: axis {a}, device output")
        calls = profiled_calls(dev.lib, dev)
        dev.lib.profile_enable(dev.h, 0)
        assert calls.get("k_range_decode", 0) == 2 * len(inputs), calls
    finally:
        mem.free()
        dev.close()


# ------------------------------------------------------------------------------------------------ (b) batches through the frame kernel
def warmed_pair(oracle, hip, sensor, n_frames=8, max_batch=8):
    """an oracle and a HIP detector at 0.25 m under the offset LUT, warmed with the recipe of test_gpu_frame_inputs.py, and the
    frames (floating targets that appeared after the warm-up)"""
    shape = synth.SENSORS[sensor]
    lut = offset_lut(sensor)
    ref, dev = make_pair(oracle, hip, sensor, 0.25, max_batch=max_batch, lut=lut)
    warm_scene, _, frames = scene_frames(DEFAULT_AREA, (0.0, 0.0), n_frames, shape=shape)
    warm_both(ref, dev, warm_scene, (0.0, 0.0), shape=shape)
    return SimpleNamespace(ref=ref, dev=dev, frames=frames, lut=lut, shape=shape, tfs=np.stack([s.tf for s in frames]))


@pytest.fixture(scope="module")
def pair16(oracle, hip):
    return warmed_pair(oracle, hip, "os1-16")


@pytest.fixture(scope="module")
def pair128(oracle, hip):
    return warmed_pair(oracle, hip, "os1-128")


# the oracle's own output on these frames (CPU run): OS1-16 4 926..7 578 points after the crops, 3 470..4 827 voxels, 16 detections;
# OS1-128 42 550..62 889 points, 23 432..28 924 voxels, 28 detections - at least one in every frame
FLOORS = {"os1-16": (4000, 3000), "os1-128": (40_000, 20_000)}


def batch_case(p, sensor, case, rerun_ok=False):
    scans_ref = decoded_scans(p.frames, p.lut, p.shape)
    scans_dev = range_scans(p.frames, p.shape)
    assert all(sd.x is None and sd.y is None and sd.z is None for sd in scans_dev)
    three_views(p.ref, p.dev, scans_ref, scans_dev, p.tfs, "packed", case, *FLOORS[sensor], rerun_ok=rerun_ok)  # (asserts detections > 0 on the oracle's side)
    _, names = _profiled(p.dev, lambda: p.dev.process_batch(scans_dev, p.tfs))
    ran_range_decode_and_packed_frame_kernel(names)
    assert names["k_range_decode"] == 1, names  # one launch per batch
    ticket = None
    p.dev.lib.profile_enable(p.dev.h, 1)
    try:
        ticket = p.dev.batch_submit(scans_dev, p.tfs)
        p.dev.batch_collect(ticket)
        names = profiled_calls(p.dev.lib, p.dev)
    finally:
        p.dev.lib.profile_enable(p.dev.h, 0)
    ran_range_decode_and_packed_frame_kernel(names)


@pytest.mark.parametrize("sensor", ["os1-16", "os1-128"])
def test_batches_of_range_images_through_the_frame_kernel(request, sensor):
    p = request.getfixturevalue("pair16" if sensor == "os1-16" else "pair128")
    assert len(p.frames) >= 8 and np.abs(p.lut[1]).max() > 0.02
    batch_case(p, sensor, f"range/{sensor}")


# ------------------------------------------------------------------------------------------------ (c) input forms
def test_input_forms_give_identical_results(pair16):
    """host ranges at a constant pitch (one 2-D copy), per-frame host buffers at irregular distances, device-resident ranges and
    a batch that mixes range images with point scans (the numpy statement's points): the same detections and the same debug view"""
    p = pair16
    n, (h_, w_) = p.frames[0].range.size, p.shape[:2]
    F = len(p.frames)
    block = np.stack([s.range for s in p.frames]).astype(np.uint32)  # [F, n], C order: pitch 4 n
    arena = np.zeros(F * (n + 64) + 1024, dtype=np.uint32)
    starts = [f * (n + 64) + 4 * (f % 3) + (f * f) % 7 for f in range(F)]  # no constant pitch
    assert len(set(np.diff(starts))) > 1
    for f, s0 in enumerate(starts):
        arena[s0 : s0 + n] = p.frames[f].range
    points = decoded_scans(p.frames, p.lut, p.shape)
    mem = DeviceMem()
    try:
        forms = {
            "host_constant_pitch": [ScanData.range_image(block[f], w_, h_) for f in range(F)],
            "host_per_frame": [ScanData.range_image(arena[s0 : s0 + n], w_, h_) for s0 in starts],
            "device": [ScanData.range_image(mem.put(s.range), w_, h_, memspace=capi.MEM_DEVICE) for s in p.frames],
            "mixed": [ScanData.range_image(block[f], w_, h_) if f % 2 == 0 else ScanData(x=points[f].x, y=points[f].y, z=points[f].z, width=w_, height=h_) for f in range(F)],
        }
        assert all(forms["host_constant_pitch"][f].range.ctypes.data - forms["host_constant_pitch"][0].range.ctypes.data == 4 * n * f for f in range(F))
        results = {}
        for name, scans in forms.items():
            (dets, per, dbg), names = _profiled(p.dev, lambda: p.dev.process_batch(scans, p.tfs, debug=True, clusters_cap=8192))
            assert names.get("k_range_decode", 0) == 1, (name, names)
            prod, per_prod = p.dev.process_batch(scans, p.tfs)
            t = [p.dev.batch_submit(scans, p.tfs) for _ in range(2)]
            coll = [p.dev.batch_collect(x) for x in t]
            results[name] = (dets, per, dbg, prod, per_prod, coll)
        first = results["host_constant_pitch"]
        assert len(first[0]) > 0
        for name, r in results.items():
            for k in ("frame", "n_points", "position", "confidence", "covariance", "detection_probability"):
                np.testing.assert_array_equal(r[0][k], first[0][k], err_msg=f"{name}: {k}")
                np.testing.assert_array_equal(r[3][k], first[3][k], err_msg=f"{name}: production, {k}")
                for c in r[5]:
                    np.testing.assert_array_equal(c[0][k], first[3][k], err_msg=f"{name}: tickets, {k}")
            np.testing.assert_array_equal(r[1], first[1])
            np.testing.assert_array_equal(r[4], first[4])
            for g, g0 in zip(r[2], first[2]):
                np.testing.assert_array_equal(g["weighted"].view(np.uint32), g0["weighted"].view(np.uint32), err_msg=name)
                np.testing.assert_array_equal(g["labels"], g0["labels"], err_msg=name)
                assert g["n_input_after_crop"] == g0["n_input_after_crop"]
    finally:
        mem.free()


# ------------------------------------------------------------------------------------------------ (d) the sensor stream
def test_sensor_stream_from_range_and_intensity_alone(oracle, hip):
    """sequential vofod_process_scan with VOFOD_SCAN_AUTO_RAYCAST (the raycast role reads the same two columns), sepclusters every
    second scan; every scan against the oracle with the tolerances of the raycast's float accumulation
    (test_gpu_stream_route.compare_cycle, as tests/test_gpu_parity.py)"""
    p = warmed_pair(oracle, hip, "os1-128", n_frames=4, max_batch=1)
    scans_ref = decoded_scans(p.frames, p.lut, p.shape)
    scans_dev = range_scans(p.frames, p.shape)

    class RangeFed:
        """the HIP detector behind compare_cycle: every call goes through, process_scan swaps the oracle's point scan for the
        range image of the same frame"""

        def __init__(self, det, swap):
            self._det, self._swap = det, swap

        def __getattr__(self, name):
            return getattr(self._det, name)

        def process_scan(self, scan, tf, **kw):
            return self._det.process_scan(self._swap[id(scan)], tf, **kw)

    fed = RangeFed(p.dev, {id(a): b for a, b in zip(scans_ref, scans_dev)})
    p.dev.lib.profile_enable(p.dev.h, 1)
    n_det = n_finished = 0
    for k, sd in enumerate(scans_ref):
        nd, fin = compare_cycle(p.ref, fed, SimpleNamespace(scan=sd, tf=p.frames[k].tf), k, ray_rtol=2e-5)
        n_det += nd
        n_finished += fin
    calls = profiled_calls(p.dev.lib, p.dev)
    p.dev.lib.profile_enable(p.dev.h, 0)
    print(f"range/stream: detections {n_det}, raycast passes finished {n_finished}, launches {calls}")
    assert n_det > 0 and n_finished >= 2  # (the oracle on the CPU: 5 + 3 + 5 + 3 = 16)
    assert calls.get("k_range_decode", 0) >= len(p.frames) and calls.get("k_raycast", 0) >= 2 and calls.get("k_ray_sweep", 0) >= 2, calls


# ------------------------------------------------------------------------------------------------ (e) errors
def test_error_returns(pair16):
    p = pair16
    s = p.frames[0]
    h_, w_ = p.shape[:2]
    x, y, z = decode_definition(s.range, *p.lut)
    tfa = np.ascontiguousarray(s.tf, dtype=f32).reshape(12)

    def scan_status(sd, batch=False, submit=False):
        cs = sd.as_c()
        n_out, dets = C.c_size_t(0), np.zeros(8, dtype=capi.DETECTION)
        if submit:
            ticket = C.c_int(-1)
            return p.dev.lib.batch_submit(p.dev.h, C.byref(cs), capi.ptr(tfa), 1, C.byref(ticket))
        if batch:
            per = np.zeros(1, dtype=np.uint32)
            return p.dev.lib.process_batch(p.dev.h, C.byref(cs), capi.ptr(tfa), 1, capi.ptr(dets), 8, capi.ptr(per), C.byref(n_out), None)
        return p.dev.lib.process_scan(p.dev.h, C.byref(cs), capi.ptr(tfa), capi.SCAN_NO_MAP_UPDATE, capi.ptr(dets), 8, C.byref(n_out), None)

    partial = [dict(x=None, y=y, z=z), dict(x=x, y=None, z=z), dict(x=x, y=y, z=None), dict(x=None, y=None, z=z), dict(x=x, y=None, z=None), dict(x=None, y=y, z=None)]
    for cols in partial:  # one or two of the three NULL - with a range column present
        sd = ScanData(width=w_, height=h_, range=s.range, **cols)
        for kw in ({}, {"batch": True}, {"submit": True}):
            assert scan_status(sd, **kw) == capi.ERR_INVALID_ARG, (cols.keys(), kw)
    nothing = ScanData(x=None, y=None, z=None, width=w_, height=h_, intensity=s.intensity)  # all NULL and no range either
    for kw in ({}, {"batch": True}, {"submit": True}):
        assert scan_status(nothing, **kw) == capi.ERR_INVALID_ARG
    wrong = ScanData.range_image(s.range[: (h_ - 1) * w_], w_, h_ - 1)
    for kw in ({}, {"batch": True}, {"submit": True}):
        assert scan_status(wrong, **kw) == capi.ERR_SIZE_MISMATCH
    assert scan_status(ScanData.range_image(s.range, w_, h_)) == capi.OK  # (the converse)
    # vofod_range_to_points
    out = [np.zeros(h_ * w_, dtype=f32) for _ in range(3)]

    def r2p(sd):
        cs = sd.as_c()
        return p.dev.lib.range_to_points(p.dev.h, C.byref(cs), *(capi.ptr(a) for a in out), capi.MEM_HOST)

    assert r2p(ScanData(x=x, y=y, z=z, width=w_, height=h_, range=s.range)) == capi.ERR_INVALID_ARG  # a point scan
    assert r2p(ScanData(x=None, y=y, z=z, width=w_, height=h_, range=s.range)) == capi.ERR_INVALID_ARG
    assert r2p(nothing) == capi.ERR_INVALID_ARG
    assert r2p(wrong) == capi.ERR_SIZE_MISMATCH
    assert r2p(ScanData.range_image(s.range, w_, h_)) == capi.OK
    np.testing.assert_array_equal(out[0].view(np.uint32), x.view(np.uint32))
    # the raycast role still needs the intensity column
    assert p.dev.raycast_begin(ScanData.range_image(s.range, w_, h_), s.tf, allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ (f) under each production fallback
@pytest.mark.parametrize("fallback", ["VOFOD_CLOSE_FIRST=0", "VOFOD_DEVICE_TAIL=0", "VOFOD_LDS_MAX_BRICKS=4096"])
def test_batches_of_range_images_under_each_production_fallback(pair128, fallback, monkeypatch):
    """(b) at OS1-128 under the switches test_bench_workload_256_frames_os1_128 parametrises (read on every call): the full
    clustering, the host tail, and frames beyond the LDS image - that batch is run again on the general kernels, from the decoded
    columns its first launch left in the staging block"""
    k, v = fallback.split("=")
    monkeypatch.setenv(k, v)
    batch_case(pair128, "os1-128", f"range/os1-128/{fallback}", rerun_ok=(k == "VOFOD_LDS_MAX_BRICKS"))
