"""Motion-compensated range images on the GPU (include/vofod.h, MOTION COMPENSATION): the HIP detector is handed the sensor's range
column and a pose per measurement column and rebuilds the compensated points itself (k_range_decode_motion, range_decode.h); the
CPU oracle, which has neither input, is handed the points of the numpy statement (tests/range_motion_cases.py).

(a) vofod_range_to_points with col_tfs against the statement, bit for bit;  (b) batches through the frame kernel, three views, mixed
with plain range images and point scans, and which decode kernels a batch launches;  (c) the input forms of the pose tables, two
tickets in flight, the caller's buffers overwritten behind submit;  (d) the sensor stream: the raycast role ignores the poses;
(e) the moving sensor of tests/test_range_motion_cpu.py on the HIP library;  (f) (b) under each production fallback;  (g) errors."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from vofod_amd import capi, synth
from vofod_amd.detector import ScanData, default_params

import range_motion_cases as rm
from helpers import assert_detections_equal, make_pair
from test_gpu_frame_inputs import _profiled, three_views
from test_gpu_range_image import FLOORS, LUTS, DeviceMem, aos48_of, hip_detector, warmed_pair
from test_gpu_stream_route import compare_cycle, profiled_calls
from test_range_image_cpu import decode_definition, sample_ranges, sim_directions

pytestmark = pytest.mark.gpu
if os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"):
    pytest.skip("oracle against oracle: the oracle has no range input", allow_module_level=True)

f32 = np.float32
OS1_16 = synth.SENSORS["os1-16"]


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ (a) the kernel against the definition
def forms_of(mem, rng, T, w_, h_):
    """every way to hand over the range column (host, device, device at stride 48) and the pose table (host, device on a 16-byte
    boundary, device 4 bytes behind one)"""
    aos = aos48_of(rng)
    ranges = {
        "host": dict(range=rng),
        "device": dict(range=mem.put(rng), memspace=capi.MEM_DEVICE),
        "device_stride48": dict(range=mem.put(aos.view(np.uint8)) + 36, stride_bytes=48, memspace=capi.MEM_DEVICE),
        "host_stride48": dict(range=aos.ctypes.data + 36, stride_bytes=48),
    }
    d16, d4 = mem.put(T), mem.put(T, shift=4)
    assert d16 % 16 == 0 and d4 % 16 == 4
    out = {}
    for rname, kw in ranges.items():
        tables = {"table_host": T} if kw.get("memspace", capi.MEM_HOST) == capi.MEM_HOST else {"table_dev16": d16, "table_dev4": d4}
        for tname, tab in tables.items():
            out[f"{rname}/{tname}"] = ScanData.range_image(width=w_, height=h_, col_tfs=tab, **kw)
    return out, aos


def check_case(dev, mem, lut, rng, T, shift, lo, hi, shape, which, d_out, case):
    """one (LUT, ranges, pose table, shift): every form of `which` to host output and to device output, against the statement"""
    h_, w_ = shape[:2]
    n = h_ * w_
    dev.set_column_shift(shift)
    x, y, z, nan = rm.motion_definition(rng, lut[0], lut[1], T, w_, lo, hi, shift)
    forms, keep = forms_of(mem, rng, T, w_, h_)
    calls = 0
    for name in which:
        sd = forms[name]
        got = dev.range_to_points(sd)
        for a, (g, w) in enumerate(zip(got, (x, y, z))):
            np.testing.assert_array_equal(bits(g), bits(w), err_msg=f"{case}/{name}: axis {a}, host output")
        for p in d_out:
            assert mem.rt.hipMemcpy(C.c_void_p(p), np.full(n, 7.0, dtype=f32).ctypes.data_as(C.c_void_p), 4 * n, 1) == 0
        assert dev.range_to_points(sd, out=d_out) is None
        for a, (p, w) in enumerate(zip(d_out, (x, y, z))):
            np.testing.assert_array_equal(bits(mem.get(p, n)), bits(w), err_msg=f"{case}/{name}: axis {a}, device output")
        calls += 2
    return calls, int(nan.sum())


ALL_FORMS = ("host/table_host", "host_stride48/table_host", "device/table_dev16", "device/table_dev4", "device_stride48/table_dev16", "device_stride48/table_dev4")


@pytest.mark.parametrize("lut_kind", list(LUTS))
@pytest.mark.parametrize("shape_name", ["5x20", "3x21", "4x18", "os1_16"])
def test_range_to_points_with_poses_is_the_definition_bit_for_bit(hip, shape_name, lut_kind):
    """every pose table kind x every shift kind; on the small sensors each with every input form, on OS1-16 with the forms taking
    turns.  A counted, non-zero number of pixels takes the NaN rule, pixels ON the faces of the box included (and their neighbours
    one float outward, which do not)."""
    shape = rm.SHAPES[shape_name]
    h_, w_ = shape[:2]
    n = h_ * w_
    small = n < 1000
    assert {"5x20": n % 4 == 0 and w_ % 4 == 0, "3x21": n % 4 == 3, "4x18": n % 4 == 0 and w_ % 4 == 2, "os1_16": n % 4 == 0}[shape_name]
    base = LUTS[lut_kind](hip, shape)
    lo, hi = rm.exclude_bounds(default_params(hip)[0])
    rs = np.random.default_rng(n)
    pixels = rs.choice(n, 17, replace=False)
    pixels, no_return = pixels[:12], pixels[12:]
    d, o, face_inside = rm.with_face_pixels(base, lo, hi, pixels)
    lut = (d, o)
    dev = hip_detector(hip, shape, lut)
    rng = rm.near_ranges(sample_ranges(n, seed=n) if n >= 64 else rs.integers(0, 60_000, n).astype(np.uint32), share=0.25, seed=n)
    rng[pixels], rng[no_return] = 700, 0
    if not small:
        for v in (0, 1, 2**24 + 1, 0xFFFFFFFF):
            assert (rng == v).any()
    mem = DeviceMem()
    try:
        d_out = [mem.empty(4 * n) for _ in range(3)]
        dev.lib.profile_enable(dev.h, 1)
        calls = k = 0
        for pose_kind, make in rm.POSES.items():
            T = make(w_, seed=n)
            for shift_kind in rm.SHIFTS:
                shift = rm.shifts(shift_kind, h_, w_, seed=n)
                which = ALL_FORMS if small else (ALL_FORMS[k % 6], ALL_FORMS[(k + 3) % 6])
                c, n_nan = check_case(dev, mem, lut, rng, T, shift, lo, hi, shape, which, d_out, f"{shape_name}/{lut_kind}/{pose_kind}/{shift_kind}")
                calls += c
                k += 1
                assert n_nan >= 6 and n_nan < n  # (the six face pixels at the least)
        # the face pixels: ON a face -> NaN, one float outward -> a finite point (identity poses: the offset itself)
        x, _, _, nan = rm.motion_definition(rng, d, o, rm.identity_poses(w_), w_, lo, hi)
        np.testing.assert_array_equal(nan[pixels], face_inside)
        assert np.isfinite(x[pixels[~face_inside]]).all()
        launched = profiled_calls(dev.lib, dev)
        dev.lib.profile_enable(dev.h, 0)
        assert launched.get("k_range_decode_motion", 0) == calls and "k_range_decode" not in launched, launched
        # without col_tfs the same handle decodes rigidly, whatever its shift table says
        got = dev.range_to_points(ScanData.range_image(rng, w_, h_))
        for g, w in zip(got, decode_definition(rng, d, o)):
            np.testing.assert_array_equal(bits(g), bits(w))
    finally:
        mem.free()
        dev.close()


def test_range_to_points_with_poses_os1_128_once(hip):
    shape = rm.SHAPES["os1_128"]
    h_, w_ = shape[:2]
    n = h_ * w_
    lut = LUTS["offsets_28mm_36mm"](hip, shape)
    dev = hip_detector(hip, shape, lut)
    lo, hi = rm.exclude_bounds(dev.sp)
    rng = rm.near_ranges(sample_ranges(n, seed=1), share=0.1, seed=1)
    mem = DeviceMem()
    try:
        d_out = [mem.empty(4 * n) for _ in range(3)]
        _, n_nan = check_case(dev, mem, lut, rng, rm.general_poses(w_, seed=1), rm.shifts("random", h_, w_, seed=1), lo, hi, shape, ("device/table_dev16", "host/table_host"), d_out, "os1_128")
        assert n_nan > 1000
    finally:
        mem.free()
        dev.close()


# ------------------------------------------------------------------------------------------------ (b) batches through the frame kernel
N_BATCH = 33


@pytest.fixture(scope="module")
def pair16(oracle, hip):
    """the warmed OS1-16 pair of tests/test_gpu_range_image.py (0.25 m, LUT with beam offsets) with 33 frames, a pose table per frame
    (a constant twist, another one per frame) and the shifts of a destaggered image"""
    p = warmed_pair(oracle, hip, "os1-16", n_frames=N_BATCH, max_batch=N_BATCH)
    h_, w_ = p.shape[:2]
    inject_body_returns(p.frames)
    p.shift = rm.shifts("random", h_, w_, seed=7)
    p.dev.set_column_shift(p.shift)
    p.lo, p.hi = rm.exclude_bounds(p.dev.sp)
    p.tables = np.stack([rm.rigid_poses(w_, seed=f, yaw_rate=0.5 + 0.05 * f, v=(2.0, 0.1 * f, 0.0)) for f in range(N_BATCH)])  # one block: constant pitch
    p.comp = [rm.motion_definition(s.range, p.lut[0], p.lut[1], p.tables[f], w_, p.lo, p.hi, p.shift)[:3] for f, s in enumerate(p.frames)]
    p.plain = [decode_definition(s.range, *p.lut) for s in p.frames]
    return p


def inject_body_returns(frames, n_px=240):
    """a part of the vehicle in view: the same pixels of every frame return from 0.5..1.1 m, inside the exclude box - the NaN rule's
    share of a batch"""
    for f, s in enumerate(frames):
        rs = np.random.default_rng(500 + f)
        r = np.array(s.range, dtype=np.uint32)
        r[np.random.default_rng(499).choice(r.size, n_px, replace=False)] = rs.integers(500, 1101, n_px).astype(np.uint32)
        s.range = r


def ref_scan(p, f, compensated=True):
    x, y, z = (p.comp if compensated else p.plain)[f]
    s = p.frames[f]
    return ScanData(x=x, y=y, z=z, width=p.shape[1], height=p.shape[0], intensity=s.intensity, range=s.range)


def dev_scan(p, f, kind="motion", table=None):
    s = p.frames[f]
    h_, w_ = p.shape[:2]
    if kind == "motion":
        return ScanData.range_image(s.range, w_, h_, intensity=s.intensity, col_tfs=p.tables[f] if table is None else table)
    if kind == "plain":
        return ScanData.range_image(s.range, w_, h_, intensity=s.intensity)
    x, y, z = p.plain[f]
    return ScanData(x=x, y=y, z=z, width=w_, height=h_)


def decode_launches(dev, scans, tfs):
    _, names = _profiled(dev, lambda: dev.process_batch(scans, tfs))
    dev.lib.profile_enable(dev.h, 1)
    try:
        dev.batch_collect(dev.batch_submit(scans, tfs))
        sub = profiled_calls(dev.lib, dev)
    finally:
        dev.lib.profile_enable(dev.h, 0)
    assert names.get("k_range_decode_motion", 0) == sub.get("k_range_decode_motion", 0) and names.get("k_range_decode", 0) == sub.get("k_range_decode", 0), (names, sub)
    return names.get("k_range_decode_motion", 0), names.get("k_range_decode", 0)


def batch_case(p, n, case, rerun_ok=False):
    tfs = p.tfs[:n]
    scans_ref = [ref_scan(p, f) for f in range(n)]
    scans_dev = [dev_scan(p, f) for f in range(n)]
    frame_kernel = n >= 4  # (the frame kernel takes batches of four frames and more)
    three_views(p.ref, p.dev, scans_ref, scans_dev, tfs, "packed" if frame_kernel else "general", case, *FLOORS["os1-16"], expect_far=frame_kernel, rerun_ok=rerun_ok)
    assert decode_launches(p.dev, scans_dev, tfs) == (1, 0)  # one launch per batch; k_range_decode has nothing to do


@pytest.mark.parametrize("n", [1, 3, 9, N_BATCH])
def test_batches_of_compensated_range_images(pair16, n):
    p = pair16
    assert all(np.isnan(c[0]).sum() >= 200 for c in p.comp[:n])  # (the body returns: NaN in every frame)
    assert np.abs(p.comp[0][0] - p.plain[0][0])[np.isfinite(p.comp[0][0])].max() > 0.05  # (the poses move the points)
    batch_case(p, n, f"motion/{n}")


def test_mixed_batches(pair16):
    """compensated range images, plain ones and point scans in one batch: each frame's result is its own, k_range_decode_motion runs
    once, k_range_decode once only when plain range images are present.  full_*: max_batch frames, alternating - the two kinds share
    one job list of max_batch entries (the compensated images first), and here every entry is taken"""
    p = pair16
    kinds = {"all_three": ["motion", "plain", "points"], "motion_and_points": ["motion", "points"], "plain_and_points": ["plain", "points"], "motion_and_plain": ["plain", "motion"],
             "full_motion_first": ["motion", "plain"], "full_plain_first": ["plain", "motion"]}
    want_launches = {"all_three": (1, 1), "motion_and_points": (1, 0), "plain_and_points": (0, 1), "motion_and_plain": (1, 1), "full_motion_first": (1, 1), "full_plain_first": (1, 1)}
    for name, cyc in kinds.items():
        n = N_BATCH if name.startswith("full_") else 9
        tfs = p.tfs[:n]
        ks = [cyc[f % len(cyc)] for f in range(n)]
        scans_ref = [ref_scan(p, f, compensated=ks[f] == "motion") for f in range(n)]
        scans_dev = [dev_scan(p, f, ks[f]) for f in range(n)]
        three_views(p.ref, p.dev, scans_ref, scans_dev, tfs, "packed", f"motion/mixed/{name}", *FLOORS["os1-16"])
        assert decode_launches(p.dev, scans_dev, tfs) == want_launches[name], name


# ------------------------------------------------------------------------------------------------ (c) input forms
def same_detections(a, b, msg):
    assert len(a) == len(b), msg
    for k in ("frame", "n_points", "position", "confidence", "covariance", "detection_probability"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg}: {k}")


def test_pose_table_forms_and_buffers_overwritten_behind_submit(pair16):
    p = pair16
    n = 9
    h_, w_ = p.shape[:2]
    npx = h_ * w_
    tfs = p.tfs[:n]
    want, want_per = p.dev.process_batch([dev_scan(p, f) for f in range(n)], tfs)
    assert len(want) > 0
    arena = np.zeros(n * (12 * w_ + 40) + 64, dtype=f32)
    starts = [f * (12 * w_ + 40) + 4 * (f % 3) + (f * f) % 5 for f in range(n)]
    assert len(set(np.diff(starts))) > 1  # no constant pitch
    mem = DeviceMem()
    try:
        def host_block():
            block = p.tables[:n].copy()
            assert all(block[f].ctypes.data - block[0].ctypes.data == 48 * w_ * f for f in range(n))
            return [block[f] for f in range(n)], [block]

        def host_irregular():
            a = arena.copy()
            views = [a[s0 : s0 + 12 * w_].reshape(w_, 3, 4) for s0 in starts]
            for f, v in enumerate(views):
                v[:] = p.tables[f]
            return views, [a]

        def device_tables():
            return [mem.put(p.tables[f], shift=4 * (f % 2)) for f in range(n)], []

        for name, make in (("host_constant_pitch", host_block), ("host_irregular", host_irregular), ("device", device_tables)):
            device = name == "device"
            tickets, owned = [], []
            for _ in range(2):  # two tickets in flight
                tables, bufs = make()
                ranges = [p.frames[f].range.copy() for f in range(n)]
                if device:
                    scans = [ScanData.range_image(mem.put(ranges[f]), w_, h_, memspace=capi.MEM_DEVICE, col_tfs=tables[f]) for f in range(n)]
                else:
                    scans = [ScanData.range_image(ranges[f], w_, h_, col_tfs=tables[f]) for f in range(n)]
                tickets.append(p.dev.batch_submit(scans, tfs))
                # submit has returned: the host buffers are the caller's again
                for b in bufs:
                    b[:] = np.nan
                if not device:
                    for r in ranges:
                        r[:] = 1234
                owned.append((scans, tables, bufs, ranges))
            for t in tickets:
                got, per = p.dev.batch_collect(t)
                same_detections(got, want, name)
                np.testing.assert_array_equal(per, want_per)
            # the synchronous call on the same forms
            tables, bufs = make()
            if device:
                scans = [ScanData.range_image(mem.put(p.frames[f].range), w_, h_, memspace=capi.MEM_DEVICE, col_tfs=tables[f]) for f in range(n)]
            else:
                scans = [ScanData.range_image(p.frames[f].range, w_, h_, col_tfs=tables[f]) for f in range(n)]
            got, per = p.dev.process_batch(scans, tfs)
            same_detections(got, want, name + "/sync")
        assert npx % 4 == 0
    finally:
        mem.free()


# ------------------------------------------------------------------------------------------------ (e) the moving sensor on the HIP library
@pytest.fixture(scope="module")
def moving_pair(oracle, hip):
    """the set-up of tests/test_range_motion_cpu.py (1 rad/s, 3 m/s, simulated LUT) on both libraries"""
    ref, dev = make_pair(oracle, hip, "os1-16", 0.25, max_batch=8)
    warm_scene, scene, frames, col_tfs, shift = rm.moving_frames()
    rm.warm([ref, dev], warm_scene)
    dev.set_column_shift(shift)
    return SimpleNamespace(ref=ref, dev=dev, scene=scene, frames=frames, col_tfs=col_tfs, shift=shift)


def statement_scans(m):
    lo, hi = rm.exclude_bounds(m.dev.sp)
    d = sim_directions("os1-16")
    h_, w_ = OS1_16[:2]
    out = []
    for s in m.frames:
        x, y, z, _ = rm.motion_definition(s.range, d, None, m.col_tfs, w_, lo, hi, m.shift)
        out.append(ScanData(x=x, y=y, z=z, width=w_, height=h_, intensity=s.intensity, range=s.range))
    return out


def test_moving_sensor_detections_on_the_hip_library(moving_pair):
    m = moving_pair
    h_, w_ = OS1_16[:2]
    tfs = np.stack([s.tf for s in m.frames])
    want, want_per = m.ref.process_batch(statement_scans(m), tfs)
    scans = [ScanData.range_image(s.range, w_, h_, intensity=s.intensity, col_tfs=m.col_tfs) for s in m.frames]
    got, per = m.dev.process_batch(scans, tfs)
    np.testing.assert_array_equal(per, want_per)
    got = got.copy()
    got["id"] = want["id"]
    assert_detections_equal(want, got)
    assert len(got) >= 4 and not rm.off_target(got, m.scene).any()
    # the rigid decode of the same range images (no poses): at least half of its detections are off every target
    rigid, _ = m.dev.process_batch([ScanData.range_image(s.range, w_, h_) for s in m.frames], tfs)
    off = rm.off_target(rigid, m.scene)
    print(f"moving sensor on the HIP library: compensated {len(got)} detections, all on a target; rigid {len(rigid)}, {int(off.sum())} off every target")
    assert len(rigid) > 0 and 2 * int(off.sum()) >= len(rigid)


# ------------------------------------------------------------------------------------------------ (d) the sensor stream
def test_sensor_stream_of_a_moving_sensor(oracle, hip):
    """sequential vofod_process_scan with VOFOD_SCAN_AUTO_RAYCAST, sepclusters every second scan, maps, flags and detections compared
    scan by scan (test_gpu_stream_route.compare_cycle).  The oracle's raycast role casts the rigid rays from `range` and the LUT: the
    comparison also pins that the HIP raycast role ignores the poses."""
    ref, dev = make_pair(oracle, hip, "os1-16", 0.25, max_batch=1)
    warm_scene, scene, frames, col_tfs, shift = rm.moving_frames(n=4)
    rm.warm([ref, dev], warm_scene)
    dev.set_column_shift(shift)
    m = SimpleNamespace(ref=ref, dev=dev, frames=frames, col_tfs=col_tfs, shift=shift)
    scans_ref = statement_scans(m)
    h_, w_ = OS1_16[:2]
    scans_dev = [ScanData.range_image(s.range, w_, h_, intensity=s.intensity, col_tfs=col_tfs) for s in frames]

    class RangeFed:
        """the HIP detector behind compare_cycle: process_scan swaps the oracle's point scan for the range image with poses"""

        def __init__(self, det, swap):
            self._det, self._swap = det, swap

        def __getattr__(self, name):
            return getattr(self._det, name)

        def process_scan(self, scan, tf, **kw):
            return self._det.process_scan(self._swap[id(scan)], tf, **kw)

    fed = RangeFed(dev, {id(a): b for a, b in zip(scans_ref, scans_dev)})
    dev.lib.profile_enable(dev.h, 1)
    n_det = n_finished = 0
    for k, sd in enumerate(scans_ref):
        nd, fin = compare_cycle(ref, fed, SimpleNamespace(scan=sd, tf=frames[k].tf), k, ray_rtol=2e-5)
        n_det += nd
        n_finished += fin
    calls = profiled_calls(dev.lib, dev)
    dev.lib.profile_enable(dev.h, 0)
    print(f"motion/stream: detections {n_det}, raycast passes finished {n_finished}, launches {calls}")
    assert n_finished >= 2
    assert calls.get("k_range_decode_motion", 0) >= len(frames) and "k_range_decode" not in calls, calls  # (a scan that runs again may stage again)
    assert calls.get("k_raycast", 0) >= 2 and calls.get("k_ray_sweep", 0) >= 2, calls
    for d in (ref, dev):
        d.close()


# ------------------------------------------------------------------------------------------------ (f) under each production fallback
@pytest.mark.parametrize("fallback", ["VOFOD_CLOSE_FIRST=0", "VOFOD_DEVICE_TAIL=0", "VOFOD_LDS_MAX_BRICKS=4096"])
def test_compensated_batch_under_each_production_fallback(pair16, fallback, monkeypatch):
    k, v = fallback.split("=")
    monkeypatch.setenv(k, v)
    batch_case(pair16, 9, f"motion/9/{fallback}", rerun_ok=(k == "VOFOD_LDS_MAX_BRICKS"))


# ------------------------------------------------------------------------------------------------ (g) errors
def test_error_returns(pair16):
    p = pair16
    h_, w_ = p.shape[:2]
    s = p.frames[0]
    T = p.tables[0]
    tfa = np.ascontiguousarray(s.tf, dtype=f32).reshape(12)
    maps_before = [p.dev.read_map(w).copy() for w in (capi.MAP_VOXELS, capi.MAP_FLAGS, capi.MAP_RAYCAST)]
    status_before = p.dev.status()

    def scan_status(sd, how):
        cs = sd.as_c()
        n_out, dets = C.c_size_t(0), np.zeros(64, dtype=capi.DETECTION)
        if how == "submit":
            ticket = C.c_int(-1)
            return p.dev.lib.batch_submit(p.dev.h, C.byref(cs), capi.ptr(tfa), 1, C.byref(ticket))
        if how == "batch":
            per = np.zeros(1, dtype=np.uint32)
            return p.dev.lib.process_batch(p.dev.h, C.byref(cs), capi.ptr(tfa), 1, capi.ptr(dets), 64, capi.ptr(per), C.byref(n_out), None)
        if how == "scan":
            return p.dev.lib.process_scan(p.dev.h, C.byref(cs), capi.ptr(tfa), capi.SCAN_DEFAULT, capi.ptr(dets), 64, C.byref(n_out), None)  # (map-updating: a refusal must not)
        out = [np.zeros(h_ * w_, dtype=f32) for _ in range(3)]
        return p.dev.lib.range_to_points(p.dev.h, C.byref(cs), *(capi.ptr(a) for a in out), capi.MEM_HOST)

    x, y, z = p.plain[0]
    mem = DeviceMem()
    try:
        # col_tfs on a point scan
        point_scan = ScanData(x=x, y=y, z=z, width=w_, height=h_, range=s.range, col_tfs=T)
        for how in ("scan", "batch", "submit", "r2p"):
            assert scan_status(point_scan, how) == capi.ERR_INVALID_ARG, how
        # a device-resident table off 4 bytes
        d_rng, d_tab = mem.put(s.range), mem.put(T, shift=4)
        for off in (1, 2, 3):
            bad = ScanData.range_image(d_rng, w_, h_, memspace=capi.MEM_DEVICE, col_tfs=d_tab + off)
            for how in ("scan", "batch", "submit", "r2p"):
                assert scan_status(bad, how) == capi.ERR_INVALID_ARG, (off, how)
        assert scan_status(ScanData.range_image(d_rng, w_, h_, memspace=capi.MEM_DEVICE, col_tfs=d_tab), "r2p") == capi.OK  # (the converse)
        # a mixed batch with one bad frame is refused as a whole
        arr = (capi.Scan * 2)(dev_scan(p, 0).as_c(), point_scan.as_c())
        tf2 = np.ascontiguousarray(p.tfs[:2], dtype=f32)
        ticket = C.c_int(-1)
        assert p.dev.lib.batch_submit(p.dev.h, arr, capi.ptr(tf2), 2, C.byref(ticket)) == capi.ERR_INVALID_ARG
        # vofod_set_column_shift while a ticket is pending
        t = p.dev.batch_submit([dev_scan(p, f) for f in range(4)], p.tfs[:4])
        assert p.dev.set_column_shift(np.zeros(h_, dtype=np.int32), allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
        assert p.dev.set_column_shift(None, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
        got, _ = p.dev.batch_collect(t)
        want, _ = p.dev.process_batch([dev_scan(p, f) for f in range(4)], p.tfs[:4])
        same_detections(got, want, "the refused shift changed nothing")
        assert p.dev.lib.set_column_shift(None, None) == capi.ERR_INVALID_ARG
        for w, before in zip((capi.MAP_VOXELS, capi.MAP_FLAGS, capi.MAP_RAYCAST), maps_before):
            np.testing.assert_array_equal(p.dev.read_map(w).view(np.uint32), before.view(np.uint32))
        st = p.dev.status()
        assert (st.detection_its, st.last_detection_id - status_before.last_detection_id >= 0, st.raycast_pending) == (status_before.detection_its, True, status_before.raycast_pending)
        # NULL restores zeros; the table is kept across vofod_reset
        one = ScanData.range_image(s.range, w_, h_, col_tfs=T)
        shifted = p.dev.range_to_points(one)
        np.testing.assert_array_equal(bits(shifted[0]), bits(p.comp[0][0]))
        assert p.dev.set_column_shift(None) == capi.OK
        zeros = rm.motion_definition(s.range, p.lut[0], p.lut[1], T, w_, p.lo, p.hi, None)
        assert (bits(zeros[0]) != bits(p.comp[0][0])).any()
        np.testing.assert_array_equal(bits(p.dev.range_to_points(one)[0]), bits(zeros[0]))
        assert p.dev.set_column_shift(p.shift) == capi.OK
        np.testing.assert_array_equal(bits(p.dev.range_to_points(one)[1]), bits(p.comp[0][1]))
    finally:
        mem.free()
        p.dev.set_column_shift(p.shift)


def test_column_shift_survives_reset_apply_and_map_shift(hip):
    shape = rm.SHAPES["4x18"]
    h_, w_ = shape[:2]
    lut = LUTS["offsets_28mm_36mm"](hip, shape)
    dev = hip_detector(hip, shape, lut)
    try:
        lo, hi = rm.exclude_bounds(dev.sp)
        rng = np.random.default_rng(3).integers(2000, 60_000, h_ * w_).astype(np.uint32)
        T = rm.general_poses(w_, seed=3)
        shift = rm.shifts("random", h_, w_, seed=3)
        want = rm.motion_definition(rng, lut[0], lut[1], T, w_, lo, hi, shift)
        dev.set_column_shift(shift)
        sd = ScanData.range_image(rng, w_, h_, col_tfs=T)
        snapshot = dev.export_map()
        for step in (dev.reset, lambda: dev.apply_map(snapshot), lambda: dev.map_shift([1, 0, 0], [40.0 + float(dev.sp.voxel_size), 20.0, -1.25])):
            step()
            got = dev.range_to_points(sd)
            for g, w in zip(got, want[:3]):
                np.testing.assert_array_equal(bits(g), bits(w))
    finally:
        dev.close()
