"""Motion-compensated point scans on the GPU (include/vofod.h, MOTION COMPENSATION OF POINT SCANS): the HIP detector is handed the
nodelet's own points and a pose per measurement column and applies the poses itself (k_point_deskew, point_deskew.h); the CPU oracle,
which has no motion input, is handed the points of the numpy statement (tests/point_motion_cases.py).

(a) vofod_deskew_points against the statement, bit for bit, over the input forms;  (b) against vofod_range_to_points with poses;
(c) the pipeline with the switch on, three views, tickets, which kernels a batch launches;  (d) mixed batches of all four kinds of
frame;  (e) (c) under each production fallback;  (f) VOFOD_SCAN_AUTO_RAYCAST;  (g) the switch and the error returns."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from vofod_amd import capi
from vofod_amd.detector import ScanData

import point_motion_cases as pm
import range_motion_cases as rm
from helpers import make_pair
from test_gpu_frame_inputs import _profiled, _switches, host_scan, lay_aos48, lay_interleaved, three_views
from test_gpu_range_image import FLOORS, DeviceMem, hip_detector, warmed_pair
from test_gpu_range_motion import inject_body_returns, same_detections
from test_gpu_stream_route import profiled_calls
from test_range_image_cpu import decode_definition, offset_lut, sample_ranges, sim_directions

pytestmark = pytest.mark.gpu
if os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"):
    pytest.skip("oracle against oracle: the oracle has no motion input", allow_module_level=True)

f32 = np.float32
DECODES = ("k_point_deskew", "k_range_decode_motion", "k_range_decode")


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def cloud(x, y, z, shape):
    """what the lay_* functions of tests/test_gpu_frame_inputs.py take"""
    return SimpleNamespace(x=x, y=y, z=z, intensity=None, range=None, scan=SimpleNamespace(width=shape[1], height=shape[0]))


# ------------------------------------------------------------------------------------------------ (a) the kernel against the definition
def forms_of(mem, x, y, z, T, shape):
    """every way to hand over the points and the pose table -> {name: (ScanData, [(device address, bytes put there)])}"""
    h_, w_ = shape[:2]
    c = cloud(x, y, z, shape)
    out = {}

    def host(name, sd):
        sd.col_tfs = T
        out[f"{name}/table_host"] = (sd, [])

    host("host_packed", ScanData(x=x, y=y, z=z, width=w_, height=h_))
    for stride in (12, 16):
        host(f"host_stride{stride}", host_scan(c, lay_interleaved(c, stride)))
    host("host_stride48", host_scan(c, lay_aos48(c)))
    d16, d4 = mem.put(T), mem.put(T, shift=4)
    assert d16 % 16 == 0 and d4 % 16 == 4
    raw48 = lay_aos48(c)[0]
    for tname, tab, traw in (("table_dev16", d16, T), ("table_dev4", d4, T)):
        cols = [mem.put(v) for v in (x, y, z)]
        out[f"device_packed/{tname}"] = (ScanData(x=cols[0], y=cols[1], z=cols[2], width=w_, height=h_, memspace=capi.MEM_DEVICE, col_tfs=tab),
                                          [(p, v) for p, v in zip(cols, (x, y, z))] + [(tab, traw)])
        cols4 = [mem.put(v, shift=4) for v in (x, y, z)]
        assert cols[0] % 16 == 0 and cols4[0] % 16 == 4
        out[f"device_plus4/{tname}"] = (ScanData(x=cols4[0], y=cols4[1], z=cols4[2], width=w_, height=h_, memspace=capi.MEM_DEVICE, col_tfs=tab),
                                         [(p, v) for p, v in zip(cols4, (x, y, z))] + [(tab, traw)])
        base = mem.put(raw48)
        out[f"device_stride48/{tname}"] = (ScanData(x=base, y=base + 4, z=base + 8, width=w_, height=h_, stride_bytes=48, memspace=capi.MEM_DEVICE, col_tfs=tab), [(base, raw48), (tab, traw)])
    return out


ALL_FORMS = ["host_packed/table_host", "host_stride12/table_host", "host_stride16/table_host", "host_stride48/table_host"] + [
    f"{d}/{t}" for d in ("device_packed", "device_plus4", "device_stride48") for t in ("table_dev16", "table_dev4")]


@pytest.mark.parametrize("shape_name", list(pm.SHAPES))
def test_deskew_points_is_the_statement_bit_for_bit(hip, shape_name):
    """every pose table kind x every shift kind; on the small sensors each with every input form, on OS1-16 with the forms taking turns;
    host and device output.  The clouds hold zeros of either sign, NaN, +-Inf and points on and just outside every face of the box.
    The caller's device buffers are unchanged after every call, and every call is one launch of k_point_deskew."""
    shape = pm.SHAPES[shape_name]
    h_, w_ = shape[:2]
    n = h_ * w_
    small = n < 1000
    assert {"5x20": n % 4 == 0, "3x21": n % 4 == 3 and n < 64, "4x18": n % 4 == 0 and w_ % 4 == 2, "3x100": w_ % 64 != 0 and w_ > 64 and n > 256, "2x70": 64 < w_ < 128, "os1_16": n % 4 == 0}[shape_name]
    dev = hip_detector(hip, shape, (sim_directions(shape), None))
    lo, hi = rm.exclude_bounds(dev.sp)
    x, y, z, special_at, face_at, face_inside = pm.sample_points(shape, lo, hi, seed=n)
    assert len(special_at) == len(pm.SPECIALS) and len(face_at) == 24
    mem = DeviceMem()
    try:
        d_out = [mem.empty(4 * n) for _ in range(3)]
        dev.lib.profile_enable(dev.h, 1)
        calls = k = 0
        for pose_kind, make in pm.POSES.items():
            T = np.ascontiguousarray(make(w_, seed=n), dtype=f32)
            forms = forms_of(mem, x, y, z, T, shape)
            assert sorted(forms) == sorted(ALL_FORMS)
            for shift_kind in pm.SHIFTS:
                shift = rm.shifts(shift_kind, h_, w_, seed=n)
                dev.set_column_shift(shift)
                want = pm.point_definition(x, y, z, T, w_, lo, hi, shift)
                which = ALL_FORMS if small else [ALL_FORMS[(3 * k + j) % len(ALL_FORMS)] for j in range(3)]
                for name in which:
                    sd, owned = forms[name]
                    case = f"{shape_name}/{pose_kind}/{shift_kind}/{name}"
                    got = dev.deskew_points(sd)
                    for a in range(3):
                        np.testing.assert_array_equal(bits(got[a]), bits(want[a]), err_msg=f"{case}: axis {a}, host output")
                    for p in d_out:
                        assert mem.rt.hipMemcpy(C.c_void_p(p), np.full(n, 7.0, dtype=f32).ctypes.data_as(C.c_void_p), 4 * n, 1) == 0
                    assert dev.deskew_points(sd, out=d_out) is None
                    for a in range(3):
                        np.testing.assert_array_equal(bits(mem.get(d_out[a], n)), bits(want[a]), err_msg=f"{case}: axis {a}, device output")
                    for addr, put in owned:  # the caller's device memory is read in place and never written
                        raw = np.ascontiguousarray(put).view(np.uint8).reshape(-1)
                        np.testing.assert_array_equal(mem.get(addr, raw.size, dtype=np.uint8), raw, err_msg=f"{case}: the caller's device buffer changed")
                    calls += 2
                k += 1
                # the hand cases inside the cloud
                nan = want[3]
                assert not nan[special_at[:4]].any() and nan[special_at[4:14]].all() and not nan[special_at[14:]].any()
                for a in range(3):
                    assert (bits(want[a][special_at[:4]]) == 0).all()
                np.testing.assert_array_equal(nan[face_at], face_inside)
        launched = profiled_calls(dev.lib, dev)
        dev.lib.profile_enable(dev.h, 0)
        assert launched.get("k_point_deskew", 0) == calls and not [k_ for k_ in launched if k_.startswith("k_range_decode")], launched
    finally:
        mem.free()
        dev.close()


# ------------------------------------------------------------------------------------------------ (b) against the compensated range image
@pytest.mark.parametrize("shape_name", ["4x18", "3x100", "os1_16"])
def test_deskewed_rigid_decode_is_the_compensated_range_image(hip, shape_name):
    shape = pm.SHAPES[shape_name]
    h_, w_ = shape[:2]
    n = h_ * w_
    dev = hip_detector(hip, shape, offset_lut(shape))
    try:
        rng = rm.near_ranges(sample_ranges(n, seed=n), share=0.25, seed=n)
        dev.lib.profile_enable(dev.h, 1)
        for pose_kind, make in pm.POSES.items():
            T = np.ascontiguousarray(make(w_, seed=n), dtype=f32)
            for shift_kind in pm.SHIFTS:
                dev.set_column_shift(rm.shifts(shift_kind, h_, w_, seed=n))
                x, y, z = dev.range_to_points(ScanData.range_image(rng, w_, h_))
                want = dev.range_to_points(ScanData.range_image(rng, w_, h_, col_tfs=T))
                got = dev.deskew_points(ScanData(x=x, y=y, z=z, width=w_, height=h_, col_tfs=T))
                for a in range(3):
                    np.testing.assert_array_equal(bits(got[a]), bits(want[a]), err_msg=f"{shape_name}/{pose_kind}/{shift_kind}: axis {a}")
                assert np.isnan(want[0]).any() and (bits(want[0]) == 0).any()
        launched = profiled_calls(dev.lib, dev)
        dev.lib.profile_enable(dev.h, 0)
        assert launched.get("k_point_deskew", 0) == launched.get("k_range_decode_motion", 0) == launched.get("k_range_decode", 0) == 9, launched
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (c) the pipeline with the switch on
N_BATCH = 33


@pytest.fixture(scope="module")
def pair16(oracle, hip):
    """the warmed OS1-16 pair of tests/test_gpu_range_motion.py: 33 frames with body returns, a pose table per frame, the shifts of a
    destaggered image; `plain` = the rigid points the nodelet would hold, `comp` = the statement's points of them"""
    p = warmed_pair(oracle, hip, "os1-16", n_frames=N_BATCH, max_batch=N_BATCH)
    h_, w_ = p.shape[:2]
    inject_body_returns(p.frames)
    p.shift = rm.shifts("random", h_, w_, seed=7)
    p.dev.set_column_shift(p.shift)
    assert p.dev.set_point_motion(True) == capi.OK
    p.lo, p.hi = rm.exclude_bounds(p.dev.sp)
    p.tables = np.stack([rm.rigid_poses(w_, seed=f, yaw_rate=0.5 + 0.05 * f, v=(2.0, 0.1 * f, 0.0)) for f in range(N_BATCH)])  # one block: constant pitch
    p.plain = [decode_definition(s.range, *p.lut) for s in p.frames]
    p.comp = [pm.point_definition(*p.plain[f], p.tables[f], w_, p.lo, p.hi, p.shift)[:3] for f in range(N_BATCH)]
    p.block = np.stack([np.stack(q) for q in p.plain])  # [frame, axis, pixel]: packed x | y | z at a constant pitch
    p.mem = DeviceMem()
    yield p
    p.mem.free()


def ref_scan(p, f, compensated=True):
    x, y, z = (p.comp if compensated else p.plain)[f]
    s = p.frames[f]
    return ScanData(x=x, y=y, z=z, width=p.shape[1], height=p.shape[0], intensity=s.intensity, range=s.range)


def dev_scan(p, f, kind="point_motion", layout="block", table=None):
    """frame f as the HIP library gets it.  kind: point_motion / points (the rigid points, no poses) / range_motion / range.
    layout of a point scan: block (one numpy block per batch: the 2-D copy), columns (separate arrays), aos48 (the nodelet's structs,
    host), device48 (the same on the device), device (packed columns on the device)"""
    s = p.frames[f]
    h_, w_ = p.shape[:2]
    T = None if kind in ("points", "range") else (p.tables[f] if table is None else table)
    if kind in ("range_motion", "range"):
        return ScanData.range_image(s.range, w_, h_, intensity=s.intensity, col_tfs=T)
    x, y, z = p.plain[f]
    c = cloud(x, y, z, p.shape)
    if layout == "block":
        sd = ScanData(x=p.block[f, 0], y=p.block[f, 1], z=p.block[f, 2], width=w_, height=h_)
    elif layout == "columns":
        sd = ScanData(x=x.copy(), y=y.copy(), z=z.copy(), width=w_, height=h_)
    elif layout == "aos48":
        sd = host_scan(c, lay_aos48(c))
    elif layout == "device48":
        base = p.mem.put(lay_aos48(c)[0])
        sd = ScanData(x=base, y=base + 4, z=base + 8, width=w_, height=h_, stride_bytes=48, memspace=capi.MEM_DEVICE)
        T = None if T is None else p.mem.put(T, shift=4 * (f % 2))
    else:
        sd = ScanData(x=p.mem.put(x), y=p.mem.put(y), z=p.mem.put(z), width=w_, height=h_, memspace=capi.MEM_DEVICE)
        T = None if T is None else p.mem.put(T)
    sd.col_tfs = T
    return sd


def decode_launches(dev, scans, tfs):
    """(k_point_deskew, k_range_decode_motion, k_range_decode) launches of one synchronous and of one submitted batch: the same"""
    _, names = _profiled(dev, lambda: dev.process_batch(scans, tfs))
    dev.lib.profile_enable(dev.h, 1)
    try:
        dev.batch_collect(dev.batch_submit(scans, tfs))
        sub = profiled_calls(dev.lib, dev)
    finally:
        dev.lib.profile_enable(dev.h, 0)
    got = tuple(names.get(k, 0) for k in DECODES)
    assert got == tuple(sub.get(k, 0) for k in DECODES), (names, sub)
    return got, names


def batch_case(p, n, case, layout="block", rerun_ok=False):
    tfs = p.tfs[:n]
    scans_ref = [ref_scan(p, f) for f in range(n)]
    scans_dev = [dev_scan(p, f, layout=layout) for f in range(n)]
    frame_kernel = n >= 4  # (the frame kernel takes batches of four frames and more)
    three_views(p.ref, p.dev, scans_ref, scans_dev, tfs, "packed" if frame_kernel else "general", case, *FLOORS["os1-16"], expect_far=frame_kernel, rerun_ok=rerun_ok)
    got, names = decode_launches(p.dev, scans_dev, tfs)
    assert got == (1, 0, 0), names  # one launch per batch, whatever its size
    return names


@pytest.mark.parametrize("n", [1, 3, 4, 9, N_BATCH])
def test_batches_of_point_scans_with_poses(pair16, n):
    p = pair16
    assert all(np.isnan(c[0]).sum() >= 200 for c in p.comp[:n])  # (the body returns: NaN in every frame)
    assert np.abs(p.comp[0][0] - p.plain[0][0])[np.isfinite(p.comp[0][0])].max() > 0.05  # (the poses move the points)
    batch_case(p, n, f"point_motion/{n}", layout="block" if n != 3 else "columns")


@pytest.mark.parametrize("layout", ["aos48", "device48", "device"])
def test_struct_frames_with_poses_take_the_packed_frame_kernel(pair16, layout):
    """the nodelet's 48-byte structs, host (through the struct staging block) and device (read in place): k_point_deskew leaves packed
    columns, so the frame kernel's packed input pass runs - without poses the same frames take the strided one"""
    p = pair16
    names = batch_case(p, 9, f"point_motion/9/{layout}", layout=layout)
    if not _switches():  # (no environment switch reroutes the batch)
        assert "k_frame_lds_far" in names and "k_frame_lds_far_strided" not in names, names
        if layout != "device":
            _, plain = _profiled(p.dev, lambda: p.dev.process_batch([dev_scan(p, f, "points", layout) for f in range(9)], p.tfs[:9]))
            assert "k_frame_lds_far_strided" in plain and "k_point_deskew" not in plain, plain


def test_process_scan_with_and_without_map_update(oracle, hip):
    """single scans: read-only against the oracle on the warmed pair's recipe, then map-updating scans with maps compared"""
    ref, dev = make_pair(oracle, hip, "os1-16", 0.25, max_batch=1)
    try:
        warm_scene, scene, frames, col_tfs, shift = rm.moving_frames(n=3)
        rm.warm([ref, dev], warm_scene)
        dev.set_column_shift(shift)
        assert dev.set_point_motion(True) == capi.OK
        lo, hi = rm.exclude_bounds(dev.sp)
        h_, w_ = rm.SHAPES["os1_16"][:2]
        d = sim_directions("os1-16")
        T = np.ascontiguousarray(col_tfs, dtype=f32)
        dev.lib.profile_enable(dev.h, 1)
        n_det = 0
        for k, s in enumerate(frames):
            x, y, z = decode_definition(s.range, d, None)
            cx, cy, cz, _ = pm.point_definition(x, y, z, T, w_, lo, hi, shift)
            for flags in (capi.SCAN_NO_MAP_UPDATE, capi.SCAN_DEFAULT):
                want = ref.process_scan(ScanData(x=cx, y=cy, z=cz, width=w_, height=h_), s.tf, flags=flags)
                got = dev.process_scan(ScanData(x=x, y=y, z=z, width=w_, height=h_, col_tfs=T), s.tf, flags=flags)
                assert len(got) == len(want)
                for key in ("frame", "n_points"):
                    np.testing.assert_array_equal(got[key], want[key], err_msg=key)
                np.testing.assert_allclose(got["position"], want["position"], atol=1e-3)
                n_det += len(want)
            ma, mb = dev.read_map(capi.MAP_VOXELS), ref.read_map(capi.MAP_VOXELS)
            fin = np.isfinite(ma)
            np.testing.assert_array_equal(np.isfinite(mb), fin)
            np.testing.assert_allclose(ma[fin], mb[fin], rtol=1e-4, atol=1e-3)
            np.testing.assert_array_equal(dev.read_map(capi.MAP_FLAGS), ref.read_map(capi.MAP_FLAGS))
        ran = profiled_calls(dev.lib, dev)
        dev.lib.profile_enable(dev.h, 0)
        assert n_det > 0
        assert ran.get("k_point_deskew", 0) >= 2 * len(frames), ran  # (a scan that runs again stages again)
    finally:
        for det in (ref, dev):
            det.close()


def test_two_tickets_and_buffers_overwritten_behind_submit(pair16):
    p = pair16
    n = 9
    h_, w_ = p.shape[:2]
    tfs = p.tfs[:n]
    want, want_per = p.dev.process_batch([dev_scan(p, f) for f in range(n)], tfs)
    assert len(want) > 0

    def host_block():
        pts, tabs = p.block[:n].copy(), p.tables[:n].copy()
        return [ScanData(x=pts[f, 0], y=pts[f, 1], z=pts[f, 2], width=w_, height=h_, col_tfs=tabs[f]) for f in range(n)], [pts, tabs]

    def host_structs():
        scans = [dev_scan(p, f, layout="aos48", table=p.tables[f].copy()) for f in range(n)]
        return scans, [sd.keep for sd in scans] + [sd.col_tfs for sd in scans]

    def host_columns():  # separate arrays: no constant pitch
        scans = [dev_scan(p, f, layout="columns", table=p.tables[f].copy()) for f in range(n)]
        return scans, [a for sd in scans for a in (sd.x, sd.y, sd.z, sd.col_tfs)]

    for name, make in (("host_block", host_block), ("host_structs", host_structs), ("host_columns", host_columns)):
        tickets, owned = [], []
        for _ in range(2):  # two tickets in flight
            scans, bufs = make()
            tickets.append(p.dev.batch_submit(scans, tfs))
            for b in bufs:  # submit has returned: the host buffers are the caller's again
                b.view(np.uint8)[:] = 0xFF
            owned.append((scans, bufs))
        for t in tickets:
            got, per = p.dev.batch_collect(t)
            same_detections(got, want, name)
            np.testing.assert_array_equal(per, want_per)
        scans, bufs = make()
        got, per = p.dev.process_batch(scans, tfs)
        same_detections(got, want, name + "/sync")


# ------------------------------------------------------------------------------------------------ (d) mixed batches
def test_mixed_batches_of_all_four_kinds(pair16):
    """point scans with poses, plain point scans, compensated range images and plain ones in one batch: each frame's result is its
    own, each decode kernel runs once.  full: max_batch frames, alternating - every entry of both job lists' share is taken"""
    p = pair16
    four = ["point_motion", "points", "range_motion", "range"]
    cases = {"all_four": (9, four, (1, 1, 1)), "full": (N_BATCH, four, (1, 1, 1)), "full_two": (N_BATCH, ["range_motion", "point_motion"], (1, 1, 0)),
             "poses_and_plain_points": (9, ["points", "point_motion"], (1, 0, 0)), "no_point_poses": (9, ["points", "range_motion", "range"], (0, 1, 1)), "plain_points": (9, ["points"], (0, 0, 0))}
    for name, (n, cyc, want_launches) in cases.items():
        tfs = p.tfs[:n]
        ks = [cyc[f % len(cyc)] for f in range(n)]
        scans_ref = [ref_scan(p, f, compensated=ks[f] in ("point_motion", "range_motion")) for f in range(n)]
        scans_dev = [dev_scan(p, f, ks[f], layout="columns") for f in range(n)]
        three_views(p.ref, p.dev, scans_ref, scans_dev, tfs, "packed", f"point_motion/mixed/{name}", *FLOORS["os1-16"])
        got, names = decode_launches(p.dev, scans_dev, tfs)
        assert got == want_launches, (name, names)


# ------------------------------------------------------------------------------------------------ (e) under each production fallback
@pytest.mark.parametrize("fallback", ["VOFOD_CLOSE_FIRST=0", "VOFOD_DEVICE_TAIL=0", "VOFOD_LDS_MAX_BRICKS=4096"])
def test_batch_under_each_production_fallback(pair16, fallback, monkeypatch):
    k, v = fallback.split("=")
    monkeypatch.setenv(k, v)
    batch_case(pair16, 9, f"point_motion/9/{fallback}", rerun_ok=(k == "VOFOD_LDS_MAX_BRICKS"))


# ------------------------------------------------------------------------------------------------ (f) VOFOD_SCAN_AUTO_RAYCAST
@pytest.mark.parametrize("ray_motion", [False, True], ids=["rigid_rays", "compensated_rays"])
def test_auto_raycast_on_point_scans_with_poses(hip, ray_motion):
    """exact accumulation on, so the passes compare as equalities.  Raycast motion off: the raycast map is that of the same scans
    without col_tfs.  On: it is that of vofod_raycast_begin on the same scan.  Host and device-resident scans take turns."""
    a, b = make_pair(hip, hip, "os1-16", 0.25, max_batch=1)
    mem = DeviceMem()
    try:
        warm_scene, scene, frames, col_tfs, shift = rm.moving_frames(n=3)
        rm.warm([a, b], warm_scene)
        h_, w_ = rm.SHAPES["os1_16"][:2]
        T = np.ascontiguousarray(col_tfs, dtype=f32)
        d = sim_directions("os1-16")
        for det in (a, b):
            det.set_column_shift(shift)
            assert det.set_raycast_exact(True) == capi.OK and det.set_raycast_motion(ray_motion) == capi.OK and det.set_point_motion(True) == capi.OK
        a.lib.profile_enable(a.h, 1)
        n_begun = 0
        for k, s in enumerate(frames):
            x, y, z = decode_definition(s.range, d, None)
            host = ScanData(x=x, y=y, z=z, width=w_, height=h_, intensity=s.intensity, range=s.range, col_tfs=T)
            if k == 2:
                auto = ScanData(x=mem.put(x), y=mem.put(y), z=mem.put(z), width=w_, height=h_, intensity=mem.put(s.intensity), range=mem.put(s.range), memspace=capi.MEM_DEVICE, col_tfs=mem.put(T))
            else:
                auto = host
            da = a.process_scan(auto, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
            if ray_motion:
                # the explicit calls AUTO stands for: the scan, then finish the pending pass or begin one with this very scan
                db = b.process_scan(host, s.tf)
                if b.status().raycast_pending:
                    assert b.raycast_finish() == capi.OK
                else:
                    assert b.raycast_begin(host, s.tf) == capi.OK
            else:
                # the same scans without col_tfs (rigid points, rigid rays): the points differ, the rays must not
                db = b.process_scan(ScanData(x=x, y=y, z=z, width=w_, height=h_, intensity=s.intensity, range=s.range), s.tf, flags=capi.SCAN_AUTO_RAYCAST)
            ta, tb = a.status(), b.status()
            assert (ta.raycast_pending, ta.detection_its) == (tb.raycast_pending, tb.detection_its)
            if ray_motion:
                same_detections(da, db, f"scan {k}")
            if ta.raycast_pending:
                (ua, sa), (ub, sb) = a.raycast_units(), b.raycast_units()
                assert sa == sb and np.count_nonzero(ua) > 10_000
                np.testing.assert_array_equal(ua, ub, err_msg=f"scan {k}: units of the pending pass")
                n_begun += 1
        ran = profiled_calls(a.lib, a)
        a.lib.profile_enable(a.h, 0)
        assert n_begun == 2, n_begun
        assert ran.get("k_point_deskew", 0) >= len(frames) and ran.get("k_raycast_exact", 0) == 2, ran
    finally:
        mem.free()
        for det in (a, b):
            det.close()


# ------------------------------------------------------------------------------------------------ (g) the switch and the errors
def scan_status(dev, sd, how, tfa, n_px):
    cs = sd.as_c()
    n_out, dets = C.c_size_t(0), np.zeros(64, dtype=capi.DETECTION)
    if how == "submit":
        ticket = C.c_int(-1)
        st = dev.lib.batch_submit(dev.h, C.byref(cs), capi.ptr(tfa), 1, C.byref(ticket))
        if st == capi.OK:
            assert dev.lib.batch_collect(dev.h, ticket.value, capi.ptr(dets), 64, None, C.byref(n_out)) == capi.OK
        return st
    if how == "batch":
        per = np.zeros(1, dtype=np.uint32)
        return dev.lib.process_batch(dev.h, C.byref(cs), capi.ptr(tfa), 1, capi.ptr(dets), 64, capi.ptr(per), C.byref(n_out), None)
    if how == "scan":
        return dev.lib.process_scan(dev.h, C.byref(cs), capi.ptr(tfa), capi.SCAN_NO_MAP_UPDATE, capi.ptr(dets), 64, C.byref(n_out), None)
    out = [np.zeros(n_px, dtype=f32) for _ in range(3)]
    fn = dev.lib.range_to_points if how == "r2p" else dev.lib.deskew_points
    return fn(dev.h, C.byref(cs), *(capi.ptr(a) for a in out), capi.MEM_HOST)


def test_switch_and_error_returns(pair16):
    p = pair16
    dev = p.dev
    h_, w_ = p.shape[:2]
    n_px = h_ * w_
    s = p.frames[0]
    T = p.tables[0]
    tfa = np.ascontiguousarray(s.tf, dtype=f32).reshape(12)
    x, y, z = p.plain[0]
    point_scan = ScanData(x=x, y=y, z=z, width=w_, height=h_, range=s.range, col_tfs=T)
    mem = DeviceMem()
    try:
        # off: INVALID_ARG on all routes, vofod_deskew_points needs no switch
        assert dev.set_point_motion(False) == capi.OK
        for how in ("scan", "batch", "submit", "r2p"):
            assert scan_status(dev, point_scan, how, tfa, n_px) == capi.ERR_INVALID_ARG, how
        assert scan_status(dev, point_scan, "deskew", tfa, n_px) == capi.OK
        # on: the three per-scan routes accept it, vofod_range_to_points stays range-image only
        assert dev.set_point_motion(True) == capi.OK
        for how in ("scan", "batch", "submit"):
            assert scan_status(dev, point_scan, how, tfa, n_px) == capi.OK, how
        assert scan_status(dev, point_scan, "r2p", tfa, n_px) == capi.ERR_INVALID_ARG
        # BUSY while a ticket is pending, and nothing changed afterwards
        scans4 = [dev_scan(p, f) for f in range(4)]
        want, _ = dev.process_batch(scans4, p.tfs[:4])
        t = dev.batch_submit(scans4, p.tfs[:4])
        assert dev.set_point_motion(False, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
        got, _ = dev.batch_collect(t)
        same_detections(got, want, "in flight")
        got, _ = dev.process_batch(scans4, p.tfs[:4])  # (still on: the refused call changed nothing)
        same_detections(got, want, "the refused switch changed nothing")
        assert dev.lib.set_point_motion(None, 1) == capi.ERR_INVALID_ARG
        # vofod_deskew_points: its refusals
        d_cols = [mem.put(v) for v in (x, y, z)]
        d_tab = mem.put(T, shift=4)
        on_device = lambda **kw: ScanData(**{**dict(x=d_cols[0], y=d_cols[1], z=d_cols[2], width=w_, height=h_, memspace=capi.MEM_DEVICE, col_tfs=d_tab), **kw})  # noqa: E731
        assert scan_status(dev, on_device(), "deskew", tfa, n_px) == capi.OK  # (the converse)
        assert scan_status(dev, ScanData.range_image(s.range, w_, h_, col_tfs=T), "deskew", tfa, n_px) == capi.ERR_INVALID_ARG  # a range image
        assert scan_status(dev, ScanData(x=x, y=y, z=z, width=w_, height=h_), "deskew", tfa, n_px) == capi.ERR_INVALID_ARG  # no col_tfs
        for off in (1, 2, 3):
            assert scan_status(dev, on_device(col_tfs=d_tab + off), "deskew", tfa, n_px) == capi.ERR_INVALID_ARG, off
            assert scan_status(dev, on_device(x=d_cols[0] + off), "deskew", tfa, n_px) == capi.ERR_INVALID_ARG, off
            assert scan_status(dev, on_device(z=d_cols[2] + off), "deskew", tfa, n_px) == capi.ERR_INVALID_ARG, off
            for how in ("scan", "batch", "submit"):  # the same rules on the per-scan routes
                assert scan_status(dev, on_device(col_tfs=d_tab + off), how, tfa, n_px) == capi.ERR_INVALID_ARG, (off, how)
                assert scan_status(dev, on_device(y=d_cols[1] + off), how, tfa, n_px) == capi.ERR_INVALID_ARG, (off, how)
        assert scan_status(dev, on_device(stride_bytes=6), "deskew", tfa, n_px) == capi.ERR_INVALID_ARG
        assert scan_status(dev, ScanData(x=x, y=y, z=z, width=w_ // 2, height=h_, col_tfs=T), "deskew", tfa, n_px) == capi.ERR_SIZE_MISMATCH
        assert scan_status(dev, ScanData(x=x, y=y, z=z, width=w_, height=h_ + 1, col_tfs=T), "deskew", tfa, n_px) == capi.ERR_SIZE_MISMATCH
        # one bad frame refuses a whole batch
        arr = (capi.Scan * 2)(dev_scan(p, 0).as_c(), on_device(col_tfs=d_tab + 2).as_c())
        tf2 = np.ascontiguousarray(p.tfs[:2], dtype=f32)
        ticket = C.c_int(-1)
        assert dev.lib.batch_submit(dev.h, arr, capi.ptr(tf2), 2, C.byref(ticket)) == capi.ERR_INVALID_ARG and ticket.value == -1
        got, _ = dev.process_batch(scans4, p.tfs[:4])
        same_detections(got, want, "after the refusals")
    finally:
        mem.free()
        dev.set_point_motion(True)


def test_switch_survives_reset_map_shift_and_map_apply(hip):
    shape = pm.SHAPES["4x18"]
    h_, w_ = shape[:2]
    dev = hip_detector(hip, shape, (sim_directions(shape), None))
    try:
        rs = np.random.default_rng(3)
        x, y, z = (rs.uniform(5.0, 30.0, h_ * w_).astype(f32) for _ in range(3))
        sd = ScanData(x=x, y=y, z=z, width=w_, height=h_, col_tfs=rm.general_poses(w_, seed=3))
        tf = np.eye(3, 4, dtype=f32)
        tfa = np.ascontiguousarray(tf).reshape(12)
        assert scan_status(dev, sd, "scan", tfa, h_ * w_) == capi.ERR_INVALID_ARG  # off after creation
        assert dev.set_point_motion(True) == capi.OK
        snapshot = dev.export_map()
        for step in (dev.reset, lambda: dev.apply_map(snapshot), lambda: dev.map_shift([1, 0, 0], [40.0 + float(dev.sp.voxel_size), 20.0, -1.25])):
            step()
            assert scan_status(dev, sd, "scan", tfa, h_ * w_) == capi.OK
        assert dev.set_point_motion(False) == capi.OK
        assert scan_status(dev, sd, "scan", tfa, h_ * w_) == capi.ERR_INVALID_ARG
    finally:
        dev.close()
