"""Motion-compensated rays on the GPU (include/vofod.h, MOTION-COMPENSATED RAYS; vofod_set_raycast_motion; k_raycast_t<MOTION = true, ...> in
vofod_amd/csrc/kernels_raycast.h, launched as k_raycast_motion).  All cases share one small operation area (24 x 24 x 12 m at 0.5 m: rays leave the map, start
inside it, and are clipped) and the small sensors of range_motion_cases.SHAPES - 5x20 (n = 100: one partial block, one wave that
spans all rows), 3x21 (n = 63, odd width), OS1-16 (64 blocks) - with the three shift kinds (the wrap of m).

(a) identity table, switch on, against the switch off on the same handle and scan: the motion front against the rigid one (one walk);
(b) quarter-turn tables against the sum of the oracle's gated rigid passes (raycast_motion_cases.oracle_quarter_sum), every input form;
(c) rigid tables with real translation and rotation against the float64 geometry statement;
(d) the switch as a handle property, and the argument rules;  (e) the sensor stream under VOFOD_SCAN_AUTO_RAYCAST (plumbing)."""
import ctypes as C
import os

import numpy as np
import pytest

from vofod_amd import capi
from vofod_amd.detector import ScanData

import range_motion_cases as rm
import raycast_motion_cases as rc
import statements
from helpers import make_pair
from test_gpu_range_image import LUTS, DeviceMem
from test_gpu_stream_route import profiled_calls

pytestmark = pytest.mark.gpu
if os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"):
    pytest.skip("oracle against oracle: the oracle has no motion input", allow_module_level=True)

f32 = np.float32
RAY_RTOL, RAY_ATOL = 2e-5, 2e-6  # the helpers' raycast tolerance: the order of the float atomics
SHAPE_NAMES = ("5x20", "3x21", "os1_16")
LUT_KINDS = ("offsets_28mm_36mm", "simulated")  # with and without beam offsets


def one_pass(dev, sd, tf):
    """raycast map of one vofod_raycast_begin (float64, flat); the pass is closed again"""
    assert dev.raycast_begin(sd, tf) == capi.OK
    got = dev.read_map(capi.MAP_RAYCAST).astype(np.float64).reshape(-1)
    assert dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
    return got


def launches(dev):
    return profiled_calls(dev.lib, dev)


def assert_same_pass(got, want, what):
    np.testing.assert_array_equal(got != 0, want != 0, err_msg=f"{what}: support")
    np.testing.assert_allclose(got, want, rtol=RAY_RTOL, atol=RAY_ATOL, err_msg=what)


def host_scan(c, shape, table=None):
    return ScanData.range_image(c.range, shape[1], shape[0], intensity=c.intensity, col_tfs=None if table is None else np.ascontiguousarray(table, dtype=f32))


def device_scan(mem, c, shape, table, shift=0):
    d_tab = mem.put(np.ascontiguousarray(table, dtype=f32), shift=shift)
    assert d_tab % 16 == shift
    return ScanData.range_image(mem.put(c.range), shape[1], shape[0], intensity=mem.put(c.intensity), memspace=capi.MEM_DEVICE, col_tfs=d_tab)


# ------------------------------------------------------------------------------------------------ (a) identity table against k_raycast
@pytest.mark.parametrize("shift_kind", rm.SHIFTS)
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_identity_table_casts_the_rigid_rays(hip, shape_name, shift_kind):
    shape = rm.SHAPES[shape_name]
    h_, w_ = shape[:2]
    c = rc.small_case(shape, seed=h_ * w_)
    dev = rc.detector(hip, shape, LUTS["offsets_28mm_36mm"](hip, shape), mask=c.mask)
    try:
        dev.set_column_shift(rm.shifts(shift_kind, h_, w_, seed=3))
        sd = host_scan(c, shape, rm.identity_poses(w_))
        dev.lib.profile_enable(dev.h, 1)
        assert dev.set_raycast_motion(True) == capi.OK
        on = one_pass(dev, sd, c.tf)
        first = launches(dev)
        assert dev.set_raycast_motion(False) == capi.OK
        off = one_pass(dev, sd, c.tf)
        second = launches(dev)
        dev.lib.profile_enable(dev.h, 0)
        assert first.get("k_raycast_motion", 0) == 1 and "k_raycast" not in first, first
        assert second.get("k_raycast", 0) == 1 and "k_raycast_motion" not in second, second
        assert np.count_nonzero(off) > 50
        assert_same_pass(on, off, f"{shape_name}/{shift_kind}: identity table against the rigid pass")
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (b) quarter turns against the oracle
@pytest.mark.parametrize("lut_kind", LUT_KINDS)
@pytest.mark.parametrize("shift_kind", rm.SHIFTS)
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_quarter_turn_tables_against_the_oracle_sum(oracle, hip, shape_name, shift_kind, lut_kind):
    """a transposed pose read, a wrong m, a wrong shift direction or a missing wrap each change the support"""
    shape = rm.SHAPES[shape_name]
    h_, w_ = shape[:2]
    c = rc.small_case(shape, seed=h_ * w_ + 1)
    assert c.n_gate_int > 0 and c.n_gate_mask > 0  # both gates drop rays
    lut = LUTS[lut_kind](hip, shape)
    shift = rm.shifts(shift_kind, h_, w_, seed=4)
    k_of_m, table = rc.quarter_table(w_, seed=h_)
    ref = rc.detector(oracle, shape, lut, mask=c.mask)
    dev = rc.detector(hip, shape, lut, mask=c.mask)
    mem = DeviceMem()
    try:
        want = rc.oracle_quarter_sum(ref, k_of_m, w_, shift, c.intensity, c.range, c.tf)
        assert np.count_nonzero(want) > 50
        dev.set_column_shift(shift)
        dev.set_raycast_motion(True)
        dev.lib.profile_enable(dev.h, 1)
        forms = {"host": host_scan(c, shape, table), "device16": device_scan(mem, c, shape, table), "device+4": device_scan(mem, c, shape, table, shift=4)}
        for name, sd in forms.items():
            got = one_pass(dev, sd, c.tf)
            assert_same_pass(got, want, f"{shape_name}/{shift_kind}/{lut_kind}/{name}")
        ran = launches(dev)
        dev.lib.profile_enable(dev.h, 0)
        assert ran.get("k_raycast_motion", 0) == len(forms) and "k_raycast" not in ran, ran
        # the gates: without them the map would differ (every gated pixel is a ray the ungated pass casts)
        rigid = one_pass(ref, ScanData(x=np.zeros(h_ * w_, dtype=f32), y=np.zeros(h_ * w_, dtype=f32), z=np.zeros(h_ * w_, dtype=f32), width=w_, height=h_, intensity=c.intensity, range=c.range), c.tf)
        assert not np.allclose(rigid, want, rtol=RAY_RTOL, atol=RAY_ATOL)  # (and the table moves the rays)
    finally:
        mem.free()
        for d in (ref, dev):
            d.close()


# ------------------------------------------------------------------------------------------------ (c) rigid tables against the geometry
TABLES = {
    "rigid_poses": lambda w: rm.rigid_poses(w, seed=w),                     # a tilted axis, 1 rad/s, 3 m/s
    "twist": lambda w: rm.twist_col_tfs(w, yaw_rate=1.0, v=(3.0, 0.5, -0.2)),  # the moving sensor of range_motion_cases
}


@pytest.mark.parametrize("table_kind", list(TABLES))
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_rigid_tables_against_the_geometry_statement(hip, shape_name, table_kind):
    """real translation and rotation: the pass against segment / voxel geometry in float64 of the rays d', o' (no DDA, no product
    code), with the tolerances of the whole-scan raycast statement + the implementation's (float atomics)"""
    shape = rm.SHAPES[shape_name]
    h_, w_ = shape[:2]
    c = rc.small_case(shape, seed=h_ * w_ + 2)
    lut = LUTS["offsets_28mm_36mm"](hip, shape)
    shift = rm.shifts("random", h_, w_, seed=6)
    table = TABLES[table_kind](w_)
    assert np.abs(table[:, :, 3]).max() > 0.05 and np.abs(table[0, :, :3] - np.eye(3)).max() > 0.01
    dev = rc.detector(hip, shape, lut, mask=c.mask)
    try:
        dev.set_column_shift(shift)
        dev.set_raycast_motion(True)
        got = one_pass(dev, host_scan(c, shape, table), c.tf)
        dm, om = rc.ray_definition(lut[0], lut[1], table, w_, shift)
        want, n_cast = rc.geometry_statement(dev, dev.dp, c.tf, dm, om, c.mask, c.intensity, c.range)
        assert n_cast > 0.4 * h_ * w_ and np.count_nonzero(want) > 50
        rc.assert_pass_matches_statement(got, want, statements.Tol(ray_rtol=RAY_RTOL, ray_atol=RAY_ATOL), what=f"{shape_name}/{table_kind} against the geometry statement")
        # the rigid rays of the same scan are another map
        dev.set_raycast_motion(False)
        rigid = one_pass(dev, host_scan(c, shape, table), c.tf)
        assert np.abs(rigid - want).max() > 0.05
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (d) the switch and the argument rules
def test_switch_is_a_handle_property_and_argument_rules(hip):
    shape = rm.SHAPES["5x20"]
    h_, w_ = shape[:2]
    n = h_ * w_
    c = rc.small_case(shape, seed=9)
    lut = LUTS["offsets_28mm_36mm"](hip, shape)
    table = np.ascontiguousarray(rm.twist_col_tfs(w_, yaw_rate=1.0, v=(3.0, 0.0, 0.0)), dtype=f32)
    dev = rc.detector(hip, shape, lut, mask=c.mask, max_batch=2)
    mem = DeviceMem()
    try:
        dev.set_column_shift(rm.shifts("random", h_, w_, seed=9))
        with_tab, without = host_scan(c, shape, table), host_scan(c, shape)
        # off (the state after vofod_create): col_tfs is ignored - the scan without the table
        dev.lib.profile_enable(dev.h, 1)
        rigid = one_pass(dev, without, c.tf)
        assert_same_pass(one_pass(dev, with_tab, c.tf), rigid, "switch off: col_tfs ignored")
        ran = launches(dev)
        assert ran.get("k_raycast", 0) == 2 and "k_raycast_motion" not in ran, ran
        # on: another map for the scan with the table, the same launch as ever for the scan without
        assert dev.lib.set_raycast_motion(dev.h, 7) == capi.OK  # (`on` is taken as on != 0)
        moved = one_pass(dev, with_tab, c.tf)
        assert np.abs(moved - rigid).max() > 0.05
        assert_same_pass(one_pass(dev, without, c.tf), rigid, "switch on, scan without col_tfs")
        ran = launches(dev)
        assert ran.get("k_raycast", 0) == 1 and ran.get("k_raycast_motion", 0) == 1, ran
        # kept across vofod_reset and vofod_map_shift
        dev.reset()
        assert_same_pass(one_pass(dev, with_tab, c.tf), moved, "after vofod_reset")
        vs = float(dev.sp.voxel_size)
        o = rc.SMALL_AREA[0]
        dev.map_shift([1, 0, 0], [o[0] + vs, o[1], o[2]])
        one_pass(dev, with_tab, c.tf)
        dev.map_shift([-1, 0, 0], list(o))
        assert_same_pass(one_pass(dev, with_tab, c.tf), moved, "after vofod_map_shift there and back")
        ran = launches(dev)
        assert ran.get("k_raycast_motion", 0) == 3 and "k_raycast" not in ran, ran
        dev.lib.profile_enable(dev.h, 0)
        # VOFOD_ERR_BUSY while a pass is pending, and the switch keeps its state
        assert dev.raycast_begin(with_tab, c.tf) == capi.OK
        for on in (False, True):
            assert dev.set_raycast_motion(on, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
        got = dev.read_map(capi.MAP_RAYCAST).astype(np.float64).reshape(-1)
        assert dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
        assert_same_pass(got, moved, "the pass behind the refused calls")
        # ... and while a submitted batch is pending
        tfs = np.stack([c.tf, c.tf])
        ticket = dev.batch_submit([without, without], tfs)
        assert dev.set_raycast_motion(False, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
        dev.batch_collect(ticket)
        assert dev.set_raycast_motion(True) == capi.OK
        assert dev.lib.set_raycast_motion(None, 1) == capi.ERR_INVALID_ARG
        # a device-resident table off 4 bytes: refused, nothing pending afterwards; the converse is accepted
        d_rng, d_int, d_tab = mem.put(c.range), mem.put(c.intensity), mem.put(table, shift=4)
        for off in (1, 2, 3):
            bad = ScanData.range_image(d_rng, w_, h_, intensity=d_int, memspace=capi.MEM_DEVICE, col_tfs=d_tab + off)
            assert dev.raycast_begin(bad, c.tf, allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG
            assert not dev.status().raycast_pending
        assert_same_pass(one_pass(dev, ScanData.range_image(d_rng, w_, h_, intensity=d_int, memspace=capi.MEM_DEVICE, col_tfs=d_tab), c.tf), moved, "device table at +4 bytes")
        # a point scan with col_tfs: the raycast role takes it (it reads range and intensity only), vofod_process_scan refuses it
        xyz = [np.zeros(n, dtype=f32) for _ in range(3)]
        point_scan = ScanData(x=xyz[0], y=xyz[1], z=xyz[2], width=w_, height=h_, intensity=c.intensity, range=c.range, col_tfs=table)
        assert_same_pass(one_pass(dev, point_scan, c.tf), moved, "point scan with col_tfs")
        dets = np.zeros(4, dtype=capi.DETECTION)
        cs, n_out, tfa = point_scan.as_c(), C.c_size_t(0), np.ascontiguousarray(c.tf, dtype=f32).reshape(12)
        assert dev.lib.process_scan(dev.h, C.byref(cs), capi.ptr(tfa), capi.SCAN_DEFAULT, capi.ptr(dets), 4, C.byref(n_out), None) == capi.ERR_INVALID_ARG
    finally:
        mem.free()
        dev.close()


# ------------------------------------------------------------------------------------------------ (e) the sensor stream (plumbing)
def test_sensor_stream_with_auto_raycast_casts_the_compensated_rays(hip):
    """four scans of the moving sensor through VOFOD_SCAN_AUTO_RAYCAST with the switch on, against the same scans through
    vofod_process_scan(DEFAULT) followed by the explicit raycast call AUTO emulates (finish the pending pass, else begin one for this
    scan) on a second HIP handle.  Host and device-resident scans take turns on the AUTO side: a host table reaches the raycast role
    through the pose block the decode staged it in, a device table is read in place.  The pass itself is pinned by (b) and (c)."""
    a, b = make_pair(hip, hip, "os1-16", 0.25, max_batch=1)
    mem = DeviceMem()
    try:
        warm_scene, scene, frames, col_tfs, shift = rm.moving_frames(n=4)
        rm.warm([a, b], warm_scene)
        h_, w_ = rm.SHAPES["os1_16"][:2]
        col_tfs = np.ascontiguousarray(col_tfs, dtype=f32)
        for d in (a, b):
            d.set_column_shift(shift)
            assert d.set_raycast_motion(True) == capi.OK
        a.lib.profile_enable(a.h, 1)
        n_det = n_begun = 0
        for k, s in enumerate(frames):
            host = ScanData.range_image(s.range, w_, h_, intensity=s.intensity, col_tfs=col_tfs)
            on_device = ScanData.range_image(mem.put(s.range), w_, h_, intensity=mem.put(s.intensity), memspace=capi.MEM_DEVICE, col_tfs=mem.put(col_tfs))
            da = a.process_scan(on_device if k == 2 else host, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
            db = b.process_scan(host, s.tf)
            if b.status().raycast_pending:
                assert b.raycast_finish() == capi.OK
            else:
                assert b.raycast_begin(host, s.tf) == capi.OK
                n_begun += 1
            # the tolerances of test_gpu_stream_route.compare_cycle
            assert len(da) == len(db)
            for key in ("id", "frame", "n_points"):
                np.testing.assert_array_equal(da[key], db[key], err_msg=key)
            np.testing.assert_allclose(da["position"], db["position"], atol=1e-3)
            np.testing.assert_allclose(da["confidence"], db["confidence"], rtol=1e-4, atol=1e-300)
            np.testing.assert_allclose(da["detection_probability"], db["detection_probability"], rtol=1e-5)
            ta, tb = a.status(), b.status()
            assert (ta.raycast_pending, ta.detection_its) == (tb.raycast_pending, tb.detection_its)
            ma, mb = a.read_map(capi.MAP_VOXELS), b.read_map(capi.MAP_VOXELS)
            fin = np.isfinite(ma)
            np.testing.assert_array_equal(np.isfinite(mb), fin)
            np.testing.assert_allclose(ma[fin], mb[fin], rtol=1e-4, atol=1e-3)
            np.testing.assert_array_equal(a.read_map(capi.MAP_FLAGS), b.read_map(capi.MAP_FLAGS))
            np.testing.assert_allclose(a.read_map(capi.MAP_RAYCAST), b.read_map(capi.MAP_RAYCAST), rtol=RAY_RTOL, atol=RAY_ATOL)
            if ta.raycast_pending:
                assert np.count_nonzero(a.read_map(capi.MAP_RAYCAST)) > 10_000
            n_det += len(da)
        ran = launches(a)
        a.lib.profile_enable(a.h, 0)
        print(f"raycast motion/stream: detections {n_det}, passes begun {n_begun}, launches {ran}")
        assert n_begun == 2
        assert ran.get("k_raycast_motion", 0) >= 2 and "k_raycast" not in ran, ran
        assert ran.get("k_ray_sweep", 0) >= 2 and ran.get("k_range_decode_motion", 0) >= len(frames), ran
    finally:
        mem.free()
        for d in (a, b):
            d.close()
