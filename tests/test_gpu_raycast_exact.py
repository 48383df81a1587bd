"""Exact raycast accumulation on the GPU (include/vofod.h, EXACT RAYCAST ACCUMULATION; vofod_set_raycast_exact, vofod_raycast_units;
the AccUnits policy of k_raycast_t / k_ray_sweep_t in vofod_amd/csrc/kernels_raycast.h, launched as k_raycast_exact / k_ray_sweep_exact).  The small operation area and sensors of
raycast_motion_cases / range_motion_cases.SHAPES: 5x20 (one partial block, one wave over all rows), 3x21 (odd width), OS1-16 with only
rows 3 and 11 above the intensity gate (2 x 1024 consecutive pixels: full waves, long merge runs).

(1) the units against the oracle one ray at a time, bit for bit;  (2) order and partition on the device alone;  (3) the float view;
(4) the sweep against the voxelwise formula;  (5) with motion-compensated rays;  (6) the clamp by hand;  (7) the switch's rules;
(8) the sensor stream, replicas and snapshots."""
import os

import numpy as np
import pytest

from vofod_amd import capi, synth
from vofod_amd.detector import ScanData

import range_motion_cases as rm
import raycast_exact_cases as rx
import raycast_motion_cases as rc
import statements
from helpers import make_pair
from test_gpu_range_image import LUTS, DeviceMem
from test_gpu_stream_route import profiled_calls

pytestmark = pytest.mark.gpu
if os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"):
    pytest.skip("oracle against oracle: the oracle has no exact accumulation", allow_module_level=True)

f32 = np.float32
LUT_KINDS = ("offsets_28mm_36mm", "simulated")  # with and without beam offsets
RAY_MAPS = (1 << capi.MAP_FLAGS) | (1 << capi.MAP_RAYCAST)


def host_scan(c, intensity=None, table=None):
    return ScanData.range_image(c.range, c.w, c.h, intensity=c.intensity if intensity is None else intensity,
                                col_tfs=None if table is None else np.ascontiguousarray(table, dtype=f32))


def device_scan(mem, c, table=None, shift=0):
    d_tab = None
    if table is not None:
        d_tab = mem.put(np.ascontiguousarray(table, dtype=f32), shift=shift)
        assert d_tab % 16 == shift
    return ScanData.range_image(mem.put(c.range), c.w, c.h, intensity=mem.put(c.intensity), memspace=capi.MEM_DEVICE, col_tfs=d_tab)


def exact_pass(dev, sd, tf, view=False):
    """(U int64 flat, S) of one exact vofod_raycast_begin [, the float view read before the pass is closed]; the pass is abandoned"""
    assert dev.raycast_begin(sd, tf) == capi.OK
    u, s = dev.raycast_units()
    r = dev.read_map(capi.MAP_RAYCAST).reshape(-1) if view else None
    assert dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
    u = u.reshape(-1).astype(np.int64)
    return (u, s, r) if view else (u, s)


def gated(c, keep):
    """the case's intensities with every pixel outside `keep` below the gate"""
    return np.where(keep, c.intensity, f32(rc.MIN_INTENSITY) - f32(1.0)).astype(f32)


# ------------------------------------------------------------------------------------------------ (1) units, bit for bit
@pytest.mark.parametrize("lut_kind", LUT_KINDS)
@pytest.mark.parametrize("shape_name", rx.SHAPE_NAMES)
def test_units_are_the_single_ray_yardstick_bit_for_bit(oracle, hip, shape_name, lut_kind):
    lut = LUTS[lut_kind](hip, rm.SHAPES[shape_name])
    c, y = rx.yardstick(oracle, shape_name, lut_kind, lut)
    dev = rc.detector(hip, c.shape, lut, mask=c.mask, vs=rx.VS)
    mem = DeviceMem()
    try:
        assert dev.set_raycast_exact(True) == capi.OK
        dev.lib.profile_enable(dev.h, 1)
        forms = {"host": host_scan(c), "device": device_scan(mem, c)}
        for name, sd in forms.items():
            u, s = exact_pass(dev, sd, c.tf)
            assert s == y.s == rx.scale_rule(c.h * c.w, rx.VS)[0]
            np.testing.assert_array_equal(u, y.units, err_msg=f"{shape_name}/{lut_kind}/{name}")
        ran = profiled_calls(dev.lib, dev)
        dev.lib.profile_enable(dev.h, 0)
        assert ran.get("k_raycast_exact", 0) == len(forms) and "k_raycast" not in ran and "k_raycast_motion" not in ran, ran
        assert np.count_nonzero(y.units) > 100
    finally:
        mem.free()
        dev.close()


# ------------------------------------------------------------------------------------------------ (2) order and partition
@pytest.mark.parametrize("shape_name", ("5x20", "os1_16"))
def test_units_add_over_any_partition_of_the_rays(hip, shape_name):
    """the device alone: U(all) == U(even columns) + U(odd columns) == the sum of the per-row passes, and two passes of one scan are
    identical - other lanes share a wave, other runs are merged, other atomics meet (the oracle's float halves of the 5x20 case differ
    from its full pass: tests/test_raycast_exact_cpu.py)"""
    c = rx.case(shape_name)
    lut = LUTS["offsets_28mm_36mm"](hip, c.shape)
    dev = rc.detector(hip, c.shape, lut, mask=c.mask, vs=rx.VS)
    try:
        dev.set_raycast_exact(True)
        row, col = np.divmod(np.arange(c.h * c.w), c.w)
        full, _ = exact_pass(dev, host_scan(c), c.tf)
        again, _ = exact_pass(dev, host_scan(c), c.tf)
        np.testing.assert_array_equal(again, full)
        assert np.count_nonzero(full) > 100
        even, _ = exact_pass(dev, host_scan(c, gated(c, col % 2 == 0)), c.tf)
        odd, _ = exact_pass(dev, host_scan(c, gated(c, col % 2 == 1)), c.tf)
        assert even.any() and odd.any()
        np.testing.assert_array_equal(even + odd, full)
        rows = np.zeros_like(full)
        n_rows = 0
        for r in range(c.h):
            u, _ = exact_pass(dev, host_scan(c, gated(c, row == r)), c.tf)
            n_rows += bool(u.any())
            rows += u
        assert n_rows >= 2
        np.testing.assert_array_equal(rows, full)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (3) the float view
@pytest.mark.parametrize("shape_name", rx.SHAPE_NAMES)
def test_float_view_is_the_converted_units(oracle, hip, shape_name):
    lut = LUTS["offsets_28mm_36mm"](hip, rm.SHAPES[shape_name])
    c, y = rx.yardstick(oracle, shape_name, "offsets_28mm_36mm", lut)
    dev = rc.detector(hip, c.shape, lut, mask=c.mask, vs=rx.VS)
    try:
        dev.set_raycast_exact(True)
        u, s, r = exact_pass(dev, host_scan(c), c.tf, view=True)
        assert (u >= 2 ** 24).any()  # (the conversion has to round somewhere)
        np.testing.assert_array_equal(r.view(np.uint32), rx.float_view(u, s).view(np.uint32))
        np.testing.assert_array_equal(r != 0, y.full != 0, err_msg="support")
        diff = np.abs(r.astype(np.float64) - y.full)
        print(f"{shape_name}: largest |view - oracle's float pass| = {diff.max():.3e} m")
        assert (diff <= rx.view_bound(y, y.full)).all()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (4) the sweep
@pytest.mark.parametrize("new_rule", (1, 0), ids=("new_rule", "old_rule"))
def test_exact_sweep_is_the_voxelwise_formula(hip, new_rule):
    """statements.raycast_update_sweep_is_the_voxelwise_formula with the switch on: exact begin, two scans, finish; the formulas are
    evaluated on the r (the float view), map and flags read from the same handle before finish - elementwise, at the statement's own
    2e-6 relative and 1e-6 absolute"""
    sensor, vs = "os1-16", 0.5
    det, sp, dp, h, w = statements.sensor_detector(hip, sensor, vs, raycast__new_update_rule=new_rule)
    try:
        assert det.set_raycast_exact(True) == capi.OK
        synth.seed_ground(det)
        scene = synth.make_scene(21, n_targets=2)
        s0, s1, s2 = synth.scan_sequence(scene, sensor, 3, seed0=300)
        det.process_scan(s0.scan, s0.tf)
        its0 = det.status().detection_its
        det.lib.profile_enable(det.h, 1)
        assert det.raycast_begin(s0.scan, s0.tf) == capi.OK
        det.process_scan(s1.scan, s1.tf)
        det.process_scan(s2.scan, s2.tf)
        its_diff = np.float32(det.status().detection_its - its0)
        assert its_diff == 2
        m, fl, r = (det.read_map(k).astype(np.float32).reshape(-1) for k in (capi.MAP_VOXELS, capi.MAP_FLAGS, capi.MAP_RAYCAST))
        u, s = det.raycast_units()
        np.testing.assert_array_equal(r.view(np.uint32), rx.float_view(u.reshape(-1), s).view(np.uint32))
        assert det.raycast_finish() == capi.OK
        ran = profiled_calls(det.lib, det)
        det.lib.profile_enable(det.h, 0)
        assert ran.get("k_raycast_exact", 0) == 1 and ran.get("k_ray_sweep_exact", 0) == 1 and "k_raycast" not in ran and "k_ray_sweep" not in ran, ran
        got = det.read_map(capi.MAP_VOXELS).reshape(-1)
        upd = (fl == 0) & (r > 0)
        assert upd.sum() > 10_000 and (fl != 0).sum() > 100 and ((fl != 0) & (r > 0)).sum() >= 1
        score, coef = np.float32(dp.voxel_map__scores__ray), np.float32(dp.raycast__weight_coefficient)
        if new_rule:
            wf = np.float32(coef / np.float32(np.float32(np.sqrt(3.0)) * np.float32(vs)))
            n_int = wf * r[upd]
            w1 = np.exp2(-(its_diff.astype(np.float64) * n_int.astype(np.float64))).astype(np.float32)
        else:
            mx = r.max()
            ws = coef * np.sqrt(r[upd] / mx, dtype=np.float32)
            w1 = np.clip(np.power((np.float32(1.0) - ws).astype(np.float64), np.float64(its_diff)).astype(np.float32), np.float32(0), np.float32(1))
        want = m.copy()
        with np.errstate(invalid="ignore"):
            want[upd] = w1 * m[upd] + (np.float32(1.0) - w1) * score
        fin = np.isfinite(want)
        np.testing.assert_array_equal(np.isfinite(got), fin)
        np.testing.assert_array_equal(got[~upd].view(np.uint32), m[~upd].view(np.uint32))  # untouched elsewhere, bit for bit
        np.testing.assert_allclose(got[fin], want[fin], rtol=2e-6, atol=1e-6)
        assert (got[upd] != m[upd]).sum() > 10_000
        assert not det.read_map(capi.MAP_FLAGS).any()
        assert not det.read_map(capi.MAP_RAYCAST).view(np.uint32).any()  # cleared to zero bits
        assert det.raycast_units(allow=(capi.ERR_NOT_PENDING,)) == (None, capi.ERR_NOT_PENDING)
    finally:
        det.close()


# ------------------------------------------------------------------------------------------------ (5) with motion
@pytest.mark.parametrize("shift_kind", rm.SHIFTS)
@pytest.mark.parametrize("shape_name", rx.SHAPE_NAMES)
def test_units_of_motion_compensated_rays(oracle, hip, shape_name, shift_kind):
    """vofod_set_raycast_motion on, quarter-turn tables (T d is a signed permutation, tf o T_k exact): U equals the single-ray yardstick
    with each ray cast under compose_quarter(tf, k of its measurement column), bit for bit; host table, device tables at 16-byte
    alignment and 4 bytes behind it"""
    c = rx.case(shape_name)
    lut = LUTS["offsets_28mm_36mm"](hip, c.shape)
    shift = rm.shifts(shift_kind, c.h, c.w, seed=4)
    k_of_m, table = rc.quarter_table(c.w, seed=c.h)
    i = np.arange(c.h * c.w, dtype=np.int64)
    m = rm.measurement_column(i // c.w, i % c.w, c.w, shift)
    tfs = [rc.compose_quarter(c.tf, k) for k in range(4)]
    ref = rc.detector(oracle, c.shape, lut, mask=c.mask, vs=rx.VS)
    dev = rc.detector(hip, c.shape, lut, mask=c.mask, vs=rx.VS)
    mem = DeviceMem()
    try:
        y = rx.single_ray_yardstick(ref, c, tf_of_pixel=lambda px: tfs[int(k_of_m[m[px]])])
        assert np.count_nonzero(y.units) > 100
        dev.set_column_shift(shift)
        assert dev.set_raycast_motion(True) == capi.OK and dev.set_raycast_exact(True) == capi.OK
        dev.lib.profile_enable(dev.h, 1)
        forms = {"host": host_scan(c, table=table), "device16": device_scan(mem, c, table), "device+4": device_scan(mem, c, table, shift=4)}
        for name, sd in forms.items():
            u, s = exact_pass(dev, sd, c.tf)
            assert s == y.s
            np.testing.assert_array_equal(u, y.units, err_msg=f"{shape_name}/{shift_kind}/{name}")
        ran = profiled_calls(dev.lib, dev)
        dev.lib.profile_enable(dev.h, 0)
        assert ran.get("k_raycast_exact", 0) == len(forms) and "k_raycast" not in ran and "k_raycast_motion" not in ran, ran
        # the table moves the rays: the rigid pass of the same scan is another map
        dev.set_raycast_motion(False)
        rigid, _ = exact_pass(dev, host_scan(c, table=table), c.tf)
        assert (rigid != y.units).any()
    finally:
        mem.free()
        for d in (ref, dev):
            d.close()


# ------------------------------------------------------------------------------------------------ (6) the clamp, by hand
def test_clamp_by_hand(hip):
    """One ray along +x from a voxel centre, motion table 0.25 * I, 0.5 m voxels, range 0 (length = max_distance = 20): |dir| = 0.25, so
    the walk's parameter runs four times as fast as metres: tmax = 0.25 / 0.25 = 1.0, tdelta = 0.5 / 0.25 = 2.0, the other axes never
    step.  Pieces: 1.0, then 2.0 per voxel up to 19.0, then 20 - 19 = 1.0.  On a sensor of 100 pixels S = 24 and QMAX = 2^24 units =
    1.0: the first piece is exactly QMAX, every 2.0-long piece counts QMAX."""
    shape = rm.SHAPES["5x20"]
    h, w = shape[:2]
    n = h * w
    dirs = np.tile(np.array([1.0, 0.0, 0.0], dtype=f32), (n, 1))
    dev = rc.detector(hip, shape, (dirs, None), vs=0.5)
    try:
        s_want, qmax = rx.scale_rule(n, 0.5)
        assert (s_want, qmax) == (24, 2 ** 24)
        off = np.array(dev.map_offset, dtype=np.float64)
        sx, sy, sz = (int(v) for v in dev.map_size)
        cell = np.array([sx // 2, sy // 2, sz // 2])
        centre = ((cell + 0.5) * 0.5 + off).astype(f32)
        assert np.array_equal(centre.astype(np.float64), (cell + 0.5) * 0.5 + off)  # exactly a voxel centre in float32
        tf = np.concatenate([np.eye(3, dtype=f32), centre[:, None]], axis=1)
        inten = np.full(n, f32(rc.MIN_INTENSITY) - f32(1.0), dtype=f32)
        inten[7] = 600.0
        table = np.tile((0.25 * np.eye(3, 4)).astype(f32), (w, 1, 1))
        sd = ScanData.range_image(np.zeros(n, dtype=np.uint32), w, h, intensity=inten, col_tfs=table)
        assert dev.set_raycast_motion(True) == capi.OK
        # the float pass first: the pieces themselves
        assert dev.raycast_begin(sd, tf) == capi.OK
        pieces = dev.read_map(capi.MAP_RAYCAST).reshape(-1)
        assert dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
        lin = (cell[2] * sy + cell[1]) * sx + cell[0]
        want_pieces = np.zeros(sx * sy * sz, dtype=f32)
        want_pieces[lin:lin + 11] = [1.0] + [2.0] * 9 + [1.0]
        assert cell[0] + 11 <= sx
        np.testing.assert_array_equal(pieces, want_pieces)
        assert dev.set_raycast_exact(True) == capi.OK
        u, s, r = exact_pass(dev, sd, tf, view=True)
        assert s == 24
        want = np.zeros(sx * sy * sz, dtype=np.int64)
        want[lin:lin + 11] = qmax
        np.testing.assert_array_equal(u, want)
        np.testing.assert_array_equal(r, np.where(want != 0, f32(1.0), f32(0.0)))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (7) the switch's rules
def test_switch_rules_and_refusals(hip):
    """on the OS1-16 detector and scans of the sweep statement (a pass there finishes: scans between begin and finish are detected)"""
    import ctypes as C

    dev, sp, dp, h, w = statements.sensor_detector(hip, "os1-16", 0.5, max_batch=2)
    try:
        synth.seed_ground(dev)
        s0 = synth.scan_sequence(synth.make_scene(21, n_targets=2), "os1-16", 1, seed0=300)[0]
        sd, c = s0.scan, s0
        n_vox = dev.n_voxels
        # off after vofod_create: the launches are k_raycast and k_ray_sweep, vofod_raycast_units has nothing to return
        dev.lib.profile_enable(dev.h, 1)
        assert dev.raycast_begin(sd, c.tf) == capi.OK
        assert dev.raycast_units(allow=(capi.ERR_NOT_PENDING,)) == (None, capi.ERR_NOT_PENDING)
        float_pass = dev.read_map(capi.MAP_RAYCAST).reshape(-1).copy()
        dev.write_map(capi.MAP_RAYCAST, float_pass)  # (a float pass takes both calls, as ever)
        dev.voxels_as_pc(0.5, True, which=capi.MAP_RAYCAST)
        dev.process_scan(sd, c.tf)
        assert dev.raycast_finish() == capi.OK
        ran = profiled_calls(dev.lib, dev)
        assert ran.get("k_raycast", 0) == 1 and ran.get("k_ray_sweep", 0) == 1 and "k_raycast_exact" not in ran and "k_ray_sweep_exact" not in ran, ran
        assert dev.raycast_units(allow=(capi.ERR_NOT_PENDING,)) == (None, capi.ERR_NOT_PENDING)
        # on (`on` is taken as on != 0); kept across vofod_reset
        assert dev.lib.set_raycast_exact(dev.h, 7) == capi.OK
        dev.reset()
        assert dev.raycast_begin(sd, c.tf) == capi.OK
        u, s = dev.raycast_units()
        assert s == rx.S_TABLE[(16, 1024, 0.5)] and u.any()
        # VOFOD_ERR_BUSY while the pass is pending, for the switch and for the two calls that would take units for floats
        for on in (False, True):
            assert dev.set_raycast_exact(on, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
        assert dev.lib.write_map(dev.h, capi.MAP_RAYCAST, capi.ptr(float_pass), n_vox) == capi.ERR_BUSY
        n_out = C.c_size_t(0)
        assert dev.lib.voxels_as_pc(dev.h, capi.MAP_RAYCAST, 0.5, 1, None, 0, C.byref(n_out)) == capi.ERR_BUSY
        dev.voxels_as_pc(0.5, True, which=capi.MAP_VOXELS)  # (the other maps are not concerned)
        dev.write_map(capi.MAP_FLAGS, dev.read_map(capi.MAP_FLAGS))
        u2, _ = dev.raycast_units()
        np.testing.assert_array_equal(u2, u)  # the pass behind the refused calls
        wrong = np.zeros(n_vox + 1, dtype=np.uint32)
        s_out = C.c_int32(0)
        assert dev.lib.raycast_units(dev.h, capi.ptr(wrong), wrong.size, C.byref(s_out)) == capi.ERR_SIZE_MISMATCH
        dev.process_scan(sd, c.tf)
        assert dev.raycast_finish() == capi.OK
        ran = profiled_calls(dev.lib, dev)
        dev.lib.profile_enable(dev.h, 0)
        assert ran.get("k_raycast_exact", 0) == 1 and ran.get("k_ray_sweep_exact", 0) == 1 and "k_raycast" not in ran and "k_ray_sweep" not in ran, ran
        # an abandoned exact pass takes its units with it: nothing but floats is ever read outside a pending exact pass
        assert dev.raycast_begin(sd, c.tf) == capi.OK
        assert dev.raycast_units()[0].any()
        assert dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
        assert not dev.read_map(capi.MAP_RAYCAST).view(np.uint32).any()
        assert not dev.export_map(1 << capi.MAP_RAYCAST)[88:128].any()  # no records, no byte
        # after the pass the two calls work again
        dev.write_map(capi.MAP_RAYCAST, np.zeros(n_vox, dtype=f32))
        # ... and VOFOD_ERR_BUSY while a submitted batch is in flight
        ticket = dev.batch_submit([sd, sd], np.stack([c.tf, c.tf]))
        assert dev.set_raycast_exact(False, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
        dev.batch_collect(ticket)
        assert dev.set_raycast_exact(False) == capi.OK
        assert dev.lib.set_raycast_exact(None, 1) == capi.ERR_INVALID_ARG
        # off again: the float pass of before (within the order of its float atomics)
        assert dev.raycast_begin(sd, c.tf) == capi.OK
        np.testing.assert_allclose(dev.read_map(capi.MAP_RAYCAST).reshape(-1), float_pass, rtol=2e-5, atol=2e-6)
        assert dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (8) stream, replicas, snapshots
def test_stream_replicas_and_snapshots(hip):
    """Four OS1-16 scans under VOFOD_SCAN_AUTO_RAYCAST: two exact handles end with all three maps bit-identical (and hold the same
    units while a pass is pending), an exact handle and a float handle agree within the stream tolerance of the suite.  Then the
    snapshot: flags + raycast taken during a pending exact pass carry S + 1 in byte 0 of the reserved block; applied to another handle
    they give equal units, and after finish on both bit-identical voxel maps."""
    a, b = make_pair(hip, hip, "os1-16", 0.25, max_batch=1)
    f, r = make_pair(hip, hip, "os1-16", 0.25, max_batch=1)
    try:
        warm_scene, scene, frames, _, _ = rm.moving_frames(n=6)
        rm.warm([a, b, f, r], warm_scene)
        h_, w_ = rm.SHAPES["os1_16"][:2]
        s_want = rx.scale_rule(h_ * w_, 0.25)[0]
        for d in (a, b):
            assert d.set_raycast_exact(True) == capi.OK
        a.lib.profile_enable(a.h, 1)
        scans = [ScanData.range_image(s.range, w_, h_, intensity=s.intensity) for s in frames]
        n_pending = 0
        for k in range(4):
            for d in (a, b, f):
                d.process_scan(scans[k], frames[k].tf, flags=capi.SCAN_AUTO_RAYCAST)
            sa, sb, sf = a.status(), b.status(), f.status()
            assert (sa.raycast_pending, sa.detection_its) == (sb.raycast_pending, sb.detection_its) == (sf.raycast_pending, sf.detection_its)
            if sa.raycast_pending:
                n_pending += 1
                ua, s = a.raycast_units()
                ub, _ = b.raycast_units()
                assert s == s_want and np.count_nonzero(ua) > 10_000
                np.testing.assert_array_equal(ua, ub)
            for which in (capi.MAP_VOXELS, capi.MAP_FLAGS, capi.MAP_RAYCAST):
                np.testing.assert_array_equal(a.read_map(which).view(np.uint32), b.read_map(which).view(np.uint32), err_msg=f"scan {k}, map {which}")
            ma, mf = a.read_map(capi.MAP_VOXELS), f.read_map(capi.MAP_VOXELS)
            fin = np.isfinite(ma)
            np.testing.assert_array_equal(np.isfinite(mf), fin)
            np.testing.assert_allclose(ma[fin], mf[fin], rtol=1e-4, atol=1e-3)
            np.testing.assert_array_equal(a.read_map(capi.MAP_FLAGS), f.read_map(capi.MAP_FLAGS))
        ran = profiled_calls(a.lib, a)
        a.lib.profile_enable(a.h, 0)
        assert n_pending == 2 and not a.status().raycast_pending
        assert ran.get("k_raycast_exact", 0) == 2 and ran.get("k_ray_sweep_exact", 0) == 2 and "k_raycast" not in ran and "k_ray_sweep" not in ran, ran
        # snapshots without a pending exact pass: 16 zero bytes - nothing pending, and a pending float pass
        assert not a.export_map(capi.MAPS_ALL)[112:128].any()
        assert f.raycast_begin(scans[4], frames[4].tf) == capi.OK
        assert not f.export_map(RAY_MAPS)[112:128].any()
        assert f.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION
        # a pending exact pass: begin, one scan, then the voxel map and flags + raycast travel to r (whose own switch is off)
        assert a.raycast_begin(scans[4], frames[4].tf) == capi.OK
        a.process_scan(scans[5], frames[5].tf)
        r.apply_map(a.export_map(1 << capi.MAP_VOXELS))
        snap = a.export_map(RAY_MAPS)
        assert snap[112] == s_want + 1 and not snap[113:128].any()
        from vofod_amd import mapsync
        dec = mapsync.decode(snap)  # the numpy statement of the wire format carries the byte: bytes -> snapshot -> the same bytes
        assert dec.raycast_log2_units == s_want and dec.raycast_pending and np.array_equal(mapsync.encode(dec), snap)
        assert not a.export_map(1 << capi.MAP_FLAGS)[112:128].any()  # (the raycast map is not in the mask)
        r.apply_map(snap)
        assert r.status().raycast_pending
        ua, _ = a.raycast_units()
        ur, s = r.raycast_units()
        assert s == s_want and ua.any()
        np.testing.assert_array_equal(ur, ua)
        np.testing.assert_array_equal(r.read_map(capi.MAP_RAYCAST).view(np.uint32), a.read_map(capi.MAP_RAYCAST).view(np.uint32))
        # a header whose S is not this handle's is refused, and so is a non-zero byte among the other 15
        bad = snap.copy()
        bad[112] = s_want + 2
        assert r.lib.map_apply(r.h, capi.ptr(bad), bad.size, capi.MEM_HOST) == capi.ERR_SIZE_MISMATCH
        bad = snap.copy()
        bad[113] = 1
        assert r.lib.map_apply(r.h, capi.ptr(bad), bad.size, capi.MEM_HOST) == capi.ERR_INVALID_ARG
        assert a.raycast_finish() == capi.OK and r.raycast_finish() == capi.OK
        ma, mr = a.read_map(capi.MAP_VOXELS), r.read_map(capi.MAP_VOXELS)
        np.testing.assert_array_equal(ma.view(np.uint32), mr.view(np.uint32))
        assert not r.read_map(capi.MAP_RAYCAST).view(np.uint32).any() and not r.read_map(capi.MAP_FLAGS).any()
    finally:
        for d in (a, b, f, r):
            d.close()
