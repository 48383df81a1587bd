"""vofod_detection_pixels (k_det_pixel_sizes + k_det_pixels, detection_pixels.h): the raw returns of every detection, asked for after
production calls.  Expected values come from the numpy statement of detection_pixels_cases.py on the oracle's debug view
(test_detection_pixels_cpu.py holds that construction on the oracle alone): span, pixels and member are compared exactly, xyz bit
for bit.

Three set-ups, one of each per file:
  bench    the recipe of test_gpu_tail_edges.py (OS1-16, 0.25 m voxels, hand-placed cell scenes, four frames): the routes, the
           large detections, the contract;
  stream   the warmed OS1-16 pair of test_gpu_range_image.py (synthetic scenes, an offset LUT): range images, pose tables;
  odd      a 15 x 1021 sensor (w * h = 3 mod 4) on the default area: device-resident columns read in place, the guard, and what
           ends the validity (reset, map_apply, map_shift).
Routes are asserted from the profiler's kernel list under the default switches only, as the neighbouring files do.  The two
fallback switches are read on every call (chain_plan.h: read_switches), so they are set with monkeypatch in this process, as
test_gpu_detection_points.py and test_gpu_tail_edges.py set them - a child process would build the 19.5 M voxel maps once more.

Mutations, each run once on an MI355X (profiles/r26_detection_pixels.txt): cell_key given the map's origin in the walk turns all 26
tests of this file red (VOFOD_ERR_DEVICE from the count check); an open area box in fetch_point turns none red, and cannot: a return
on the area's face lies in the map's outermost voxel layer, whose clusters exploreToGround never calls floating."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import detection_pixels_cases as pxc
from test_gpu_tail_edges import Bench, _profiled, _route_checked
from vofod_amd import capi
from vofod_amd.detector import ScanData

pytestmark = pytest.mark.gpu
if __import__("os").environ.get("VOFOD_TEST_HARNESS_SELFCHECK"):
    pytest.skip("oracle against oracle: the oracle has no vofod_detection_pixels", allow_module_level=True)
f32 = np.float32
ROOT = Path(__file__).resolve().parent.parent
NP = capi.ERR_NOT_PENDING


# ------------------------------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope="module")
def bench(oracle, hip):
    b = Bench(oracle, hip)
    b.oracle = oracle
    b.cache = {}
    yield b
    b.close()


def _expected(bench, name):
    """the oracle's batch over the loaded scene, once per scene: (detections, per-frame counts, expectation per frame)"""
    if name not in bench.cache:
        da, pa, exp, _ = pxc.expected_batch(bench.oracle, bench.ref, bench.scans, bench.tfs)
        bench.cache[name] = (da, pa, exp)
    return bench.cache[name]


def _same_detections(want, got):
    assert len(want) == len(got) >= 1
    np.testing.assert_array_equal(got["frame"], want["frame"])
    np.testing.assert_array_equal(got["n_points"], want["n_points"])


def _ask(dev, source=capi.POINTS_SYNC, first=True):
    """the answer, and the launches it took: the sizing kernel once per production call, the walk once per answer"""
    out, ran = _profiled(dev, lambda: dev.detection_pixels(source))
    if _route_checked():
        want = {"k_det_pixels": 1, **({"k_det_pixel_sizes": 1} if first else {})}
        assert ran == want, ran
    return out


# ------------------------------------------------------------------------------------------------------------ 1. the routes
@pytest.mark.parametrize("route", ["scan", "scan_no_update", "batch", "tickets"])
@pytest.mark.parametrize("name", pxc.ROUTE_SCENES)
def test_routes(bench, name, route):
    """scan: single map-updating scans (kernels_far.h: k_far_final + k_tail_far); scan_no_update: the same with
    VOFOD_SCAN_NO_MAP_UPDATE; batch: a read-only batch of four frames on k_frame_lds_far through process_batch; tickets: the
    batch and its reverse as two tickets in flight, collected in order, asked in the reverse order"""
    checked = _route_checked()
    pxc.load(bench, name)
    dev = bench.dev
    da, pa, exp = _expected(bench, name)
    if route in ("scan", "scan_no_update"):
        k = 0
        for f in (0, 1):
            flags = capi.SCAN_DEFAULT if route == "scan" else capi.SCAN_NO_MAP_UPDATE
            d, ran = _profiled(dev, lambda: dev.process_scan(bench.scans[f], bench.tf, flags=flags))
            want = da[k : k + int(pa[f])].copy()
            want["frame"] = 0
            k += int(pa[f])
            _same_detections(want, d)
            if checked and route == "scan":
                assert ran.get("k_far_final", 0) == 1 and "k_det_pixels" not in ran, ran
            span, px, member, xyz = _ask(dev)
            pxc.assert_pixels(span, px, member, xyz, d, [exp[f]])
            if route == "scan":
                bench.reset_maps()
        return
    if route == "batch":
        (db, pb), ran = _profiled(dev, lambda: dev.process_batch(bench.scans, bench.tfs))
        np.testing.assert_array_equal(pb, pa)
        _same_detections(da, db)
        if checked:
            assert "k_frame_lds_far" in ran and "k_det_pixels" not in ran and "k_det_pixel_sizes" not in ran, ran
        span, px, member, xyz = _ask(dev)
        pxc.assert_pixels(span, px, member, xyz, db, exp)
        # asked again: the same bytes, no second sizing launch
        again = _ask(dev, first=False)
        for a, b in zip((span, px, member, xyz), again):
            assert a.tobytes() == b.tobytes()
        print(f"\n[detection pixels] {name} batch: {len(span)} detections, {len(px)} pixels, largest {int(span['count'].max())}")
        return
    orders = [[0, 1, 2, 3], [3, 2, 1, 0]]
    dev.lib.profile_enable(dev.h, 1)
    try:
        tickets = [dev.batch_submit([bench.scans[i] for i in o], bench.tfs[o]) for o in orders]
        for t in tickets:
            assert dev.detection_pixels(t, allow=(NP,)) == NP
        dets = [dev.batch_collect(t)[0] for t in tickets]
        from test_gpu_stream_route import profiled_calls

        ran = profiled_calls(dev.lib, dev)
    finally:
        dev.lib.profile_enable(dev.h, 0)
    if checked:
        assert ran.get("k_frame_lds_far", 0) >= 1 and "k_det_pixels" not in ran, ran
    assert dev.detection_pixels(capi.POINTS_SYNC, allow=(NP,)) == NP  # (a ticket's, not a synchronous call's)
    for t, o, d in reversed(list(zip(tickets, orders, dets))):
        span, px, member, xyz = _ask(dev, t)
        pxc.assert_pixels(span, px, member, xyz, d, [exp[i] for i in o])


# --------------------------------------------------------------------------------------------------------- 2. the fallbacks
@pytest.mark.parametrize("fallback", ["VOFOD_DEVICE_TAIL=0", "VOFOD_CLOSE_FIRST=0"])
def test_batch_under_a_production_fallback(bench, monkeypatch, fallback):
    """the batch under the host tail (k_pack, lists read back) and under the full clustering (k_frame_lds_full, member lists in
    arrival order): the switches are read on every call"""
    k, v = fallback.split("=")
    monkeypatch.setenv(k, v)
    pxc.load(bench, "weights")
    dev = bench.dev
    da, pa, exp = _expected(bench, "weights")
    (db, pb), ran = _profiled(dev, lambda: dev.process_batch(bench.scans, bench.tfs))
    _same_detections(da, db)
    assert ({"VOFOD_DEVICE_TAIL": "k_pack", "VOFOD_CLOSE_FIRST": "k_frame_lds_full"}[k]) in ran, ran
    span, px, member, xyz = dev.detection_pixels()
    pxc.assert_pixels(span, px, member, xyz, db, exp)


# --------------------------------------------------------------------------------------------------- 3. the large detections
@pytest.mark.parametrize("name", pxc.LARGE_SCENES)
def test_large_detections(bench, name):
    """one detection of 343 voxels (one LDS list), of 576 and of 729 (more than PX_CAP: the sorted list is built pass by pass in
    the staging buffer, one walk), beside a pair"""
    src = (ROOT / "vofod_amd" / "csrc" / "detection_pixels.h").read_text()
    cap = int(re.search(r"constexpr\s+uint32_t\s+PX_CAP\s*=\s*(\d+)\s*;", src).group(1))
    pxc.load(bench, name)
    dev = bench.dev
    da, pa, exp = _expected(bench, name)
    db, pb = dev.process_batch(bench.scans, bench.tfs)
    _same_detections(da, db)
    largest = int(db["n_points"].max())
    assert largest == pxc.dpc.LARGEST[name] and (largest > cap) == (name != "block_7x7x7"), (largest, cap)
    span, px, member, xyz = _ask(dev)
    pxc.assert_pixels(span, px, member, xyz, db, exp)
    # the two calls tie together: the pixel's member is a position in the detection's list of detection_points
    ext, pts, idx = dev.detection_points()
    np.testing.assert_array_equal(ext["id"], span["id"])
    for e, s in zip(ext, span):
        m = member[int(s["first"]) : int(s["first"]) + int(s["count"])]
        assert int(m.max()) == int(e["count"]) - 1
        w = pts["range"][int(e["first"]) : int(e["first"]) + int(e["count"])]
        np.testing.assert_array_equal(np.bincount(m, minlength=int(e["count"])), w)


# -------------------------------------------------------------------------------------------------------- 4. the input forms
def _cloud(sd):
    return SimpleNamespace(x=sd.x, y=sd.y, z=sd.z, intensity=None, range=None, scan=SimpleNamespace(width=sd.width, height=sd.height))


@pytest.mark.parametrize("form", ["host_columns", "host_aos48"])
def test_host_forms(bench, form):
    """host packed columns at no constant pitch (a copy per column) and the nodelet's 48-byte structs (one copy of the block, read
    in place at the struct's stride): the same pixels"""
    from test_gpu_frame_inputs import host_scan, lay_aos48

    pxc.load(bench, "boundary")
    dev = bench.dev
    da, pa, exp = _expected(bench, "boundary")
    if form == "host_aos48":
        scans = [host_scan(_cloud(s), lay_aos48(_cloud(s))) for s in bench.scans]
        assert all(s.stride_bytes == 48 for s in scans)
    else:
        scans = [ScanData(x=s.x.copy(), y=s.y.copy(), z=s.z.copy(), width=s.width, height=s.height) for s in bench.scans]
    db, pb = dev.process_batch(scans, bench.tfs)
    _same_detections(da, db)
    span, px, member, xyz = _ask(dev)
    pxc.assert_pixels(span, px, member, xyz, db, exp)


@pytest.fixture(scope="module")
def stream(oracle, hip):
    from test_gpu_range_image import DeviceMem, warmed_pair

    import range_motion_cases as rm

    p = warmed_pair(oracle, hip, "os1-16", n_frames=4, max_batch=4)
    p.oracle = oracle
    w_ = p.shape[1]
    p.tables = np.stack([rm.rigid_poses(w_, seed=f, yaw_rate=0.5 + 0.05 * f, v=(2.0, 0.1 * f, 0.0)) for f in range(4)])
    assert p.dev.set_point_motion(True) == capi.OK
    p.mem = DeviceMem()
    yield p
    p.mem.free()
    p.ref.close()
    p.dev.close()


@pytest.mark.parametrize("form", ["range_image", "range_image_col_tfs", "point_scan_col_tfs"])
def test_decoded_and_compensated_forms(stream, form):
    """the point is the one the pipeline consumed: the decoded point of a range image, the compensated point of a range image or
    a point scan with a pose per column.  The statement is fed what range_to_points / deskew_points return, and so is the oracle"""
    p, dev = stream, stream.dev
    h_, w_ = p.shape[:2]
    plain = [dev.range_to_points(ScanData.range_image(s.range, w_, h_)) for s in p.frames]
    if form == "range_image":
        scans = [ScanData.range_image(s.range, w_, h_) for s in p.frames]
        cols = plain
        kernel = "k_range_decode"
    elif form == "range_image_col_tfs":
        scans = [ScanData.range_image(s.range, w_, h_, col_tfs=p.tables[f]) for f, s in enumerate(p.frames)]
        cols = [dev.range_to_points(sd) for sd in scans]
        kernel = "k_range_decode_motion"
    else:
        scans = [ScanData(x=c[0], y=c[1], z=c[2], width=w_, height=h_, col_tfs=p.tables[f]) for f, c in enumerate(plain)]
        cols = [dev.deskew_points(sd) for sd in scans]
        kernel = "k_point_deskew"
    if form != "range_image":
        moved = np.abs(cols[0][0] - plain[0][0])
        assert moved[np.isfinite(moved)].max() > 0.05  # (the poses move the points)
    ref_scans = [ScanData(x=c[0], y=c[1], z=c[2], width=w_, height=h_) for c in cols]
    da, pa, exp, _ = pxc.expected_batch(p.oracle, p.ref, ref_scans, p.tfs)
    (db, pb), ran = _profiled(dev, lambda: dev.process_batch(scans, p.tfs))
    np.testing.assert_array_equal(pb, pa)
    _same_detections(da, db)
    if _route_checked():
        assert ran.get(kernel, 0) == 1, ran
    span, px, member, xyz = _ask(dev)
    pxc.assert_pixels(span, px, member, xyz, db, exp)
    assert len(px) > int(db["n_points"].sum())  # (real scans: member voxels of more than one return)
    print(f"\n[detection pixels] {form}: {len(span)} detections, {len(px)} pixels")


ODD = (15, 1021, 33.2, 120.0)  # w * h = 15 315 = 3 mod 4


@pytest.fixture(scope="module")
def odd(oracle, hip):
    from test_gpu_frame_inputs import DEFAULT_AREA, make_area_pair, scene_frames, warm_both
    from test_gpu_range_image import DeviceMem

    ref, dev = make_area_pair(oracle, hip, shape=ODD, max_batch=4)
    before_any_call = dev.detection_pixels(allow=(NP,)), dev.detection_pixels(0, allow=(NP,))
    warm_scene, _, frames = scene_frames(DEFAULT_AREA, (0.0, 0.0), 4, shape=ODD, scene_seed=5, seed0=70)
    warm_both(ref, dev, warm_scene, (0.0, 0.0), shape=ODD)
    p = SimpleNamespace(ref=ref, dev=dev, frames=frames, tfs=np.stack([s.tf for s in frames]), oracle=oracle, before_any_call=before_any_call, mem=DeviceMem())
    p.scans = [s.scan for s in frames]
    p.da, p.pa, p.exp, _ = pxc.expected_batch(oracle, ref, p.scans, p.tfs)
    assert len(p.da) >= 1
    yield p
    p.mem.free()
    ref.close()
    dev.close()


def _device_scans(p):
    from test_gpu_frame_inputs import lay_columns

    scans = [p.mem.scan(s, lay_columns(s, 4)) for s in p.frames]
    assert all(sd.x % 16 == 4 and sd.y % 16 == 4 and sd.z % 16 == 4 for sd in scans) and (ODD[0] * ODD[1]) % 4 == 3
    return scans


def test_device_columns_read_in_place_and_the_guard(odd):
    """device-resident columns whose bases lie 4 bytes behind a 16-byte boundary, 15 315 pixels (no multiple of 4): read in place
    by the batch and once more by the query.  Then the guard: one listed pixel's point is zeroed in the caller's buffer (the
    exclude box drops it) - the returns found no longer number the weights: VOFOD_ERR_DEVICE, the detection named, nothing
    written, the handle usable.  An error return, not a fault; run once."""
    p, dev = odd, odd.dev
    scans = _device_scans(p)
    db, pb = dev.process_batch(scans, p.tfs)
    _same_detections(p.da, db)
    span, px, member, xyz = _ask(dev)
    pxc.assert_pixels(span, px, member, xyz, db, p.exp)
    # the guard
    victim = int(px[0])
    f = int(span["frame"][0])
    zero = np.zeros(1, dtype=f32)
    for base in (scans[f].x, scans[f].y, scans[f].z):
        assert p.mem.rt.hipMemcpy(C.c_void_p(base + 4 * victim), capi.ptr(zero), 4, 1) == 0
    n_span, n_px = C.c_size_t(0), C.c_size_t(0)
    s2 = np.full(len(span) * 16, 0xAB, dtype=np.uint8).view(capi.DETECTION_SPAN)
    p2, m2, x2 = np.full(len(px), 0xCDCDCDCD, dtype=np.uint32), np.full(len(px), 0xCDCDCDCD, dtype=np.uint32), np.full(3 * len(px), 0xCDCDCDCD, dtype=np.uint32)
    st = dev.lib.detection_pixels(dev.h, -1, capi.ptr(s2), len(s2), C.byref(n_span), capi.ptr(p2), capi.ptr(m2), capi.ptr(x2), len(p2), C.byref(n_px), capi.MEM_HOST)
    assert st == capi.ERR_DEVICE, st
    msg = dev.lib.last_error_string(dev.h).decode()
    assert f"detection {int(span['id'][0])} " in msg and str(int(span["count"][0]) - 1) in msg, msg
    assert (s2.view(np.uint8) == 0xAB).all() and (p2 == 0xCDCDCDCD).all() and (m2 == 0xCDCDCDCD).all() and (x2 == 0xCDCDCDCD).all()
    # the handle is still usable: the same batch from host columns
    db, pb = dev.process_batch(p.scans, p.tfs)
    span, px, member, xyz = dev.detection_pixels()
    pxc.assert_pixels(span, px, member, xyz, db, p.exp)


# ------------------------------------------------------------------------------------------------------------ 5. the contract
def _raw(dev, source, span, span_cap, px, member, xyz, px_cap, memspace=capi.MEM_HOST):
    n_span, n_px = C.c_size_t(12345), C.c_size_t(12345)
    st = dev.lib.detection_pixels(dev.h, source, capi.ptr(span), span_cap, C.byref(n_span), capi.ptr(px), capi.ptr(member), capi.ptr(xyz), px_cap, C.byref(n_px), memspace)
    return st, n_span.value, n_px.value


def test_contract(bench):
    """size query (the sizing kernel at most, never the walk), buffers one element short (both counts, nothing written, no walk),
    outputs left out, bad arguments, zero detections (no launch), a collect that returned VOFOD_ERR_CAPACITY, a workspace taken
    again"""
    dev = bench.dev
    checked = _route_checked()
    pxc.load(bench, "weights")
    da, pa, exp = _expected(bench, "weights")
    db, pb = dev.process_batch(bench.scans, bench.tfs)
    n, total = len(db), sum(len(p) for e in exp for p, _, _ in e)
    (st, ns, npx), ran = _profiled(dev, lambda: _raw(dev, capi.POINTS_SYNC, None, 0, None, None, None, 0))
    assert (st, ns, npx) == (capi.OK, n, total) and (not checked or ran == {"k_det_pixel_sizes": 1}), (st, ns, npx, ran)
    (st, ns, npx), ran = _profiled(dev, lambda: _raw(dev, capi.POINTS_SYNC, None, 0, None, None, None, 0))
    assert (st, ns, npx) == (capi.OK, n, total) and (not checked or ran == {}), (st, ns, npx, ran)
    for span_cap, px_cap in ((n - 1, total), (n, total - 1)):
        span = np.full(n * 16, 0xAB, dtype=np.uint8).view(capi.DETECTION_SPAN)
        px, member, xyz = (np.full(k * total, 0xCDCDCDCD, dtype=np.uint32) for k in (1, 1, 3))
        (st, ns, npx), ran = _profiled(dev, lambda: _raw(dev, capi.POINTS_SYNC, span, span_cap, px, member, xyz, px_cap))
        assert (st, ns, npx) == (capi.ERR_CAPACITY, n, total) and (not checked or ran == {}), (st, ns, npx, ran)
        assert (span.view(np.uint8) == 0xAB).all() and all((a == 0xCDCDCDCD).all() for a in (px, member, xyz))
    span, px, member, xyz = dev.detection_pixels()
    pxc.assert_pixels(span, px, member, xyz, db, exp)
    # span alone (no walk), pixels alone
    s2 = np.zeros(n, dtype=capi.DETECTION_SPAN)
    (st, ns, npx), ran = _profiled(dev, lambda: _raw(dev, capi.POINTS_SYNC, s2, n, None, None, None, 0))
    assert (st, ns, npx) == (capi.OK, n, total) and s2.tobytes() == span.tobytes() and (not checked or ran == {}), ran
    p2 = np.zeros(total, dtype=np.uint32)
    assert _raw(dev, capi.POINTS_SYNC, None, 0, p2, None, None, total) == (capi.OK, n, total) and p2.tobytes() == px.tobytes()
    # bad arguments
    m1, x1 = np.zeros(total, dtype=np.uint32), np.zeros(3 * total, dtype=f32)
    for source in (8, -2):
        assert _raw(dev, source, s2, n, p2, m1, x1, total)[0] == capi.ERR_INVALID_ARG
    assert _raw(dev, capi.POINTS_SYNC, s2, n, p2, m1, x1, total, memspace=2)[0] == capi.ERR_INVALID_ARG
    assert _raw(dev, capi.POINTS_SYNC, s2, n, None, m1, None, total)[0] == capi.ERR_INVALID_ARG  # member without pixels
    assert _raw(dev, capi.POINTS_SYNC, s2, n, None, None, x1, total)[0] == capi.ERR_INVALID_ARG  # xyz without pixels
    ok = C.c_size_t(0)
    assert dev.lib.detection_pixels(dev.h, -1, None, 0, None, None, None, None, 0, C.byref(ok), capi.MEM_HOST) == capi.ERR_INVALID_ARG
    assert dev.lib.detection_pixels(dev.h, -1, None, 0, C.byref(ok), None, None, None, 0, None, capi.MEM_HOST) == capi.ERR_INVALID_ARG
    assert _raw(dev, 3, s2, n, p2, m1, x1, total)[0] == NP  # a ticket never submitted
    # a batch without detections: OK, 0 / 0, no launch
    w, h = bench.scans[0].width, bench.scans[0].height
    empty = ScanData(x=np.zeros(w * h, f32), y=np.zeros(w * h, f32), z=np.zeros(w * h, f32), width=w, height=h)
    d0, _ = dev.process_batch([empty] * 4, bench.tfs)
    assert len(d0) == 0
    for args in ((s2, n, p2, m1, x1, total), (None, 0, None, None, None, 0)):
        (st, ns, npx), ran = _profiled(dev, lambda: _raw(dev, capi.POINTS_SYNC, *args))
        assert (st, ns, npx) == (capi.OK, 0, 0) and (not checked or ran == {}), (st, ns, npx, ran)
    # a collect with too small an array returns VOFOD_ERR_CAPACITY and leaves nothing valid
    import os

    arr = (capi.Scan * 4)(*[sc.as_c() for sc in bench.scans])
    tfa = np.ascontiguousarray(bench.tfs, dtype=f32).reshape(4, 12)
    ticket = C.c_int(-1)
    assert dev.lib.batch_submit(dev.h, arr, capi.ptr(tfa), 4, C.byref(ticket)) == capi.OK
    tk = ticket.value
    assert tk == 0 and _raw(dev, capi.POINTS_SYNC, None, 0, None, None, None, 0)[0] == NP and _raw(dev, 0, None, 0, None, None, None, 0)[0] == NP  # the workspace is taken again
    dets, per, n_out = np.zeros(n, dtype=capi.DETECTION), np.zeros(4, dtype=np.uint32), C.c_size_t(0)
    assert dev.lib.batch_collect(dev.h, tk, capi.ptr(dets), 1, capi.ptr(per), C.byref(n_out)) == capi.ERR_CAPACITY and n_out.value == n
    assert _raw(dev, tk, s2, n, p2, m1, x1, total)[0] == NP
    st = dev.lib.batch_collect(dev.h, tk, capi.ptr(dets), n, capi.ptr(per), C.byref(n_out))
    if os.environ.get("VOFOD_DEVICE_TAIL") == "0":
        assert st == NP and _raw(dev, tk, s2, n, p2, m1, x1, total)[0] == NP
    else:
        assert st == capi.OK and n_out.value == n
        span, px, member, xyz = dev.detection_pixels(tk)
        pxc.assert_pixels(span, px, member, xyz, dets, exp)


def test_device_output(bench):
    """pixels, member and xyz into device buffers at addresses that are 4-byte but not 16-byte aligned: the host answer byte for
    byte, nothing written around them; a 2-byte aligned address is refused"""
    from test_gpu_range_image import DeviceMem

    dev = bench.dev
    pxc.load(bench, "block_8x8x9")
    da, pa, exp = _expected(bench, "block_8x8x9")
    db, _ = dev.process_batch(bench.scans, bench.tfs)
    span, px, member, xyz = dev.detection_pixels()
    pxc.assert_pixels(span, px, member, xyz, db, exp)
    total = len(px)
    mem = DeviceMem()
    try:
        fill = lambda k: np.full(k * total + 8, 0x7FC00000, dtype=np.uint32)
        addr = [mem.put(fill(k)) for k in (1, 1, 3)]
        assert all(a % 16 == 0 for a in addr)
        sd, none_p, none_m, none_x = dev.detection_pixels(device_out=(addr[0] + 4, addr[1] + 4, addr[2] + 4, total))
        assert none_p is None and none_m is None and none_x is None and sd.tobytes() == span.tobytes()
        assert dev.detection_pixels(device_out=(addr[0] + 2, None, None, total), allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG
        assert dev.detection_pixels(device_out=(addr[0] + 4, None, addr[2] + 6, total), allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG
        got = [mem.get(a, k * total + 8, dtype=np.uint32) for a, k in zip(addr, (1, 1, 3))]
    finally:
        mem.free()
    for g, want, k in zip(got, (px, member, xyz), (1, 1, 3)):
        assert g[1 : 1 + k * total].tobytes() == want.tobytes()
        assert g[0] == 0x7FC00000 and (g[1 + k * total :] == 0x7FC00000).all()  # nothing outside


def test_what_ends_the_validity(odd):
    """VOFOD_ERR_NOT_PENDING before any call on a handle, after vofod_range_to_points took the synchronous workspace, after
    vofod_reset, vofod_map_apply and vofod_map_shift - and the answer again after the next production call"""
    from map_shift_cases import shifted_offset

    p, dev = odd, odd.dev
    assert p.before_any_call == (NP, NP)
    size = lambda: dev.detection_pixels(allow=(NP,))
    run = lambda: dev.process_batch(p.scans, p.tfs)
    run()
    assert isinstance(size(), tuple)
    w, h = ODD[1], ODD[0]
    dev.range_to_points(ScanData.range_image(np.full(w * h, 5000, dtype=np.uint32), w, h))
    assert size() == NP
    run()
    snapshot = dev.export_map()
    assert isinstance(size(), tuple)  # (an export reads the map: the answer stands)
    dev.apply_map(snapshot)
    assert size() == NP
    db, _ = run()
    span, px, member, xyz = dev.detection_pixels()
    pxc.assert_pixels(span, px, member, xyz, db, p.exp)
    off = [float(v) for v in dev.sp.oparea_offset]
    s = (4, 0, 0)
    assert dev.map_shift(s, shifted_offset(off, s, dev.sp.voxel_size)) == capi.OK
    assert size() == NP
    assert dev.map_shift((-4, 0, 0), tuple(off)) == capi.OK
    run()
    assert isinstance(size(), tuple)
    dev.reset()
    assert size() == NP
