"""vofod_detection_points (k_det_points, detection_points.h): the member voxels and the AABB of every detection, asked for after
production calls - no debug view on the HIP side.  Expected values come from the oracle's debug view alone
(detection_points_cases.py; test_detection_points_cpu.py checks that construction on the oracle itself): indices and AABBs are
compared exactly, points bit for bit.

The recipe and the scenes are those of test_gpu_tail_edges.py (OS1-16, 0.25 m voxels, four frames, one Bench for the file), the
routes too:
  batch   read-only batch, k_frame_lds_far + k_tail_far (members of a cluster ascending in the list);
  full    the same under VOFOD_CLOSE_FIRST=0: k_frame_lds_full + k_tail_prep / k_explore / k_tail_finish (list in arrival order);
  scan    single map-updating scans, k_far_final + k_tail_far.
The production call's kernel list is asserted as that file asserts it, and k_det_points ran exactly once per query with
detections - under the default switches only (tools/run_fallback_matrix.sh style runs set VOFOD_* from outside: the kernel must
not care which route filled the workspace)."""
import ctypes as C

import numpy as np
import pytest

import detection_points_cases as dpc
from test_gpu_tail_edges import Bench, _assert_tail, _profiled, _route_checked
from vofod_amd import capi

pytestmark = pytest.mark.gpu

ROUTES = ["batch", "full", "scan"]


@pytest.fixture(scope="module")
def bench(oracle, hip):
    b = Bench(oracle, hip)
    b.oracle_cache = {}
    yield b
    b.close()


def _reload_sheet(bench):
    """after vofod_reset on both sides (ids at zero, latches dropped): the recipe's apriori sheet again, which sets both latches"""
    zz, yy, xx = np.nonzero(np.isinf(bench.base))
    sheet = bench.world(np.stack([xx, yy, zz], axis=1)).astype(np.float32)
    for d in (bench.ref, bench.dev):
        d.load_apriori(sheet)


def _oracle_batch(bench, name):
    """(detections, per-frame counts, expectation per frame) of the loaded scene's batch, once per scene"""
    key = ("batch", name)
    if key not in bench.oracle_cache:
        da, pa, gs = bench.ref.process_batch(bench.scans, bench.tfs, debug=True)
        dpc.self_check(da, pa, gs)
        bench.oracle_cache[key] = (da, pa, [dpc.expected_frame(g) for g in gs])
    return bench.oracle_cache[key]


def _oracle_scan(bench, name, f):
    key = ("scan", name, f)
    if key not in bench.oracle_cache:
        d1, g1 = bench.ref.process_scan(bench.scans[f], bench.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
        dpc.self_check(d1, [len(d1)], [g1])
        bench.oracle_cache[key] = (d1, dpc.expected_frame(g1))
    return bench.oracle_cache[key]


def _same_detections(want, got):
    """frames and point counts of the production call are the oracle's (ids count on from call to call on either side)"""
    assert len(want) == len(got)
    np.testing.assert_array_equal(got["frame"], want["frame"])
    np.testing.assert_array_equal(got["n_points"], want["n_points"])
    np.testing.assert_allclose(got["position"], want["position"], atol=1e-3)


def _query(dev, checked, source=capi.POINTS_SYNC, n_dets=None):
    (ext, pts, idx), ran = _profiled(dev, lambda: dev.detection_points(source))
    if checked:
        assert ran == ({"k_det_points": 1} if (n_dets is None or n_dets) else {}), ran  # (the size query in front launches nothing)
    return ext, pts, idx


def _batch_case(bench, name, full, monkeypatch):
    checked = _route_checked()
    if full:
        monkeypatch.setenv("VOFOD_CLOSE_FIRST", "0")
    scene = dpc.load(bench, name)
    dev = bench.dev
    da, pa, exp = _oracle_batch(bench, name)
    (db, pb), ran = _profiled(dev, lambda: dev.process_batch(bench.scans, bench.tfs))
    np.testing.assert_array_equal(pb, pa)
    _same_detections(da, db)
    if checked:
        host_tail = None if scene.trips == "open" else scene.trips is not None
        if full:
            assert "k_frame_lds_full" in ran and "k_frame_lds_far" not in ran and "k_tail_far" not in ran, ran
            assert ran.get("k_tail_finish", 0) == 1 and ran.get("k_explore", 0) >= 1, ran
            _assert_tail(ran, "k_tail_prep", host_tail)
        else:
            assert "k_frame_lds_far" in ran and "k_frame_lds_full" not in ran and "k_tail_prep" not in ran, ran
            _assert_tail(ran, "k_tail_far", host_tail, host_fill=scene.trips == "radius")
        assert "k_det_points" not in ran, ran
    ext, pts, idx = _query(dev, checked)
    dpc.assert_points(ext, pts, idx, db, exp)
    print(f"\n[detection points] {name} {'full' if full else 'batch'}: {len(ext)} detections, {len(pts)} points, largest {int(ext['count'].max())}")
    return ext, pts, idx


def _scan_case(bench, name):
    checked = _route_checked()
    scene = dpc.load(bench, name)
    dev = bench.dev
    for f in scene.scan_frames:
        d1, exp = _oracle_scan(bench, name, f)
        b, ran = _profiled(dev, lambda: dev.process_scan(bench.scans[f], bench.tf))
        _same_detections(d1, b)
        if checked:
            assert ran.get("k_far_final", 0) == 1 and "k_tail_prep" not in ran and "k_det_points" not in ran, ran
            trips = scene.trips if f == 0 or scene.trips in ("radius", "open") else None
            _assert_tail(ran, "k_tail_far", None if trips == "open" else trips in ("clusters", "members", "radius"), host_fill=trips == "radius")
        ext, pts, idx = _query(dev, checked)
        dpc.assert_points(ext, pts, idx, b, [exp])
        bench.reset_maps()


# ---------------------------------------------------------------------------------------------------- 1. three routes x scenes
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", dpc.ROUTE_SCENES)
def test_routes(bench, monkeypatch, name, route):
    """the production call, then the points: member_512 (720 members in 11 blocks), 16 and 17 detections (17: host tail in a batch,
    device_tail_overflow_records in a scan), 1025 candidate members (TAIL_FB_MEMBERS: host tail, lists beyond the tail's capacity
    leave the frame kernel unordered), 65 candidate clusters, the degenerate shapes"""
    if route == "scan":
        _scan_case(bench, name)
    else:
        _batch_case(bench, name, route == "full", monkeypatch)


# ------------------------------------------------------------------------------------------------------------ 2. large members
@pytest.mark.parametrize("route", ["batch", "full", "scan"])
@pytest.mark.parametrize("name", dpc.LARGE_SCENES)
def test_large_members(bench, monkeypatch, name, route):
    """one detection of 343 voxels (more than a tile of 256 list entries), of 576 (more than the kernel's LDS list: two passes,
    ranks counted tile by tile) and of 729, beside a pair"""
    if route == "scan":
        _scan_case(bench, name)
    else:
        ext, _, _ = _batch_case(bench, name, route == "full", monkeypatch)
        assert int(ext["count"].max()) == dpc.LARGEST[name]


# ------------------------------------------------------------------------------------------------------------------ 3. weights
@pytest.mark.parametrize("route", ["batch", "scan"])
def test_weights(bench, monkeypatch, route):
    """cells hit 1 + (i % 5) times and one member cell hit 300 times (the extras path of the lean emission's byte counters): the
    records carry those counts"""
    if route == "scan":
        _scan_case(bench, "weights")
        return
    ext, pts, idx = _batch_case(bench, "weights", False, monkeypatch)
    _, hits = dpc.weights_hits(dpc.SCENES["weights"]())
    n0 = int(ext["count"][ext["frame"] == 0].sum())
    assert sorted(pts["range"][:n0].tolist()) == sorted(hits.tolist()) and int(pts["range"][:n0].max()) == dpc.HEAVY
    assert (pts["range"][n0:] == 1).all()


# ------------------------------------------------------------------------------------------------------------ 4. lean emission
def test_stale_records_under_lean_emission(bench, monkeypatch):
    """the far-only debug view of OTHER frames first (full emission: complete, plausible records in every slot of the workspace),
    then the scene's production batch (lean: only the pure-far bricks' records are written): the points are the scene's, and the
    same bytes come back under VOFOD_LEAN_EMIT=0"""
    dev = bench.dev
    dpc.load(bench, "member_512")
    other = list(bench.scans)

    def run():
        dev.process_batch(other, bench.tfs, debug=True, far_only=True)
        dpc.load(bench, "detections_16")
        da, pa, exp = _oracle_batch(bench, "detections_16")
        db, pb = dev.process_batch(bench.scans, bench.tfs)
        np.testing.assert_array_equal(pb, pa)
        ext, pts, idx = dev.detection_points()
        dpc.assert_points(ext, pts, idx, db, exp)
        return ext, pts, idx

    lean = run()
    monkeypatch.setenv("VOFOD_LEAN_EMIT", "0")
    full = run()
    for a, b, k in zip(lean, full, ("ext", "points", "index")):
        if k == "ext":
            a, b = a.copy(), b.copy()
            a["id"], b["id"] = 0, 0  # (the ids count on)
        assert a.tobytes() == b.tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- 5. pipelined
def test_pipelined_tickets(bench):
    """three tickets with the frames in different orders, collected in order, each queried after its collect and the first once
    more after the third; NOT_PENDING before a collect, for a reused ticket number before its new collect, and for ticket 0 after
    a synchronous scan in its workspace - which VOFOD_POINTS_SYNC then answers for"""
    dev = bench.dev
    dpc.load(bench, "member_512")
    _, _, exp = _oracle_batch(bench, "member_512")
    scans, tfs = bench.scans, bench.tfs
    orders = [[0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2]]

    def submit(order):
        return dev.batch_submit([scans[i] for i in order], tfs[order])

    def check(ticket, order, dets):
        ext, pts, idx = dev.detection_points(ticket)
        dpc.assert_points(ext, pts, idx, dets, [exp[i] for i in order])

    tickets = [submit(o) for o in orders]
    assert tickets == [0, 1, 2]
    for t in tickets:
        assert dev.detection_points(t, allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
    assert dev.detection_points(capi.POINTS_SYNC, allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING  # (ticket 0 took the synchronous workspace)
    dets = []
    for t, o in zip(tickets, orders):
        d, per = dev.batch_collect(t)
        dets.append(d)
        check(t, o, d)
        for later in tickets[t + 1:]:
            assert dev.detection_points(later, allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
    check(0, orders[0], dets[0])  # still there after the others were collected
    check(1, orders[1], dets[1])
    # a ticket number is reused
    t0 = submit(orders[2])
    assert t0 == 0
    assert dev.detection_points(0, allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
    check(1, orders[1], dets[1])  # (another workspace: untouched)
    d0, _ = dev.batch_collect(t0)
    check(0, orders[2], d0)
    assert dev.detection_points(capi.POINTS_SYNC, allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING  # (a ticket's, not a synchronous call's)
    # a synchronous scan in ticket 0's workspace
    d1, exp1 = _oracle_scan(bench, "member_512", 1)
    b = dev.process_scan(scans[1], bench.tf, flags=capi.SCAN_NO_MAP_UPDATE)
    assert dev.detection_points(0, allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
    ext, pts, idx = dev.detection_points(capi.POINTS_SYNC)
    dpc.assert_points(ext, pts, idx, b, [exp1])
    check(1, orders[1], dets[1])


# ----------------------------------------------------------------------------------------------------------------- 6. contract
def _raw(dev, source, ext, ext_cap, pts, idx, pts_cap, memspace=capi.MEM_HOST):
    n_ext, n_pts = C.c_size_t(12345), C.c_size_t(12345)
    st = dev.lib.detection_points(dev.h, source, capi.ptr(ext), ext_cap, C.byref(n_ext), capi.ptr(pts), capi.ptr(idx), pts_cap, C.byref(n_pts), memspace)
    return st, n_ext.value, n_pts.value


def test_contract(bench):
    dev = bench.dev
    checked = _route_checked()
    dpc.load(bench, "degenerate")
    _, pa, exp = _oracle_batch(bench, "degenerate")
    db, pb = dev.process_batch(bench.scans, bench.tfs)
    n, total = len(db), int(db["n_points"].sum())
    assert n == int(pa.sum()) and total > n
    # a size query launches nothing
    (st, ne, npts), ran = _profiled(dev, lambda: _raw(dev, capi.POINTS_SYNC, None, 0, None, None, 0))
    assert (st, ne, npts) == (capi.OK, n, total) and (not checked or ran == {}), (st, ne, npts, ran)
    # capacities one too small, ext and points in turn: both counts, nothing written, nothing launched
    for ext_cap, pts_cap in ((n - 1, total), (n, total - 1)):
        ext = np.full(n, 0xAB, dtype=np.uint8).repeat(40).view(capi.DETECTION_EXTENT)
        pts = np.full(total * 16, 0xCD, dtype=np.uint8).view(capi.POINT_XYZR)
        idx = np.full(total, 0xEFEFEFEF, dtype=np.uint32)
        (st, ne, npts), ran = _profiled(dev, lambda: _raw(dev, capi.POINTS_SYNC, ext, ext_cap, pts, idx, pts_cap))
        assert (st, ne, npts) == (capi.ERR_CAPACITY, n, total) and (not checked or ran == {}), (st, ne, npts, ran)
        assert (ext.view(np.uint8) == 0xAB).all() and (pts.view(np.uint8) == 0xCD).all() and (idx == 0xEFEFEFEF).all()
    # exact capacities: the answer (ext alone and points alone too)
    ext, pts, idx = dev.detection_points()
    dpc.assert_points(ext, pts, idx, db, exp)
    ext2 = np.zeros(n, dtype=capi.DETECTION_EXTENT)
    assert _raw(dev, capi.POINTS_SYNC, ext2, n, None, None, 0) == (capi.OK, n, total) and ext2.tobytes() == ext.tobytes()
    pts2 = np.zeros(total, dtype=capi.POINT_XYZR)
    assert _raw(dev, capi.POINTS_SYNC, None, 0, pts2, None, total) == (capi.OK, n, total) and pts2.tobytes() == pts.tobytes()
    # bad arguments
    e1, p1, i1 = np.zeros(n, dtype=capi.DETECTION_EXTENT), np.zeros(total, dtype=capi.POINT_XYZR), np.zeros(total, dtype=np.uint32)
    for source in (8, -2):
        assert _raw(dev, source, e1, n, p1, i1, total)[0] == capi.ERR_INVALID_ARG
    assert _raw(dev, capi.POINTS_SYNC, e1, n, p1, i1, total, memspace=2)[0] == capi.ERR_INVALID_ARG
    assert _raw(dev, capi.POINTS_SYNC, e1, n, None, i1, total)[0] == capi.ERR_INVALID_ARG  # index without points
    ok = C.c_size_t(0)
    assert dev.lib.detection_points(dev.h, -1, None, 0, None, None, None, 0, C.byref(ok), capi.MEM_HOST) == capi.ERR_INVALID_ARG
    assert dev.lib.detection_points(dev.h, -1, None, 0, C.byref(ok), None, None, 0, None, capi.MEM_HOST) == capi.ERR_INVALID_ARG
    assert _raw(dev, 3, e1, n, p1, i1, total)[0] == capi.ERR_NOT_PENDING  # a ticket never submitted
    # a batch without detections: OK, 0 / 0, no launch
    n_px = bench.scans[0].width * bench.scans[0].height
    from vofod_amd.detector import ScanData

    empty = ScanData(x=np.zeros(n_px, np.float32), y=np.zeros(n_px, np.float32), z=np.zeros(n_px, np.float32), width=bench.scans[0].width, height=bench.scans[0].height, stride_bytes=4)
    d0, p0 = dev.process_batch([empty] * 4, bench.tfs)
    assert len(d0) == 0
    (st, ne, npts), ran = _profiled(dev, lambda: _raw(dev, capi.POINTS_SYNC, e1, n, p1, i1, total))
    assert (st, ne, npts) == (capi.OK, 0, 0) and (not checked or ran == {}), (st, ne, npts, ran)
    # a collect with too small an array returns VOFOD_ERR_CAPACITY and leaves nothing valid.  include/vofod.h: the ticket of a
    # device-tail batch stays pending, a batch that took the host tail (VOFOD_DEVICE_TAIL=0) is consumed by the failing call
    import os

    arr = (capi.Scan * 4)(*[sc.as_c() for sc in bench.scans])
    tfa = np.ascontiguousarray(bench.tfs, dtype=np.float32).reshape(4, 12)
    ticket = C.c_int(-1)
    assert dev.lib.batch_submit(dev.h, arr, capi.ptr(tfa), 4, C.byref(ticket)) == capi.OK
    tk = ticket.value
    dets, per, n_out = np.zeros(n, dtype=capi.DETECTION), np.zeros(4, dtype=np.uint32), C.c_size_t(0)
    assert dev.lib.batch_collect(dev.h, tk, capi.ptr(dets), 1, capi.ptr(per), C.byref(n_out)) == capi.ERR_CAPACITY and n_out.value == n
    assert _raw(dev, tk, e1, n, p1, i1, total)[0] == capi.ERR_NOT_PENDING
    st = dev.lib.batch_collect(dev.h, tk, capi.ptr(dets), n, capi.ptr(per), C.byref(n_out))
    if os.environ.get("VOFOD_DEVICE_TAIL") == "0":
        assert st == capi.ERR_NOT_PENDING and _raw(dev, tk, e1, n, p1, i1, total)[0] == capi.ERR_NOT_PENDING
    else:
        assert st == capi.OK and n_out.value == n
        ext, pts, idx = dev.detection_points(tk)
        dpc.assert_points(ext, pts, idx, dets, exp)
    # reset ends every source
    dev.process_batch(bench.scans, bench.tfs)
    assert _raw(dev, capi.POINTS_SYNC, None, 0, None, None, 0)[0] == capi.OK
    try:
        dev.reset()
        assert _raw(dev, capi.POINTS_SYNC, None, 0, None, None, 0)[0] == capi.ERR_NOT_PENDING
        assert _raw(dev, tk, None, 0, None, None, 0)[0] == capi.ERR_NOT_PENDING
    finally:
        bench.ref.reset()
        _reload_sheet(bench)  # the recipe's state for the tests behind this one


# ------------------------------------------------------------------------------------------------------------ 7. device output
def test_device_output(bench):
    """points and index into device buffers on the handle's device - at addresses that are 4-byte but not 16-byte aligned - equal
    the host-memspace answer byte for byte, and nothing is written around them.  The buffers are hipMalloc'ed through ctypes from
    the runtime the library loaded, as test_gpu_frame_inputs.py allocates its device inputs: the pointer is all the C-ABI sees."""
    rt = C.CDLL("libamdhip64.so")
    rt.hipMalloc.argtypes, rt.hipMemcpy.argtypes, rt.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    dev = bench.dev
    dpc.load(bench, "block_8x8x9")
    _, _, exp = _oracle_batch(bench, "block_8x8x9")
    db, _ = dev.process_batch(bench.scans, bench.tfs)
    ext, pts, idx = dev.detection_points()
    dpc.assert_points(ext, pts, idx, db, exp)
    total = len(pts)
    hbuf, hibuf = np.full(total * 4 + 8, 0x7FC00000, dtype=np.uint32), np.full(total + 8, 0xFFFFFFFF, dtype=np.uint32)
    pb, pi = C.c_void_p(), C.c_void_p()
    assert rt.hipMalloc(C.byref(pb), hbuf.nbytes) == 0 and rt.hipMalloc(C.byref(pi), hibuf.nbytes) == 0
    try:
        assert rt.hipMemcpy(pb, capi.ptr(hbuf), hbuf.nbytes, 1) == 0 and rt.hipMemcpy(pi, capi.ptr(hibuf), hibuf.nbytes, 1) == 0  # host to device
        d_pts, d_idx = pb.value + 4, pi.value + 4  # one word in: 4-byte aligned only
        assert pb.value % 16 == 0 and d_pts % 16 != 0
        ext_d, none_p, none_i = dev.detection_points(device_out=(d_pts, d_idx, total))
        assert none_p is None and none_i is None and ext_d.tobytes() == ext.tobytes()
        assert dev.detection_points(device_out=(d_pts + 2, None, total), allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG  # 2-byte aligned
        got, goti = np.zeros_like(hbuf), np.zeros_like(hibuf)
        assert rt.hipMemcpy(capi.ptr(got), pb, got.nbytes, 2) == 0 and rt.hipMemcpy(capi.ptr(goti), pi, goti.nbytes, 2) == 0  # device to host
    finally:
        assert rt.hipFree(pb) == 0 and rt.hipFree(pi) == 0
    assert got[1 : 1 + total * 4].tobytes() == pts.tobytes() and goti[1 : 1 + total].tobytes() == idx.tobytes()
    assert got[0] == 0x7FC00000 and (got[1 + total * 4 :] == 0x7FC00000).all() and goti[0] == 0xFFFFFFFF and (goti[1 + total :] == 0xFFFFFFFF).all()  # nothing outside


# ---------------------------------------------------------------------------------------------- 7b. what else ends the validity
def test_launch_groups_and_range_to_points_end_the_validity(bench):
    """a vofod_process_batch of more frames than max_batch_frames (4 here) runs as successive launch groups that overwrite each
    other's lists: nothing valid afterwards; vofod_range_to_points stages its input in the synchronous workspace: VOFOD_POINTS_SYNC
    and ticket 0 end there, another ticket's workspace does not"""
    from vofod_amd.detector import ScanData

    dev = bench.dev
    dpc.load(bench, "member_512")
    _, _, exp = _oracle_batch(bench, "member_512")
    scans, tfs = bench.scans, bench.tfs
    size = lambda src: _raw(dev, src, None, 0, None, None, 0)[0]
    db, _ = dev.process_batch(scans, tfs)
    assert size(capi.POINTS_SYNC) == capi.OK
    d8, p8 = dev.process_batch(scans + scans, np.concatenate([tfs, tfs]))
    assert len(d8) == 2 * len(db) and p8.tolist() == 2 * dpc.PER_FRAME["member_512"]
    assert size(capi.POINTS_SYNC) == capi.ERR_NOT_PENDING
    w, h = scans[0].width, scans[0].height
    image = ScanData.range_image(np.full(w * h, 5000, dtype=np.uint32), w, h)
    dev.process_batch(scans, tfs)
    assert size(capi.POINTS_SYNC) == capi.OK
    dev.range_to_points(image)
    assert size(capi.POINTS_SYNC) == capi.ERR_NOT_PENDING
    t0, t1 = dev.batch_submit(scans, tfs), dev.batch_submit(scans, tfs)
    assert (t0, t1) == (0, 1)
    dev.batch_collect(t0)
    d1, _ = dev.batch_collect(t1)
    assert size(0) == capi.OK and size(1) == capi.OK
    dev.range_to_points(image)
    assert size(0) == capi.ERR_NOT_PENDING
    ext, pts, idx = dev.detection_points(1)
    dpc.assert_points(ext, pts, idx, d1, exp)


# --------------------------------------------------------------------------------------------------------- 8. nothing else moved
def test_queries_change_nothing(bench):
    """the same call sequence on the HIP side without and with interleaved queries, and on the oracle: detections and ids equal"""
    from helpers import assert_detections_equal

    ref, dev = bench.ref, bench.dev
    for d in (ref, dev):  # (the oracle's answers are cached in this file: the two id counters are not in step until here)
        d.reset()
    _reload_sheet(bench)
    dpc.load(bench, "gates")
    scans, tfs = bench.scans, bench.tfs

    def sequence(d, ask):
        out = []
        q = (lambda *a: d.detection_points(*a)) if ask else (lambda *a: None)
        a, pa = d.process_batch(scans, tfs)
        q()
        out += [a, pa]
        if d is dev:
            t1, t2 = d.batch_submit(scans, tfs), d.batch_submit(scans[::-1], tfs[::-1])
            b, pb = d.batch_collect(t1)
            q(t1)
            c, pc = d.batch_collect(t2)
            q(t2)
            q(t1)
        else:
            b, pb = d.process_batch(scans, tfs)
            c, pc = d.process_batch(scans[::-1], tfs[::-1])
        out += [b, pb, c, pc]
        for f in (0, 1):
            out.append(d.process_scan(scans[f], bench.tf, flags=capi.SCAN_NO_MAP_UPDATE))
            q()
        q()
        out.append(d.process_batch(scans, tfs)[0])
        return out

    for ask in (False, True):
        want, got = sequence(ref, False), sequence(dev, ask)
        for x, y in zip(want, got):
            if x.dtype == capi.DETECTION:
                assert_detections_equal(x, y)
            else:
                np.testing.assert_array_equal(y, x)
