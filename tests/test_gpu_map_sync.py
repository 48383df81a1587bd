"""Map snapshots and deltas on the device (include/vofod.h: vofod_map_export / vofod_map_apply / vofod_broadcast_map; kernels in
vofod_amd/csrc/mapsync.h) against numpy statements of the same sets.  Setting: OS1-128 at 0.25 m with an a-priori map and the
production cycle of tests/test_gpu_stream_route.py (VOFOD_SCAN_AUTO_RAYCAST, sepclusters every second scan)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_detections_equal, assert_scan_debug_equal, far_view, make_pair
from test_gpu_stream_route import compare_cycle, cycle, profiled_calls
from vofod_amd import capi, mapsync, synth
from vofod_amd.detector import VofodError

pytestmark = pytest.mark.gpu

MS_KERNELS = ("k_ms_count", "k_ms_emit", "k_ms_check", "k_ms_scatter")


@pytest.fixture(scope="module")
def world():
    scene = synth.make_scene(21, n_targets=3)
    ap = synth.apriori_points(scene, 0.25, n_voxels=1_000_000, solid_ground_to=-1.2)
    scans = synth.scan_sequence(scene, "os1-128", 16, seed0=300)
    return ap, scans


def fresh(oracle, hip, ap=None, max_batch=4, voxel_size=0.25):
    _, d = make_pair(oracle, hip, "os1-128", voxel_size, max_batch=max_batch)
    if ap is not None:
        d.load_apriori(ap)
    return d


def maps_of(d):
    return {m: d.read_map(m).reshape(-1).view(np.uint32).copy() for m in range(3)}


def assert_maps_equal(a, b):
    for m in range(3):
        np.testing.assert_array_equal(a[m], b[m], err_msg=f"map {m}")


def status_tuple(d):
    s = d.status()
    return (s.detection_its, s.last_detection_id, s.background_pts_sufficient, s.sure_background_sufficient, s.raycast_pending)


def export(d, maps, kind, cap, buf=None, memspace=capi.MEM_HOST):
    n = C.c_size_t(0)
    st = d.lib.map_export(d.h, maps, kind, buf, cap, memspace, C.byref(n))
    return st, n.value


def test_full_snapshot_content_against_numpy(oracle, hip, world):
    ap, scans = world
    d = fresh(oracle, hip, ap)
    for k, s in enumerate(scans[:8]):
        cycle(d, s, k)
    snap = mapsync.decode(d.export_map(capi.MAPS_ALL, full=True))
    assert snap.kind == mapsync.KIND_FULL and snap.base_gen == 0 and snap.new_gen != 0
    cur = maps_of(d)
    init = {m: mapsync.init_bits(m, d.sp.score_init) for m in range(3)}
    for m in range(3):
        idx, bits = snap.records[m]
        np.testing.assert_array_equal(idx, np.flatnonzero(cur[m] != init[m]).astype(np.uint32), err_msg=f"map {m}")
        np.testing.assert_array_equal(bits, cur[m][idx])
    assert len(snap.records[0][0]) > 900_000  # the a-priori voxels at least
    st = d.status()
    assert (snap.detection_its, snap.last_detection_id, snap.background_pts_sufficient, snap.sure_background_sufficient, snap.raycast_pending) == status_tuple(d)
    assert snap.map_size == tuple(st.map_size) and snap.map_offset == pytest.approx(tuple(st.map_offset))
    assert snap.voxel_size == np.float32(0.25) and snap.score_init == np.float32(d.sp.score_init)


def test_restore_into_a_fresh_handle_then_continue(oracle, hip, world):
    ap, scans = world
    own = fresh(oracle, hip, ap)
    k = 0
    while True:
        cycle(own, scans[k], k)
        k += 1
        if own.status().raycast_pending and k >= 6:
            break
    assert own.status().raycast_pending
    rep = fresh(oracle, hip)
    rep.apply_map(own.export_map(capi.MAPS_ALL, full=True))
    assert_maps_equal(maps_of(own), maps_of(rep))
    assert status_tuple(rep) == status_tuple(own)
    n_finished = 0
    for j in range(4):
        _, fin = compare_cycle(own, rep, scans[k + j], k + j, ray_rtol=2e-5)
        n_finished += fin
    assert n_finished >= 2  # the restored raycast pass was finished on the replica as on the owner


def test_delta_chain_and_a_skipped_delta(oracle, hip, world):
    ap, scans = world
    own, rep = fresh(oracle, hip, ap), fresh(oracle, hip)
    for k in range(4):
        cycle(own, scans[k], k)
    full = own.export_map(capi.MAPS_ALL, full=True)
    prev = maps_of(own)
    rep.apply_map(full)
    gen = mapsync.decode(full).new_gen
    for k in range(4, 8):
        cycle(own, scans[k], k)
        delta = own.export_map(capi.MAPS_ALL, full=False)
        cur = maps_of(own)
        snap = mapsync.decode(delta)
        assert snap.kind == mapsync.KIND_DELTA and snap.base_gen == gen
        gen = snap.new_gen
        for m in range(3):
            np.testing.assert_array_equal(snap.records[m][0], np.flatnonzero(cur[m] != prev[m]).astype(np.uint32))
        assert sum(len(r[0]) for r in snap.records.values()) == sum(int((cur[m] != prev[m]).sum()) for m in range(3))
        rep.apply_map(delta)
        assert_maps_equal(cur, maps_of(rep))
        assert status_tuple(rep) == status_tuple(own)
        prev = cur
    # a skipped delta: DELTA_BASE, replica untouched; then the skipped one and the next apply
    cycle(own, scans[8], 8)
    d1 = own.export_map(capi.MAPS_ALL, full=False)
    cycle(own, scans[9], 9)
    d2 = own.export_map(capi.MAPS_ALL, full=False)
    before = maps_of(rep)
    with pytest.raises(VofodError) as e:
        rep.apply_map(d2)
    assert e.value.status == capi.ERR_DELTA_BASE
    assert_maps_equal(before, maps_of(rep))
    with pytest.raises(VofodError) as e:  # a delta of another mask does not fit the chain either
        rep.apply_map(mapsync.encode(mapsync.Snapshot(**{**mapsync.decode(d1).__dict__, "maps": 1, "records": {0: mapsync.decode(d1).records[0]}})))
    assert e.value.status == capi.ERR_DELTA_BASE
    rep.apply_map(d1)
    rep.apply_map(d2)
    assert_maps_equal(maps_of(own), maps_of(rep))
    # owner side: a delta of a mask without a chain
    st, _ = export(own, 1 << capi.MAP_VOXELS, capi.SNAPSHOT_DELTA, 0)
    assert st == capi.ERR_DELTA_BASE


def test_no_stale_derived_images_after_apply(oracle, hip, world):
    ap, scans = world
    own, rep = fresh(oracle, hip, ap), fresh(oracle, hip)
    for k in range(4):
        cycle(own, scans[k], k)
    rep.apply_map(own.export_map(capi.MAPS_ALL, full=True))
    batch = scans[12:16]
    tfs = np.stack([s.tf for s in batch])
    rep.process_batch([s.scan for s in batch], tfs, debug=True, far_only=True)  # occupancy + dilated images now valid
    thr = own.dp.voxel_map__thresholds__new_obstacles
    old = own.read_map(capi.MAP_VOXELS).reshape(-1)
    for k in range(4, 8):
        cycle(own, scans[k], k)
    new = own.read_map(capi.MAP_VOXELS).reshape(-1)
    flipped = int(((old > thr) != (new > thr)).sum())
    assert flipped >= 1, "no voxel crossed new_obstacles: the check would be vacuous"
    rep.apply_map(own.export_map(capi.MAPS_ALL, full=False))
    dr, pr, gr = rep.process_batch([s.scan for s in batch], tfs, debug=True, far_only=True)
    do, po, go = own.process_batch([s.scan for s in batch], tfs, debug=True, far_only=True)
    np.testing.assert_array_equal(pr, po)
    assert_detections_equal(do, dr)
    for a, b in zip(go, gr):
        assert_scan_debug_equal(a, b)
    # the oracle, given the owner's map through the existing entry points
    ref, _ = make_pair(oracle, hip, "os1-128", 0.25, max_batch=4)
    ref.load_apriori(np.zeros((0, 3), np.float32))  # both latches set, as the owner's are
    assert own.status().background_pts_sufficient and own.status().sure_background_sufficient
    for m in (capi.MAP_VOXELS, capi.MAP_FLAGS):
        ref.write_map(m, own.read_map(m))
    dref, pref, gref = ref.process_batch([s.scan for s in batch], tfs, debug=True)
    np.testing.assert_array_equal(pref, pr)
    rel, oref = dr.copy(), dref.copy()
    if len(rel) and len(oref):  # (ids continue each handle's own counter)
        rel["id"] -= rel["id"].min()
        oref["id"] -= oref["id"].min()
    assert_detections_equal(oref, rel)
    for a, b in zip(gref, gr):
        assert_scan_debug_equal(far_view(a), b)


def test_size_query_capacity_and_chain(oracle, hip, world):
    ap, scans = world
    own, rep = fresh(oracle, hip, ap), fresh(oracle, hip)
    for k in range(3):
        cycle(own, scans[k], k)
    full = own.export_map(capi.MAPS_ALL, full=True)
    rep.apply_map(full)
    prev = maps_of(own)
    cycle(own, scans[3], 3)
    st, n = export(own, capi.MAPS_ALL, capi.SNAPSHOT_DELTA, 0)
    assert st == capi.OK
    cur = maps_of(own)
    recs = {m: mapsync.diff_records(cur[m].view(np.float32), prev[m].view(np.float32)) for m in range(3)}
    assert n == mapsync.nbytes([len(recs[m][0]) for m in range(3)])
    short = np.zeros(n - 1, np.uint8)
    st, n2 = export(own, capi.MAPS_ALL, capi.SNAPSHOT_DELTA, n - 1, capi.ptr(short))
    assert st == capi.ERR_CAPACITY and n2 == n
    buf = np.zeros(n, np.uint8)
    st, n3 = export(own, capi.MAPS_ALL, capi.SNAPSHOT_DELTA, n, capi.ptr(buf))
    assert st == capi.OK and n3 == n
    snap = mapsync.decode(buf)
    assert snap.base_gen == mapsync.decode(full).new_gen  # the capacity error did not advance the chain
    expect = mapsync.Snapshot(**{**snap.__dict__, "records": recs})
    assert mapsync.encode(expect).tobytes() == buf.tobytes()
    rep.apply_map(buf)
    assert_maps_equal(cur, maps_of(rep))


class DeviceBuffer:
    """device memory through the HIP runtime the library itself runs on (hipMalloc / hipMemcpy / hipFree via ctypes)"""

    _rt = None

    def __init__(self, n):
        if DeviceBuffer._rt is None:
            DeviceBuffer._rt = C.CDLL("libamdhip64.so")
        self.n, self.ptr = n, C.c_void_p()
        assert self._rt.hipMalloc(C.byref(self.ptr), C.c_size_t(max(n, 1))) == 0

    def to_host(self):
        out = np.zeros(self.n, np.uint8)
        assert self._rt.hipMemcpy(capi.ptr(out), self.ptr, C.c_size_t(self.n), 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free(self):
        if self.ptr:
            self._rt.hipFree(self.ptr)
            self.ptr = C.c_void_p()


def test_device_buffers(oracle, hip, world):
    ap, scans = world
    own, rep_h, rep_d = fresh(oracle, hip, ap), fresh(oracle, hip), fresh(oracle, hip)
    for k in range(3):
        cycle(own, scans[k], k)
    host = own.export_map(capi.MAPS_ALL, full=True)
    dev = DeviceBuffer(host.size)
    st, n = export(own, capi.MAPS_ALL, capi.SNAPSHOT_FULL, host.size, dev.ptr, capi.MEM_DEVICE)
    assert st == capi.OK and n == host.size
    got = dev.to_host()
    same = np.ones(n, bool)
    same[56:64] = False  # new_gen: every export has its own
    np.testing.assert_array_equal(got[same], host[same])
    rep_h.apply_map(host)
    assert rep_d.lib.map_apply(rep_d.h, dev.ptr, n, capi.MEM_DEVICE) == capi.OK
    cycle(own, scans[3], 3)
    st, n = export(own, capi.MAPS_ALL, capi.SNAPSHOT_DELTA, 0)
    dd = DeviceBuffer(n)
    st, n = export(own, capi.MAPS_ALL, capi.SNAPSHOT_DELTA, n, dd.ptr, capi.MEM_DEVICE)
    assert st == capi.OK
    delta = dd.to_host()
    assert mapsync.decode(delta).base_gen == mapsync.decode(got).new_gen
    assert rep_d.lib.map_apply(rep_d.h, dd.ptr, n, capi.MEM_DEVICE) == capi.OK
    assert_maps_equal(maps_of(own), maps_of(rep_d))
    # the host replica follows the host export's chain: the device delta is not its next one
    assert rep_h.lib.map_apply(rep_h.h, capi.ptr(delta), n, capi.MEM_HOST) == capi.ERR_DELTA_BASE
    dev.free()
    dd.free()


def test_special_values_round_trip(oracle, hip):
    a, b = fresh(oracle, hip, max_batch=1), fresh(oracle, hip, max_batch=1)
    specials = np.array([0x7F800000, 0x80000000, 0x7FC01234, 0x00000001, 0xFF800000, 0x3F800000], np.uint32)
    rng = np.random.default_rng(3)
    for m in range(3):
        arr = a.read_map(m).reshape(-1).copy()
        pos = np.sort(rng.choice(arr.size, size=len(specials), replace=False))
        arr.view(np.uint32)[pos] = specials
        arr.view(np.uint32)[-1] = specials[2]  # the last voxel (the partial tile of the count pass)
        a.write_map(m, arr)
    snap = a.export_map(capi.MAPS_ALL, full=True)
    b.apply_map(snap)
    assert_maps_equal(maps_of(a), maps_of(b))
    assert sum(len(r[0]) for r in mapsync.decode(snap).records.values()) == 3 * (len(specials) + 1)


def test_error_cases_leave_the_replica_untouched(oracle, hip, world):
    ap, scans = world
    own = fresh(oracle, hip, ap)
    cycle(own, scans[0], 0)
    snap = own.export_map(capi.MAPS_ALL, full=True)
    # geometry
    other = fresh(oracle, hip, voxel_size=0.5, max_batch=1)
    before = maps_of(other)
    with pytest.raises(VofodError) as e:
        other.apply_map(snap)
    assert e.value.status == capi.ERR_SIZE_MISMATCH
    assert_maps_equal(before, maps_of(other))
    del other, before
    # a pending submitted batch
    rep = fresh(oracle, hip)
    before, st0 = maps_of(rep), status_tuple(rep)
    t = rep.batch_submit([s.scan for s in scans[12:14]], np.stack([s.tf for s in scans[12:14]]))
    with pytest.raises(VofodError) as e:
        rep.apply_map(snap)
    assert e.value.status == capi.ERR_BUSY
    rep.batch_collect(t)
    assert_maps_equal(before, maps_of(rep))
    assert status_tuple(rep) == st0
    # records out of order, an index past the map, a bad magic: INVALID_ARG before anything is written
    d = mapsync.decode(snap)
    idx, bits = d.records[0]
    for bad in ((idx[::-1].copy(), bits), (np.append(idx[:-1], np.uint32(own.n_voxels)), bits)):
        b = mapsync.encode(mapsync.Snapshot(**{**d.__dict__, "records": {**d.records, 0: bad}}))
        with pytest.raises(VofodError) as e:
            rep.apply_map(b)
        assert e.value.status == capi.ERR_INVALID_ARG
    b = snap.copy()
    b[0] ^= 0xFF
    with pytest.raises(VofodError) as e:
        rep.apply_map(b)
    assert e.value.status == capi.ERR_INVALID_ARG
    with pytest.raises(VofodError) as e:
        rep.apply_map(snap[:-8])
    assert e.value.status == capi.ERR_INVALID_ARG
    assert_maps_equal(before, maps_of(rep))
    assert status_tuple(rep) == st0


def _same_map(a, b):
    for m in range(3):
        x, y = a.read_map(m).reshape(-1).view(np.uint32), b.read_map(m).reshape(-1).view(np.uint32)
        assert np.array_equal(x, y), f"map {m}"
        del x, y


def test_config5_os2_128x2048_at_01_round_trip(oracle, hip):
    """configs[4]: OS2-128 x 2048 at 0.1 m (M = 301 752 451): two scans with raycast, a full snapshot and a delta of all maps"""
    sensor = "os2-128x2048"
    _, own = make_pair(oracle, hip, sensor, 0.1)
    assert own.n_voxels == 301_752_451
    vs = 0.1
    gx, gy = np.meshgrid(np.arange(-20, 30, vs), np.arange(-20, 30, vs), indexing="ij")
    pts = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.01)], axis=1).astype(np.float32)
    own.load_apriori(pts[np.hypot(pts[:, 0], pts[:, 1]) < 30])
    scans = synth.scan_sequence(synth.bench_scene(), sensor, 3, seed0=1000)
    for k in range(2):
        cycle(own, scans[k], k)
    _, rep = make_pair(oracle, hip, sensor, 0.1)
    own.lib.profile_enable(own.h, 1)
    rep.lib.profile_enable(rep.h, 1)
    rep.apply_map(own.export_map(capi.MAPS_ALL, full=True))
    _same_map(own, rep)
    cycle(own, scans[2], 2)
    delta = own.export_map(capi.MAPS_ALL, full=False)
    assert mapsync.decode(delta).kind == mapsync.KIND_DELTA
    rep.apply_map(delta)
    _same_map(own, rep)
    assert status_tuple(own) == status_tuple(rep)
    calls = {**profiled_calls(own.lib, own), **{k + "@rep": v for k, v in profiled_calls(rep.lib, rep).items()}}
    assert calls.get("k_ms_count", 0) >= 6 and calls.get("k_ms_emit", 0) >= 3, calls
    assert calls.get("k_ms_check@rep", 0) >= 1 and calls.get("k_ms_scatter@rep", 0) >= 2, calls


def test_one_rank_broadcast(oracle, hip, world):
    from vofod_amd import dist as vdist

    ap, scans = world
    own = fresh(oracle, hip, ap)
    for k in range(3):
        cycle(own, scans[k], k)
    first = mapsync.decode(own.export_map(capi.MAPS_ALL, full=True))
    st, n = export(own, capi.MAPS_ALL, capi.SNAPSHOT_FULL, 0)
    before = maps_of(own)
    comm = vdist.CabiComm(hip, rank=0, world=1, device=0)
    try:
        assert comm.broadcast_map(own, root=0, maps=capi.MAPS_ALL, full=True) == n
        with pytest.raises(VofodError) as e:  # the root's export fails (no chain for this mask): the call returns its status
            comm.broadcast_map(own, root=0, maps=1 << capi.MAP_VOXELS, full=False)
        assert e.value.status == capi.ERR_DELTA_BASE
    finally:
        comm.close()
    assert_maps_equal(before, maps_of(own))
    nxt = mapsync.decode(own.export_map(capi.MAPS_ALL, full=False))
    assert nxt.base_gen not in (0, first.new_gen)  # the chain moved on to the broadcast's export ...
    assert all(len(r[0]) == 0 for r in nxt.records.values())  # ... which left the shadows equal to the maps
