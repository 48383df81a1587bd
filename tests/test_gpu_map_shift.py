"""vofod_map_shift on the device (include/vofod.h, vofod_amd/csrc/map_shift.h) against the numpy statement of
map_shift_cases.shift_statement, and the handle behind a shift against a handle created at the new offset: the CPU oracle as
handle B of test_map_shift_cpu.py, which receives the statement applied to the maps."""
import os

import numpy as np
import pytest

import map_shift_cases as mc
from helpers import assert_detections_equal, assert_scan_debug_equal, far_view, sync_maps
from vofod_amd import capi, synth
from vofod_amd.detector import VofodError

pytestmark = pytest.mark.gpu

BASE = (40.0, 20.0, -1.25)
# (oparea_size, voxel size) -> map sizes
SMALL = ((10.0, 6.0, 4.0), 0.5)     # 21 x 13 x 9: M = 2457, odd, below one tile of the kernel
MEDIUM = ((30.0, 20.0, 8.0), 0.25)  # 121 x 81 x 33: M = 323 433, M % 4 != 0, many tiles
SIZES = {"21x13x9": (SMALL, (21, 13, 9)), "121x81x33": (MEDIUM, (121, 81, 33))}


def _shifts(S):
    return [(1, 0, 0), (-1, 0, 0), (3, 0, 0), (-3, 0, 0), (4, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (2, -3, 1), (-5, 4, -2), (S[0] - 1, 0, 0), (0, S[1], 0), (0, 0, 0)]


CASES = [(name, s) for name, (_, S) in SIZES.items() for s in _shifts(S)]


def _det(lib, which, offset=BASE, **kw):
    (size, vs), S = SIZES[which]
    d = mc.make_det(lib, voxel_size=vs, oparea_offset=offset, oparea_size=size, **kw)
    assert d.map_size == S
    return d, vs


def _fill(det, seed):
    """random 32-bit patterns (with +inf, -0.0f, NaNs) in all three maps; returns them"""
    rng = np.random.default_rng(seed)
    sx, sy, sz = det.map_size
    bits = {}
    for which in mc.MAPS:
        bits[which] = mc.random_bits(rng, (sz, sy, sx))
        mc.write_bits(det, which, bits[which])
    return bits


def _offset_bits(det):
    return np.array(list(det.status().map_offset), dtype=np.float32).view(np.uint32).tolist()


def _snapshot_state(det):
    return {w: mc.read_bits(det, w).copy() for w in mc.MAPS}, mc.status_tuple(det)


def _assert_unchanged(det, before, what):
    maps, st = before
    assert mc.status_tuple(det) == st, what
    for w in mc.MAPS:
        np.testing.assert_array_equal(mc.read_bits(det, w), maps[w], err_msg=f"{what}: map {w}")


# ------------------------------------------------------------------------------------------------ (a) the statement
@pytest.mark.parametrize("which,s", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_shift_equals_the_statement(hip, which, s):
    det, vs = _det(hip, which)
    bits = _fill(det, seed=CASES.index((which, s)))
    off = mc.shifted_offset(BASE, s, vs)
    assert det.map_shift(s, off) == capi.OK
    for w in mc.MAPS:
        want = mc.shift_statement(bits[w], s, mc.init_bits(det, w))
        np.testing.assert_array_equal(mc.read_bits(det, w), want, err_msg=f"map {w}")
    fresh, _ = _det(hip, which, offset=off)
    assert _offset_bits(det) == _offset_bits(fresh)
    assert det.map_offset == fresh.map_offset and tuple(det.status().map_size) == tuple(fresh.status().map_size)


# ------------------------------------------------------------------------------------------------ (b) there and back
@pytest.mark.parametrize("s", [(2, -3, 1), (-5, 0, 0), (3, 1, 0)], ids=str)
def test_two_shifts_in_a_row_the_second_undoing_the_first(hip, s):
    det, vs = _det(hip, "121x81x33")
    bits = _fill(det, seed=7)
    off0 = _offset_bits(det)
    back = tuple(-v for v in s)
    assert det.map_shift(s, mc.shifted_offset(BASE, s, vs)) == capi.OK
    assert det.map_shift(back, mc.shifted_offset(BASE, (0, 0, 0), vs)) == capi.OK
    assert _offset_bits(det) == off0
    for w in mc.MAPS:
        init = mc.init_bits(det, w)
        want = mc.shift_statement(mc.shift_statement(bits[w], s, init), back, init)
        got = mc.read_bits(det, w)
        np.testing.assert_array_equal(got, want, err_msg=f"map {w}")
        # the overlap is back, the rim is init
        sz, sy, sx = want.shape
        keep = np.zeros(want.shape, dtype=bool)
        keep[max(0, s[2]):sz + min(0, s[2]), max(0, s[1]):sy + min(0, s[1]), max(0, s[0]):sx + min(0, s[0])] = True
        np.testing.assert_array_equal(got[keep], bits[w][keep])
        assert (got[~keep] == np.uint32(init)).all() and (~keep).any()


# ------------------------------------------------------------------------------------------------ (c) continuation against the oracle
def _compare_maps(ref, dev, what):
    """the tolerances of test_gpu_stream_route.compare_cycle behind a raycast update"""
    ma, mb = ref.read_map(capi.MAP_VOXELS), dev.read_map(capi.MAP_VOXELS)
    fin = np.isfinite(ma)
    np.testing.assert_array_equal(np.isfinite(mb), fin, err_msg=what)
    np.testing.assert_allclose(mb[fin], ma[fin], rtol=1e-4, atol=1e-3, err_msg=what)  # tolerance: float-atomic accumulation order of the ray lengths
    np.testing.assert_array_equal(dev.read_map(capi.MAP_FLAGS), ref.read_map(capi.MAP_FLAGS), err_msg=what)


def test_continuation_after_a_shift_against_the_oracle(oracle, hip):
    tgt = mc.TARGET_IN_NEW_STRIP
    ref, dev = mc.make_det(oracle), mc.make_det(hip)
    # A's warm-up on both sides (existing parity), from identical maps at every scan
    for d in (ref, dev):
        d.load_apriori(mc.ground_apriori())
    for k, s in enumerate(mc.scans(tgt, 0, mc.N_WARM)):
        da = ref.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        db = dev.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        assert len(da) == len(db), k
        np.testing.assert_array_equal(da["id"], db["id"])
        _compare_maps(ref, dev, f"warm-up scan {k}")
        sync_maps(ref, dev)
    st = dev.status()
    assert not st.raycast_pending and st.detection_its == mc.N_WARM
    id_shift = int(st.last_detection_id)
    assert id_shift > 0 and id_shift == int(ref.status().last_detection_id)
    # the shift on the device; handle B at the new offset with the statement applied to the oracle's own maps
    off = mc.shifted_offset(tuple(dev.sp.oparea_offset), mc.SHIFT, mc.VS)
    own = {w: mc.read_bits(ref, w) for w in mc.MAPS}
    assert dev.map_shift(mc.SHIFT, off) == capi.OK
    b = mc.hand_over(oracle, {w: mc.shift_statement(own[w], mc.SHIFT, mc.init_bits(ref, w)).view(np.float32) for w in mc.MAPS}, oparea_offset=off)
    assert _offset_bits(dev) == _offset_bits(b)
    st = dev.status()
    assert (st.detection_its, st.last_detection_id, st.background_pts_sufficient, st.sure_background_sufficient, st.raycast_pending) == (mc.N_WARM, id_shift, 1, 1, 0)
    _compare_maps(b, dev, "after the shift")  # (the raycast map is compared in the statement tests: no pass is pending here, and the oracle clears it at the next begin where the device's sweep has left it zero)
    n_det = 0
    for k, s in enumerate(mc.continuation_scans(tgt)):
        da = b.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        db = dev.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        print(f"continuation scan {k}: oracle {len(da)} detections (ids {da['id'].tolist()}), HIP {len(db)} (ids {db['id'].tolist()})")
        mc.assert_detections_equal_mod_id(da, db, id_shift)
        _compare_maps(b, dev, f"continuation scan {k}")
        assert b.status().raycast_pending == dev.status().raycast_pending
        sync_maps(b, dev)
        if k == 1:
            (sa, sure_a), (sb, sure_b) = b.sepclusters_begin(allow=(capi.ERR_EMPTY,)), dev.sepclusters_begin(allow=(capi.ERR_EMPTY,))
            assert (sa, sure_a) == (sb, sure_b) and sa == capi.OK and sure_a
            assert b.sepclusters_finish() == capi.OK and dev.sepclusters_finish() == capi.OK
            _compare_maps(b, dev, "after sepclusters")
            sync_maps(b, dev)
        n_det += int((np.abs(da["position"] - np.array(tgt)).max(axis=1) < 1.0).sum()) if len(da) else 0
    assert n_det >= 1  # the oracle detects the box in the strip that only exists after the shift


# ------------------------------------------------------------------------------------------------ (d) the frame kernel after a shift
def _rebase(got, want):
    got = got.copy()
    if len(got) and len(want):
        got["id"] = (got["id"].astype(np.int64) + int(want["id"][0]) - int(got["id"][0])).astype(got["id"].dtype)
    return got


def test_frame_kernel_after_a_shift_off_the_brick_lattice(oracle, hip):
    """0.25 m, a warmed map, a shift by (3, 1, 0) voxels - no multiple of the 4-voxel brick, so the reference lattice of the frame
    kernel is anchored anew - then read-only batches through submit / collect and the far-only debug view"""
    from test_gpu_stream_route import profiled_calls

    sensor, vs, n = "os1-16", 0.25, 4
    s = (3, 1, 0)
    dev = mc.make_det(hip, sensor, vs, max_batch=n)
    warm_scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=0)
    scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=8)
    synth.warm_map(dev, warm_scene, sensor, 8)
    assert not dev.status().raycast_pending
    # 16 rings leave unknown gaps between the rays at any range: a long raycast history is stood in for by turning what the warm-up
    # left unknown into sure air (as test_gpu_frame_inputs.survey_free_space does), and both latches are set - the targets that
    # appear in the batch are then found floating, on both sides
    m = dev.read_map(capi.MAP_VOXELS)
    m[m == np.float32(dev.sp.score_init)] = np.float32(dev.dp.voxel_map__thresholds__frontiers)
    dev.write_map(capi.MAP_VOXELS, m)
    dev.load_apriori(np.zeros((0, 3), dtype=np.float32))
    frames = synth.bench_frames(scene, sensor, n)
    scans, tfs = [f.scan for f in frames], np.stack([f.tf for f in frames])
    dev.lib.profile_enable(dev.h, 1)
    d0, p0 = dev.batch_collect(dev.batch_submit(scans, tfs))  # (the images of the unshifted map exist: k_dilate has run)
    before = profiled_calls(dev.lib, dev)
    pre = {w: mc.read_bits(dev, w) for w in (capi.MAP_VOXELS, capi.MAP_FLAGS)}
    off = mc.shifted_offset(tuple(dev.sp.oparea_offset), s, vs)
    assert dev.map_shift(s, off) == capi.OK
    d1, p1 = dev.batch_collect(dev.batch_submit(scans, tfs))
    after = profiled_calls(dev.lib, dev)
    dev.lib.profile_enable(dev.h, 0)
    if not any(k.startswith("VOFOD_") and k != "VOFOD_TEST_HARNESS_SELFCHECK" for k in os.environ):  # (a fallback switch reroutes the batch)
        assert before.get("k_dilate", 0) >= 1 and before.get("k_frame_lds_far", 0) >= 1, before
        assert after.get("k_map_shift", 0) == 3 and after.get("k_dilate", 0) >= 1 and after.get("k_frame_lds_far", 0) >= 1, after
    # handle B: the oracle at the new offset, the statement applied to the maps as they were
    b = mc.make_det(oracle, sensor, vs, oparea_offset=off, max_batch=n)
    b.load_apriori(np.zeros((0, 3), dtype=np.float32))
    for w in pre:
        want = mc.shift_statement(pre[w], s, mc.init_bits(dev, w))
        np.testing.assert_array_equal(mc.read_bits(dev, w), want)
        mc.write_bits(b, w, want)
    da, pa, ga = b.process_batch(scans, tfs, debug=True)
    assert len(da) >= 4 and max(int((g["clusters"]["is_close"] == 0).sum()) for g in ga) >= 2  # (the oracle on the CPU: 9 detections, 25-28 far clusters a frame)
    np.testing.assert_array_equal(p1, pa)
    assert_detections_equal(da, _rebase(d1, da))
    db, pb, gb = dev.process_batch(scans, tfs, debug=True, far_only=True)  # a second, identical batch
    np.testing.assert_array_equal(pb, pa)
    assert_detections_equal(da, _rebase(db, da))
    for f, (x, y) in enumerate(zip(ga, gb)):
        try:
            assert_scan_debug_equal(far_view(x), y)
        except AssertionError as e:
            raise AssertionError(f"frame {f}: {e}") from e


# ------------------------------------------------------------------------------------------------ (e) refusals change nothing
def test_refusals_change_nothing(hip):
    tgt = mc.TARGET_IN_AREA
    dev = mc.make_det(hip)
    dev.load_apriori(mc.ground_apriori())
    scans = mc.scans(tgt, 0, 2)
    dev.process_scan(scans[0].scan, scans[0].tf)
    s = (4, -2, 0)
    good = mc.shifted_offset(BASE, s, mc.VS)
    # an offset one voxel off, on each axis, and with the wrong sign
    before = _snapshot_state(dev)
    for bad in [mc.shifted_offset(BASE, (5, -2, 0), mc.VS), mc.shifted_offset(BASE, (4, -1, 0), mc.VS), mc.shifted_offset(BASE, (4, -2, 1), mc.VS),
                mc.shifted_offset(BASE, (-4, 2, 0), mc.VS), mc.shifted_offset(BASE, (-2, 4, 0), mc.VS)]:
        assert dev.map_shift(s, bad, allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG, bad
        _assert_unchanged(dev, before, f"offset {bad}")
    assert dev.map_shift((0, 0, 0), good, allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG
    _assert_unchanged(dev, before, "shift 0 with a moved offset")
    # a ticket in flight
    t = dev.batch_submit([scans[1].scan], scans[1].tf[None])
    assert dev.map_shift(s, good, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
    dev.batch_collect(t)
    _assert_unchanged(dev, (before[0], mc.status_tuple(dev)), "ticket in flight")  # (the collect may hand out ids: the maps are compared)
    # a raycast pass pending
    dev.raycast_begin(scans[1].scan, scans[1].tf)
    before = _snapshot_state(dev)
    assert before[1][4] == 1
    assert dev.map_shift(s, good, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
    _assert_unchanged(dev, before, "raycast pending")
    dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION, capi.ERR_RAYCAST_EMPTY))
    # a sepclusters pass pending
    st, sure = dev.sepclusters_begin(allow=(capi.ERR_EMPTY,))
    if st == capi.OK and sure:
        before = _snapshot_state(dev)
        assert dev.map_shift(s, good, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
        _assert_unchanged(dev, before, "sepclusters pending")
        assert dev.sepclusters_finish() == capi.OK
    # nothing pending any more: the same call goes through
    before = _snapshot_state(dev)
    assert dev.map_shift(s, good) == capi.OK
    for w in mc.MAPS:
        np.testing.assert_array_equal(mc.read_bits(dev, w), mc.shift_statement(before[0][w], s, mc.init_bits(dev, w)))


def test_ticket_in_flight_leaves_the_status_alone(hip):
    """the BUSY answer itself, before the ticket is collected: status and maps as they were"""
    dev = mc.make_det(hip)
    dev.load_apriori(mc.ground_apriori())
    sc = mc.scans(mc.TARGET_IN_AREA, 0, 1)[0]
    before = _snapshot_state(dev)
    t = dev.batch_submit([sc.scan], sc.tf[None])
    assert dev.map_shift((1, 0, 0), mc.shifted_offset(BASE, (1, 0, 0), mc.VS), allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
    assert mc.status_tuple(dev) == before[1]
    dev.batch_collect(t)
    for w in mc.MAPS:
        np.testing.assert_array_equal(mc.read_bits(dev, w), before[0][w])


# ------------------------------------------------------------------------------------------------ (f) snapshots
def test_snapshot_chain_ends_at_a_shift(hip):
    s = (2, -1, 1)
    owner, vs = _det(hip, "21x13x9")
    _fill(owner, seed=21)
    off = mc.shifted_offset(BASE, s, vs)
    old = owner.export_map(capi.MAPS_ALL, full=True)
    assert len(owner.export_map(capi.MAPS_ALL, full=False)) == 128  # the chain stands: an empty delta
    assert owner.map_shift(s, off) == capi.OK
    with pytest.raises(VofodError) as e:
        owner.export_map(capi.MAPS_ALL, full=False)
    assert e.value.status == capi.ERR_DELTA_BASE
    with pytest.raises(VofodError) as e:
        owner.apply_map(old)  # a snapshot from before the shift: the header carries the offset
    assert e.value.status == capi.ERR_SIZE_MISMATCH
    new = owner.export_map(capi.MAPS_ALL, full=True)  # a new chain
    fresh, _ = _det(hip, "21x13x9", offset=off)
    fresh.apply_map(new)
    for w in mc.MAPS:
        np.testing.assert_array_equal(mc.read_bits(fresh, w), mc.read_bits(owner, w))
    mc.write_bits(owner, capi.MAP_FLAGS, mc.read_bits(owner, capi.MAP_FLAGS) ^ np.uint32(1))
    fresh.apply_map(owner.export_map(capi.MAPS_ALL, full=False))  # ... on which deltas follow again
    np.testing.assert_array_equal(mc.read_bits(fresh, capi.MAP_FLAGS), mc.read_bits(owner, capi.MAP_FLAGS))
    # the applying side forgets its generation too: the replica goes there and back (the offset bits are the owner's again), and
    # the owner's next delta no longer follows anything it knows
    back = tuple(-v for v in s)
    assert fresh.map_shift(back, mc.shifted_offset(BASE, (0, 0, 0), vs)) == capi.OK
    assert fresh.map_shift(s, off) == capi.OK
    mc.write_bits(owner, capi.MAP_FLAGS, mc.read_bits(owner, capi.MAP_FLAGS) ^ np.uint32(2))
    with pytest.raises(VofodError) as e:
        fresh.apply_map(owner.export_map(capi.MAPS_ALL, full=False))
    assert e.value.status == capi.ERR_DELTA_BASE


# ------------------------------------------------------------------------------------------------ (g) detection points
def test_detection_points_after_a_shift(hip):
    tgt = mc.TARGET_IN_NEW_STRIP
    dev = mc.make_det(hip)
    dets = mc.warm(dev, tgt)[-1]
    assert len(dets) > 0
    ext, pts, idx = dev.detection_points()
    np.testing.assert_array_equal(ext["id"], dets["id"])
    assert dev.map_shift(mc.SHIFT, mc.shifted_offset(BASE, mc.SHIFT, mc.VS)) == capi.OK
    assert dev.detection_points(allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
    for t in range(8):
        assert dev.detection_points(source=t, allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
    s = mc.continuation_scans(tgt)[0]
    dets = dev.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
    ext, pts, idx = dev.detection_points()
    np.testing.assert_array_equal(ext["id"], dets["id"])
    assert int(ext["count"].sum()) == len(pts) == int(dets["n_points"].sum())
