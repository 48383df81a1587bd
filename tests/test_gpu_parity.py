"""GPU parity tests: the HIP path (through its C-ABI) against the CPU oracle on the same seeded inputs.

Bar (north_star): bit-exact voxel indices, weights, centres, cluster membership, close/far flags, classes
and map contents after integer/byte-exact stages; stated tolerances on OBB-derived positions, confidences
and on everything downstream of the float-atomic raycast accumulation.
"""
import ctypes as C
import os

import numpy as np
import pytest

from vofod_amd import capi, synth
from vofod_amd.detector import ScanData, VofodError, cluster, voxel_grid_counted, voxel_grid_weighted

from helpers import assert_detections_equal, assert_scan_debug_equal, far_view, make_pair, sync_maps

pytestmark = pytest.mark.gpu


def _world_cloud(seed, sensor="os1-128"):
    scene = synth.make_scene(seed)
    tf = synth.make_pose(seed)
    s = synth.make_scan(scene, tf, sensor, seed=seed)
    ok = s.range > 0
    p = np.stack([s.x[ok], s.y[ok], s.z[ok]], axis=1).astype(np.float64)
    q = (p @ tf[:, :3].astype(np.float64).T + tf[:, 3]).astype(np.float32)
    return q


@pytest.mark.parametrize("leaf", [0.5, 0.25, 0.1])
@pytest.mark.parametrize("seed", [0, 1])
def test_voxel_grid_weighted_bit_exact(oracle, hip, leaf, seed):
    ref, dev = make_pair(oracle, hip)
    q = _world_cloud(seed)
    for align in (None, (-19.75, -29.75, -1.0), (0.37, -0.11, 0.05)):
        a = voxel_grid_weighted(oracle, q[:, 0], q[:, 1], q[:, 2], leaf, align)
        b = voxel_grid_weighted(hip, q[:, 0], q[:, 1], q[:, 2], leaf, align, handle=dev.h)
        np.testing.assert_array_equal(b[1], a[1])
        np.testing.assert_array_equal(b[0].view(np.uint32), a[0].view(np.uint32))
        for f in ("leaf", "offset", "min_b", "div_b"):
            assert list(getattr(b[2], f)) == list(getattr(a[2], f)), f
        assert int(a[0]["range"].sum()) == q.shape[0]


def test_voxel_grid_edge_cases(oracle, hip):
    ref, dev = make_pair(oracle, hip)
    e = np.zeros(0, dtype=np.float32)
    out, keys, grid, st = voxel_grid_weighted(hip, e, e, e, 0.5, handle=dev.h)
    assert st == capi.OK and out.size == 0
    one = np.float32([[1.3, -2.2, 0.7]])
    a = voxel_grid_weighted(oracle, one[:, 0], one[:, 1], one[:, 2], 0.5)
    b = voxel_grid_weighted(hip, one[:, 0], one[:, 1], one[:, 2], 0.5, handle=dev.h)
    np.testing.assert_array_equal(b[0].view(np.uint32), a[0].view(np.uint32))
    x = np.float32([0, 1e6])
    out, keys, grid, st = voxel_grid_weighted(hip, x, x, x, 0.01, handle=dev.h, allow=(capi.ERR_INDEX_OVERFLOW,))
    assert st == capi.ERR_INDEX_OVERFLOW and out.size == 0
    # many duplicates of one point: weight saturates nothing, count is exact
    d = np.full(100000, 3.21, dtype=np.float32)
    out, keys, grid, st = voxel_grid_weighted(hip, d, d, d, 0.5, handle=dev.h)
    assert out.size == 1 and out["range"][0] == 100000


@pytest.mark.parametrize("leaf,thr", [(1.0, -0.1), (3.0, -0.1), (2.0, -100.0)])
def test_voxel_grid_counted_positional_quirk(oracle, hip, leaf, thr):
    ref, dev = make_pair(oracle, hip)
    rng = np.random.default_rng(5)
    # an index cloud in voxelsAsVoxelPC order (x outer, z inner) with map values as intensity
    occ = rng.random((60, 50, 20)) < 0.08
    xs, ys, zs = np.nonzero(occ)
    inten = rng.choice(np.float32([0.0, -50.0, -200.0, np.inf]), size=xs.size)
    a = voxel_grid_counted(oracle, xs, ys, zs, inten, leaf, thr)
    b = voxel_grid_counted(hip, xs, ys, zs, inten, leaf, thr, handle=dev.h)
    np.testing.assert_array_equal(b[1], a[1])
    np.testing.assert_array_equal(b[0].view(np.uint32), a[0].view(np.uint32))
    assert int(b[0]["range"].sum()) == int((inten > thr).sum())


@pytest.mark.parametrize("leaf,tol", [(0.5, 1.5), (0.25, 1.5), (0.5, 0.7), (0.1, 1.5), (1.0, 2.0), (3.0, 4.0)])
def test_cluster_membership_bit_exact(oracle, hip, leaf, tol):
    ref, dev = make_pair(oracle, hip)
    q = _world_cloud(3)
    if leaf >= 1.0:
        q = q * 4.0
    pts, keys, grid, _ = voxel_grid_weighted(oracle, q[:, 0], q[:, 1], q[:, 2], leaf, (-19.75, -29.75, -1.0))
    la, na = cluster(oracle, pts, keys, grid, tol)
    lb, nb = cluster(hip, pts, keys, grid, tol, handle=dev.h)
    np.testing.assert_array_equal(lb, la)
    assert na == nb


def test_cluster_tolerance_boundary(oracle, hip):
    # lattice chains exactly on the tolerance boundary: 3 voxels apart at tol 1.5 / leaf 0.5
    ref, dev = make_pair(oracle, hip)
    x = np.float32([0.25, 1.75, 3.25, 4.25, 10.25, 10.25, 10.25])
    y = np.float32([0.25, 0.25, 0.25, 0.25, 0.25, 1.25, 2.75])
    z = np.float32([0.25] * 7)
    pts, keys, grid, _ = voxel_grid_weighted(oracle, x, y, z, 0.5)
    la, na = cluster(oracle, pts, keys, grid, 1.5)
    lb, nb = cluster(hip, pts, keys, grid, 1.5, handle=dev.h)
    np.testing.assert_array_equal(lb, la)
    assert na == 5  # {0},{1},{2,3},{4,5},{6}
    # far from the origin the centres are not exact multiples any more: evaluate in float like FLANN does
    off = np.float32(91.3)
    pts2, keys2, grid2, _ = voxel_grid_weighted(oracle, x + off, y + off, z + off, 0.5, (0.05, 0.05, 0.05))
    la, _ = cluster(oracle, pts2, keys2, grid2, 1.5)
    lb, _ = cluster(hip, pts2, keys2, grid2, 1.5, handle=dev.h)
    np.testing.assert_array_equal(lb, la)


def _run_sequence(ref, dev, scans, flags=capi.SCAN_DEFAULT, sep_every=2, debug=True, route=None):
    """Step both detectors through the same scans; every step starts from identical maps.  debug=False: the production call of
    a sensor stream (no debug output: the classification tail runs on the device and writes its frontiers to the map itself).
    `route` (a dict, debug=False only) receives the number of production calls and the kernels they launched (vofod_profile_read)."""
    n_det = 0
    n_calls = 0
    if route is not None and not debug:
        dev.lib.profile_enable(dev.h, 1)

    def step(s, fl):
        nonlocal n_calls
        if debug:
            dr, gr = ref.process_scan(s.scan, s.tf, flags=fl, debug=True)
            dh, gh = dev.process_scan(s.scan, s.tf, flags=fl, debug=True)
            assert_scan_debug_equal(gr, gh)
        else:
            dr = ref.process_scan(s.scan, s.tf, flags=fl)
            dh = dev.process_scan(s.scan, s.tf, flags=fl)
            n_calls += 1
        assert_detections_equal(dr, dh)
        return dr

    for k, s in enumerate(scans):
        dr = step(s, flags)
        n_det += len(dr)
        np.testing.assert_array_equal(dev.read_map(capi.MAP_VOXELS), ref.read_map(capi.MAP_VOXELS))
        np.testing.assert_array_equal(dev.read_map(capi.MAP_FLAGS), ref.read_map(capi.MAP_FLAGS))
        # raycast of this scan, applied after the next detection iteration (vofod_nodelet.cpp:1530-1539)
        if k + 1 < len(scans):
            assert ref.raycast_begin(s.scan, s.tf) == dev.raycast_begin(s.scan, s.tf) == capi.OK
            ra, rb = ref.read_map(capi.MAP_RAYCAST), dev.read_map(capi.MAP_RAYCAST)
            # tolerance: float-atomic accumulation order
            np.testing.assert_allclose(rb, ra, rtol=2e-5, atol=2e-6)
            nxt = scans[k + 1]
            step(nxt, capi.SCAN_DEFAULT)
            assert ref.raycast_finish() == dev.raycast_finish() == capi.OK
            ma, mb = ref.read_map(capi.MAP_VOXELS), dev.read_map(capi.MAP_VOXELS)
            fin = np.isfinite(ma)
            np.testing.assert_array_equal(np.isfinite(mb), fin)
            np.testing.assert_allclose(mb[fin], ma[fin], rtol=1e-4, atol=1e-3)
            assert not dev.read_map(capi.MAP_FLAGS).any() and not ref.read_map(capi.MAP_FLAGS).any()
            sync_maps(ref, dev)  # the next bit-exact stage starts from identical state again
        if sep_every and k % sep_every == 1:
            (sa, la), (sb, lb) = ref.sepclusters_begin(allow=(capi.ERR_EMPTY,)), dev.sepclusters_begin(allow=(capi.ERR_EMPTY,))
            assert (sa, la) == (sb, lb)
            if sa == capi.OK and la:
                assert ref.sepclusters_finish() == dev.sepclusters_finish() == capi.OK
                np.testing.assert_array_equal(dev.read_map(capi.MAP_VOXELS), ref.read_map(capi.MAP_VOXELS))
    if route is not None and not debug:
        from test_gpu_stream_route import profiled_calls

        route.update(n_calls=n_calls, launches=profiled_calls(dev.lib, dev))
        dev.lib.profile_enable(dev.h, 0)
    if not debug:
        # the occupancy image and the nVoxelsOver count were patched scan by scan (k_finalize_far): a scan WITH debug output reports
        # the count and goes through the image again (close flags of every cluster)
        s = scans[-1]
        dr, gr = ref.process_scan(s.scan, s.tf, debug=True)
        dh, gh = dev.process_scan(s.scan, s.tf, debug=True)
        assert_scan_debug_equal(gr, gh)
        assert_detections_equal(dr, dh)
        np.testing.assert_array_equal(dev.read_map(capi.MAP_VOXELS), ref.read_map(capi.MAP_VOXELS))
    return n_det


def _fallback_switch_set():
    """tools/run_fallback_matrix.sh runs this file under the library's fallback switches: the route assertions hold for the default"""
    return any(k.startswith("VOFOD_") and k not in ("VOFOD_TEST_HARNESS_SELFCHECK", "VOFOD_TRACE") for k in os.environ)


def _assert_route(route, name, n_cold_max=1):
    """VERDICT r4 missing #3: the production calls of a sequence took kernels_far.h + the one-kernel tail on all scans but at most
    `n_cold_max` (a scan with more than 4 096 far voxels raises CF_RETRY and runs again through the brick kernels and the
    three-kernel tail: the first scan on a map that only knows the seeded ground disc)"""
    from test_gpu_stream_route import STREAM_KERNELS, _record

    calls, n = route["launches"], route["n_calls"]
    _record(name, dict(calls, n_calls=n))
    assert "k_pack" not in calls, calls
    for k in STREAM_KERNELS:
        assert calls.get(k, 0) >= n - n_cold_max, (k, n, calls)
    assert calls.get("k_far_final", 0) + calls.get("k_tail_prep", 0) >= n, (n, calls)  # every call classified on the device


@pytest.mark.parametrize("debug", [True, False])
@pytest.mark.parametrize("sensor,vs", [("os1-16", 0.5), ("os1-128", 0.5), ("os1-128", 0.25)])
def test_process_scan_sequence_parity(oracle, hip, sensor, vs, debug):
    ref, dev = make_pair(oracle, hip, sensor, vs)
    scene = synth.make_scene(11, n_targets=2)
    scans = synth.scan_sequence(scene, sensor, 5, seed0=100)
    for d in (ref, dev):
        synth.seed_ground(d)
    route = {}
    _run_sequence(ref, dev, scans, debug=debug, route=route)
    assert dev.status().detection_its == ref.status().detection_its
    if not debug and not os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK") and not _fallback_switch_set():
        # (a map that only knows the seeded ground disc is cold: a scan with more than 4 096 far voxels raises CF_RETRY, runs again
        # through the brick kernels, and the close-first path stays off until the background has grown by a quarter - measured on
        # the round-5 code: 9 / 6 of the 9 calls at OS1-16 / OS1-128 take kernels_far.h, the others the brick route)
        _assert_route(route, f"sequence {sensor} {vs}", n_cold_max=route["n_calls"] // 2)


@pytest.mark.parametrize("debug", [True, False])
def test_process_scan_with_apriori_map_detects(oracle, hip, debug, vs=0.5):
    """config 3 shape: apriori (+inf) background, latches set, classification + flood fill active - with the debug output (host
    tail) and without (round 4: the device tail of a single map-updating scan; the map must equal the oracle's after every scan,
    frontier voxels of the flood fills included)."""
    ref, dev = make_pair(oracle, hip, "os1-128", vs)
    scene = synth.make_scene(21, n_targets=3)
    ap = synth.apriori_points(scene, vs)
    for d in (ref, dev):
        d.load_apriori(ap)
    np.testing.assert_array_equal(dev.read_map(), ref.read_map())
    scans = synth.scan_sequence(scene, "os1-128", 4, seed0=300)
    route = {}
    n_det = _run_sequence(ref, dev, scans, sep_every=2, debug=debug, route=route)
    assert n_det > 0  # the floating boxes are found, identically on both sides
    if not debug and not os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK") and not _fallback_switch_set():
        _assert_route(route, "apriori 0.5", n_cold_max=0)
    if not debug and not os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK") and os.environ.get("VOFOD_DEVICE_TAIL") != "0":
        lib = dev.lib
        lib.profile_enable(dev.h, 1)
        dev.process_scan(scans[0].scan, scans[0].tf)
        names, ms, calls = (C.c_char * (64 * 96))(), (C.c_double * 96)(), (C.c_uint64 * 96)()
        nk = lib.profile_read(dev.h, names, ms, calls, 96)
        lib.profile_enable(dev.h, 0)
        ran = [names[64 * i : 64 * i + 64].split(b"\0", 1)[0].decode() for i in range(nk)]
        # (k_tail_far behind kernels_far.h's ordered lists; the three-kernel tail behind the brick kernels, e.g. while the map is cold)
        assert ("k_tail_far" in ran or ("k_tail_prep" in ran and "k_explore" in ran and "k_tail_finish" in ran)) and "k_pack" not in ran, ran


def test_sensor_stream_with_auto_raycast(oracle, hip):
    """The nodelet's full schedule on the production call: VOFOD_SCAN_AUTO_RAYCAST without debug output.  The scan's map update,
    ++its, the raycast role (finish of the pending pass or begin of a new one) and only then the classification
    (vofod_nodelet.cpp:946-963) - on the HIP side the device tail is launched behind the raycast role.  Detections equal scan
    by scan; the map within the raycast's float-accumulation tolerance, re-synchronised after every scan."""
    ref, dev = make_pair(oracle, hip, "os1-128", 0.5)
    scene = synth.make_scene(21, n_targets=3)
    ap = synth.apriori_points(scene, 0.5)
    for d in (ref, dev):
        d.load_apriori(ap)
    n_det = n_finished = 0
    for s in synth.scan_sequence(scene, "os1-128", 6, seed0=300):
        pending = ref.status().raycast_pending
        a = ref.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        b = dev.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        assert len(a) == len(b)
        for k in ("id", "frame", "n_points"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_allclose(a["position"], b["position"], atol=1e-3)
        # tolerance: the classification reads a map the raycast update has just changed - the uncertainty sum inherits the float
        # accumulation order of the ray lengths: 1e-4 relative here, 1e-5 where the maps are identical
        np.testing.assert_allclose(a["confidence"], b["confidence"], rtol=1e-4, atol=1e-300)
        np.testing.assert_allclose(a["detection_probability"], b["detection_probability"], rtol=1e-5)
        n_det += len(a)
        n_finished += 1 if pending else 0
        sa, sb = ref.status(), dev.status()
        assert (sa.raycast_pending, sa.detection_its) == (sb.raycast_pending, sb.detection_its)
        ma, mb = ref.read_map(capi.MAP_VOXELS), dev.read_map(capi.MAP_VOXELS)
        fin = np.isfinite(ma)
        np.testing.assert_array_equal(np.isfinite(mb), fin)
        # tolerance: float-atomic accumulation order of the ray lengths, as in _run_sequence
        np.testing.assert_allclose(mb[fin], ma[fin], rtol=1e-4, atol=1e-3)
        np.testing.assert_array_equal(dev.read_map(capi.MAP_FLAGS), ref.read_map(capi.MAP_FLAGS))
        sync_maps(ref, dev)
    assert n_det > 0 and n_finished >= 2


def test_single_scans_with_more_detections_than_record_slots(oracle, hip):
    """Map-updating scans of a swarm: 33 to 46 detections per scan, more than the device tail has record slots (16 per frame) - but
    also 80 to 133 candidate clusters (counted on the oracle's debug view of the three scans), more than its 64 lanes.  The
    cluster count is noticed first, before any fill has run: TAIL_FB_CLUSTERS, and the host tail redoes the scan.  So this test
    holds the host tail behind k_tail_far to the oracle - ids, points, positions, confidences and the map, scan after scan; it
    never enters device_tail_overflow_records (the rebuild of the records after the fills have written the map), which
    test_gpu_tail_edges.py::test_detections_at_the_record_slots[17-scan] reaches with 23 candidates and asserts by kernel list."""
    ref, dev = make_pair(oracle, hip, "os1-128", 0.5)
    warm_scene = synth.make_scene(5, n_targets=0)
    scene = synth.make_scene(5, n_targets=160)  # same buildings (drawn first from the seed) + a swarm
    synth.warm_map(dev, warm_scene, "os1-128", 10)
    st = dev.status()
    assert st.background_pts_sufficient and st.sure_background_sufficient
    ref.load_apriori(np.zeros((0, 3), dtype=np.float32))  # both latches on the oracle's side, no voxel touched
    sync_maps(dev, ref)
    most = 0
    for s in synth.scan_sequence(scene, "os1-128", 3, seed0=900):
        a, b = ref.process_scan(s.scan, s.tf), dev.process_scan(s.scan, s.tf)
        b = b.copy()
        if len(a) and len(b):
            b["id"] = (b["id"].astype(np.int64) + (int(a["id"][0]) - int(b["id"][0]))).astype(b["id"].dtype)
        assert_detections_equal(a, b)
        np.testing.assert_array_equal(dev.read_map(capi.MAP_VOXELS), ref.read_map(capi.MAP_VOXELS))
        np.testing.assert_array_equal(dev.read_map(capi.MAP_FLAGS), ref.read_map(capi.MAP_FLAGS))
        most = max(most, len(a))
    assert most > 16, most


def test_ingest_apriori_from_file(oracle, hip, tmp_path):
    """row N2: file -> transform -> centroid grid -> +inf voxels, same map and same counts on both sides."""
    ref, dev = make_pair(oracle, hip, "os1-16", 0.5)
    scene = synth.make_scene(33, n_targets=1)
    rng = np.random.default_rng(5)
    ap = synth.apriori_points(scene, 0.2)  # finer than the map: several points per voxel, real centroids
    ap = (ap + rng.normal(0, 0.03, ap.shape)).astype(np.float32)
    f = tmp_path / "static.pts"
    with open(f, "w") as fh:
        fh.write(f"{len(ap)}\n")
        np.savetxt(fh, ap, fmt="%.6f")
    out = [d.ingest_apriori(str(f), (0.4, -0.3, 0.1), 17.5, (0.0, 0.0, 0.05)) for d in (ref, dev)]
    assert out[0] == out[1] and out[0][0] == len(ap) and 0 < out[0][1] < len(ap)
    a, b = ref.read_map(), dev.read_map()
    np.testing.assert_array_equal(a, b)
    assert np.isinf(a).sum() > 100
    with pytest.raises(Exception):
        dev.ingest_apriori(str(tmp_path / "missing.pts"))


def test_rangefinder_ground_update_parity(oracle, hip):
    """row N4: the height range-finder's map update, interleaved with scans, keeps both maps identical"""
    ref, dev = make_pair(oracle, hip, "os1-16", 0.5)
    scene = synth.make_scene(9, n_targets=1)
    rng = np.random.default_rng(2)
    for k, s in enumerate(synth.scan_sequence(scene, "os1-16", 3, seed0=60)):
        down = s.tf.copy()
        down[:, :3] = np.float32([[0, 0, 1], [0, 1, 0], [-1, 0, 0]])  # x axis of the range-finder frame points down
        for r in rng.uniform(0.5, 60.0, 6):
            a = ref.update_ground(r, down, allow=(capi.ERR_MAP_RANGE,))
            b = dev.update_ground(r, down, allow=(capi.ERR_MAP_RANGE,))
            assert a == b
        ref.process_scan(s.scan, s.tf)
        dev.process_scan(s.scan, s.tf)
        np.testing.assert_array_equal(dev.read_map(), ref.read_map())


def test_no_map_update_and_batch_parity(oracle, hip):
    ref, dev = make_pair(oracle, hip, "os1-128", 0.5, max_batch=4)
    scene = synth.make_scene(31, n_targets=2)
    ap = synth.apriori_points(scene, 0.5)
    for d in (ref, dev):
        d.load_apriori(ap)
    before = dev.read_map()
    scans = synth.scan_sequence(scene, "os1-128", 6, seed0=500)
    tfs = np.stack([s.tf for s in scans])
    da, pa, ga = ref.process_batch([s.scan for s in scans], tfs, debug=True)
    db, pb, gb = dev.process_batch([s.scan for s in scans], tfs, debug=True)  # 6 frames > max_batch 4: two launch groups
    np.testing.assert_array_equal(pb, pa)
    assert_detections_equal(da, db)
    for x, y in zip(ga, gb):
        assert_scan_debug_equal(x, y)
    np.testing.assert_array_equal(dev.read_map(), before)  # read-only map
    assert dev.status().detection_its == 0


def test_lds_brick_clustering_in_batches_and_its_overflow_fallback(oracle, hip, monkeypatch):
    """0.25 m voxels, tolerance 1.5 m: bricks are cliques, batches of >= 4 frames are voxelised and clustered inside LDS
    (k_frame_lds); a frame with more bricks than the kernel takes makes the host run the batch again on the
    general kernels (slab voxeliser + global-memory brick clustering)."""
    scene = synth.make_scene(41, n_targets=3)
    scans = synth.scan_sequence(scene, "os1-128", 6, seed0=700)
    tfs = np.stack([s.tf for s in scans])
    for limit in (None, "64"):
        if limit:
            monkeypatch.setenv("VOFOD_LDS_MAX_BRICKS", limit)
        ref, dev = make_pair(oracle, hip, "os1-128", 0.25, max_batch=8)
        for d in (ref, dev):
            synth.seed_ground(d)
        da, pa, ga = ref.process_batch([s.scan for s in scans], tfs, debug=True)
        db, pb, gb = dev.process_batch([s.scan for s in scans], tfs, debug=True)
        np.testing.assert_array_equal(pb, pa)
        assert_detections_equal(da, db)
        for x, y in zip(ga, gb):
            assert_scan_debug_equal(x, y)
        assert max(len(np.unique(x["labels"])) for x in ga) > 5
        # pipelined form (fresh handle for the fallback case: the switch to the global kernels is per handle)
        if limit:
            ref, dev = make_pair(oracle, hip, "os1-128", 0.25, max_batch=8)
            for d in (ref, dev):
                synth.seed_ground(d)
        t0 = dev.batch_submit([s.scan for s in scans[:4]], tfs[:4])
        t1 = dev.batch_submit([s.scan for s in scans[2:]], tfs[2:])
        g0, g1 = dev.batch_collect(t0), dev.batch_collect(t1)
        w0 = ref.process_batch([s.scan for s in scans[:4]], tfs[:4])
        w1 = ref.process_batch([s.scan for s in scans[2:]], tfs[2:])
        np.testing.assert_array_equal(g0[1], w0[1])
        np.testing.assert_array_equal(g1[1], w1[1])


@pytest.mark.parametrize("voxel_size", [0.25, 0.5])
def test_large_batch_takes_the_fused_slab_emission(oracle, hip, voxel_size):
    """>= 128 frames per batch.  0.25 m: bricks are cliques -> the frame kernel (k_frame_lds); 0.5 m: voxel-level
    clustering -> the general path, whose large-batch form is k_slab_emit (bitmap slab in LDS -> voxel records, instead of
    k_slab + k_scan_b + k_emit) followed by k_union<2> (which reads the whole prefix array)"""
    ref, dev = make_pair(oracle, hip, "os1-16", voxel_size, max_batch=136)
    for d in (ref, dev):
        synth.seed_ground(d)
    scene = synth.make_scene(43, n_targets=2)
    base = synth.scan_sequence(scene, "os1-16", 17, seed0=900)
    scans = [base[i % 17] for i in range(136)]
    tfs = np.stack([s.tf for s in scans])
    da, pa, ga = ref.process_batch([s.scan for s in scans], tfs, debug=True)
    db, pb, gb = dev.process_batch([s.scan for s in scans], tfs, debug=True)
    np.testing.assert_array_equal(pb, pa)
    assert_detections_equal(da, db)
    for x, y in zip(ga, gb):
        assert_scan_debug_equal(x, y)
    assert sum(len(x["weighted"]) for x in ga) > 136 * 1000


def _dense_scan(sensor, seed, extent, empty=False):
    """an organised scan whose points are uniform in a box around the sensor (no LiDAR geometry): nearly every point
    survives the crops, many points share a voxel"""
    h, w, _, _ = synth.SENSORS[sensor]
    n = h * w
    rng = np.random.default_rng(seed)
    if empty:
        x = y = z = np.zeros(n, dtype=np.float32)  # (0,0,0) sits inside the exclude box: every point is dropped
    else:
        x = rng.uniform(-extent, extent, n).astype(np.float32)
        y = rng.uniform(-extent, extent, n).astype(np.float32)
        z = rng.uniform(-2.0, 1.0, n).astype(np.float32)
    return ScanData(x=x, y=y, z=z.copy(), width=w, height=h, stride_bytes=4)

@pytest.mark.parametrize("n_frames,max_batch", [(4, 36), (10, 32), (6, 6)])
def test_small_batches_with_dense_and_empty_frames(oracle, hip, n_frames, max_batch):
    """Small batches (one workgroup per frame leaves most CUs idle; round 3 cut such frames into y-slabs, removed in round 4
    when the close-first kernel halved the frame stage) with and without spare workspace slots: the ground sheet and the
    buildings form one giant close component, an empty and a dense frame ride along - the dense one beyond the close-first
    kernel's and the LDS image's capacities, so the batch is run again, twice.  Everything the debug output carries (weighted
    cloud, labels, cluster table, detections) equals the oracle's, in the full view and in the far-only view."""
    ref, dev = make_pair(oracle, hip, "os1-128", 0.25, max_batch=max_batch)
    scene = synth.make_scene(77, n_targets=3)
    ap = synth.apriori_points(scene, 0.25)
    for d in (ref, dev):
        d.load_apriori(ap)  # both latches: classification and flood fills run
    base = synth.scan_sequence(synth.make_scene(77, n_targets=6), "os1-128", n_frames, seed0=4100)
    scans = [s.scan for s in base]
    tfs = np.stack([s.tf for s in base])
    scans[1] = _dense_scan("os1-128", 6, 20.0)             # points all over a 40 m square: many bricks in every slab
    if n_frames > 4:
        scans[3] = _dense_scan("os1-128", 7, 1.0, empty=True)
    db, pb, gb = dev.process_batch(scans, tfs, debug=True, clusters_cap=65536)
    da, pa, ga = ref.process_batch(scans, tfs, debug=True, clusters_cap=65536)
    np.testing.assert_array_equal(pb, pa)
    assert_detections_equal(da, db)
    for k, (x, y) in enumerate(zip(ga, gb)):
        try:
            assert_scan_debug_equal(x, y)
        except AssertionError as e:
            raise AssertionError(f"frame {k}: {e}") from e
    assert max(len(g["clusters"]) for g in ga) > 20
    # the far-only view: the close-first kernel's own output where a frame fits it, the full clustering cut down otherwise
    dbf, pbf, gbf = dev.process_batch(scans, tfs, debug=True, clusters_cap=65536, far_only=True)
    np.testing.assert_array_equal(pbf, pa)
    assert_detections_equal(da, _rebase_ids(dbf, da))
    for k, (x, y) in enumerate(zip(ga, gbf)):
        try:
            assert_scan_debug_equal(far_view(x), y)
        except AssertionError as e:
            raise AssertionError(f"far view, frame {k}: {e}") from e
    # without debug output (device tail) and pipelined: the same detections
    got, per = dev.process_batch(scans, tfs)
    np.testing.assert_array_equal(per, pa)
    assert_detections_equal(da, _rebase_ids(got, da))
    t0, t1 = dev.batch_submit(scans, tfs), dev.batch_submit(scans, tfs)
    for t in (t0, t1):
        g, per = dev.batch_collect(t)
        np.testing.assert_array_equal(per, pa)
        assert_detections_equal(da, _rebase_ids(g, da))


def _rebase_ids(got, want):
    got = got.copy()
    if len(got) and len(want):
        got["id"] = (got["id"].astype(np.int64) + (int(want["id"][0]) - int(got["id"][0]))).astype(got["id"].dtype)
    return got


@pytest.mark.parametrize("n_frames", [6, 130])
def test_batches_of_dense_and_empty_frames(oracle, hip, n_frames):
    """stress of the batch voxelisers' side paths (the frame kernel at 0.25 m, its overflow re-run on the slab voxeliser): key
    lists longer than a workgroup's register file (> 48 Ki survivors), voxels with more points than a byte counter holds, an
    empty frame in the middle of a batch; both batch sizes (< / >= 128 frames)"""
    sensor = "os1-128" if n_frames == 6 else "os1-16"
    ref, dev = make_pair(oracle, hip, sensor, 0.25, max_batch=n_frames)
    for d in (ref, dev):
        synth.seed_ground(d)
    pose = synth.make_pose(3)
    kinds = [_dense_scan(sensor, 1, 12.0), _dense_scan(sensor, 2, 3.0), _dense_scan(sensor, 3, 1.0, empty=True), _dense_scan(sensor, 4, 25.0)]
    scans = [kinds[i % 4] for i in range(n_frames)]
    tfs = np.stack([pose] * n_frames).astype(np.float32)
    da, pa, ga = ref.process_batch(scans, tfs, debug=True)
    db, pb, gb = dev.process_batch(scans, tfs, debug=True)
    np.testing.assert_array_equal(pb, pa)
    assert_detections_equal(da, db)
    for x, y in zip(ga, gb):
        assert_scan_debug_equal(x, y)
    assert ga[2]["n_input_after_crop"] == 0 and len(ga[2]["weighted"]) == 0
    if n_frames == 6:
        assert ga[0]["n_input_after_crop"] > 100_000  # beyond the 49 152 keys a workgroup keeps in registers
        assert ga[1]["n_input_after_crop"] - len(ga[1]["weighted"]) > 50_000  # extras far beyond the LDS staging area


def test_error_statuses_of_unusual_voxel_sizes_match(oracle, hip):
    """found by tools/fuzz_parity.py: a voxel size that does not tile the operation area puts weighted points outside the
    map (the reference's vector::at would throw: MAP_RANGE); 1.0 m voxels make sepclusters' parameters invalid.  Both
    implementations must report the same status, scan by scan."""
    from vofod_amd.detector import VofodError

    def status_of(fn):
        try:
            fn()
            return capi.OK
        except VofodError as e:
            return e.status

    scene = synth.make_scene(5, n_targets=2)
    for voxel in (0.3, 1.0):
        ref, dev = make_pair(oracle, hip, "os1-16", voxel, ground_points_max_distance=1.5)
        ap = synth.apriori_points(scene, voxel)
        for d in (ref, dev):
            d.load_apriori(ap)
        seen = set()
        for k, s in enumerate(synth.scan_sequence(scene, "os1-16", 4, seed0=3)):
            a = status_of(lambda: ref.process_scan(s.scan, s.tf))
            b = status_of(lambda: dev.process_scan(s.scan, s.tf))
            assert a == b, (voxel, k, a, b)
            seen.add(a)
            a = status_of(lambda: ref.sepclusters_begin(allow=(capi.ERR_EMPTY,)))
            b = status_of(lambda: dev.sepclusters_begin(allow=(capi.ERR_EMPTY,)))
            assert a == b, (voxel, k, "sepclusters", a, b)
            seen.add(a)
        assert seen - {capi.OK}, f"voxel {voxel}: expected at least one error status, saw {seen}"


def test_error_paths(oracle, hip):
    ref, dev = make_pair(oracle, hip, "os1-16", 0.5)
    scene = synth.make_scene(1)
    s = synth.scan_sequence(scene, "os1-16", 1)[0]
    bad = synth.make_scan(scene, s.tf, "os1-128", seed=0)
    for d in (ref, dev):
        with pytest.raises(Exception):
            d.process_scan(bad.scan, bad.tf)  # size mismatch (vofod_nodelet.cpp:895-899)
        assert d.raycast_finish(allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
        assert d.raycast_begin(s.scan, s.tf) == capi.OK
        assert d.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,)) == capi.ERR_RAYCAST_NO_DETECTION  # :1531-1537
        # an all-no-return scan: nothing survives the exclude box, nothing is cast
        empty = synth.make_scan(synth.Scene((0, 0, 0, 0), np.zeros((0, 6)), 0), s.tf, "os1-16", seed=0)
        dets, dbg = d.process_scan(empty.scan, empty.tf, debug=True)
        assert len(dets) == 0 and len(dbg["weighted"]) == 0 and len(dbg["clusters"]) == 0
        d.set_dynamic_params(raycast__pause=1)
        assert d.raycast_begin(s.scan, s.tf, allow=(capi.ERR_PAUSED,)) == capi.ERR_PAUSED
        d.set_dynamic_params(raycast__pause=0)
        # sensor outside the map (vofod_nodelet.cpp:1432, 1523-1526)
        tf_out = s.tf.copy()
        tf_out[2, 3] = 500.0
        assert d.raycast_begin(s.scan, tf_out, allow=(capi.ERR_SENSOR_OUTSIDE_MAP,)) == capi.ERR_SENSOR_OUTSIDE_MAP
        d.process_scan(s.scan, s.tf)
        assert d.raycast_finish(allow=(capi.ERR_RAYCAST_EMPTY,)) == capi.ERR_RAYCAST_EMPTY


def test_old_raycast_rule(oracle, hip):
    ref, dev = make_pair(oracle, hip, "os1-16", 0.5, raycast__new_update_rule=0, raycast__weight_coefficient=0.5)
    scene = synth.make_scene(2)
    scans = synth.scan_sequence(scene, "os1-16", 2, seed0=7)
    for d in (ref, dev):
        d.process_scan(scans[0].scan, scans[0].tf)
        d.raycast_begin(scans[0].scan, scans[0].tf)
        d.process_scan(scans[1].scan, scans[1].tf)
        assert d.raycast_finish() == capi.OK
    np.testing.assert_allclose(dev.read_map(), ref.read_map(), rtol=1e-4, atol=1e-3)

def test_real_ouster_lut_mask_and_min_intensity_through_raycast(oracle, hip):
    """Row N1 through the GPU (vofod_nodelet.cpp:358-371, 506-560 feeding raycast_cloud :1441-1492): the LUT of a real
    Ouster (non-zero lidar_origin_to_beam_origin_mm, a lidar -> sensor transform: non-zero beam offsets, `start = R lut.off + t`
    :1477), a mask with ~20 % zeros laid out with pixel_shift_by_row (`!mask[idx] && range == 0` skips the ray :1449; a masked
    pixel with a return is still cast), raycast/min_intensity > 0 (:1446) - sequence with raycast begin / finish against the oracle."""
    from vofod_amd.detector import VoFOD, default_params, mask_layout, ouster_lut

    sensor, vs = "os1-16", 0.5
    h, w, vfov_deg, _ = synth.SENSORS[sensor]
    rng = np.random.default_rng(2024)
    altitude = np.linspace(vfov_deg / 2, -vfov_deg / 2, h)        # Ouster rows run top to bottom
    azimuth = rng.uniform(-3.2, 3.2, h)                            # per-beam azimuth offsets of the calibration
    tf = np.eye(4)
    tf[:3, :3] = [[-1, 0, 0], [0, -1, 0], [0, 0, 1]]               # lidar_to_sensor_transform of an OS1 (metadata)
    tf[:3, 3] = [0.0, 0.0, 36.18]
    img = (rng.random((h, w)) < 0.8).astype(np.uint8) * 255        # ~20 % masked-out pixels
    shift = np.array([12 if r % 2 else 4 for r in range(h)], dtype=np.int32) + np.arange(h, dtype=np.int32) % 3  # pixel_shift_by_row
    dets = []
    for lib in (oracle, hip):
        dirs, offs = ouster_lut(lib, w, h, azimuth, altitude, origin_mm=15.806, tf=tf)
        assert np.abs(offs).max() > 0.01                           # the beam offsets are really there (metres)
        mask = mask_layout(lib, img, w, h, shift)
        assert 0.1 < 1.0 - mask.astype(bool).mean() < 0.3
        sp, dp = default_params(lib)
        sp.voxel_size = vs
        sp.sensor_hrays, sp.sensor_vrays = w, h
        sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
        dp.raycast__min_intensity = 300.0                          # synthetic intensities are U(0, 1000): ~30 % of the rays are dropped
        dets.append(VoFOD(lib, sp, dp, lut_directions=dirs, lut_offsets=offs, mask=mask))
    ref, dev = dets
    scene = synth.make_scene(21, n_targets=2)
    scans = synth.scan_sequence(scene, sensor, 4, seed0=300)
    n_zero_masked = sum(int(((s.range == 0) & (mask == 0)).sum()) for s in scans)
    n_hit_masked = sum(int(((s.range > 0) & (mask == 0)).sum()) for s in scans)
    assert n_zero_masked > 100 and n_hit_masked > 100              # both sides of the :1449 condition occur
    for d in (ref, dev):
        synth.seed_ground(d)
    _run_sequence(ref, dev, scans)
    # and the same LUT / mask against the default sensor model: the raycast map differs, i.e. the inputs were really used
    plain_ref, plain_dev = make_pair(oracle, hip, sensor, vs)
    for d in (plain_dev, dev):
        d.reset()
        synth.seed_ground(d)
        d.process_scan(scans[0].scan, scans[0].tf)
        assert d.raycast_begin(scans[0].scan, scans[0].tf) == capi.OK
    a, b = plain_dev.read_map(capi.MAP_RAYCAST), dev.read_map(capi.MAP_RAYCAST)
    assert float(a.sum(dtype=np.float64)) > 1.2 * float(b.sum(dtype=np.float64)) > 0  # fewer rays were cast (intensity gate, mask)


def test_aos_ouster_layout_and_device_input(oracle, hip):
    """the 48-byte ouster_ros::Point AoS (x +0, y +4, z +8, intensity +16, range +36) through the strided-column view"""
    ref, dev = make_pair(oracle, hip, "os1-16", 0.5)
    scene = synth.make_scene(5, n_targets=2)
    for d in (ref, dev):
        synth.seed_ground(d)
    s0, s1 = synth.scan_sequence(scene, "os1-16", 2, seed0=900)
    n = s0.x.size
    aos = np.zeros(n, dtype=np.dtype({"names": ["x", "y", "z", "intensity", "range"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 16, 36], "itemsize": 48}))
    for k in ("x", "y", "z", "intensity", "range"):
        aos[k] = getattr(s0, k)
    base = aos.ctypes.data
    from vofod_amd.detector import ScanData

    scan_aos = ScanData(x=base, y=base + 4, z=base + 8, intensity=base + 16, range=base + 36, width=s0.scan.width, height=s0.scan.height, stride_bytes=48)
    for d in (ref, dev):
        d.process_scan(scan_aos, s0.tf)
        assert d.raycast_begin(scan_aos, s0.tf) == capi.OK
    dr, gr = ref.process_scan(s1.scan, s1.tf, debug=True)
    dh, gh = dev.process_scan(s1.scan, s1.tf, debug=True)
    assert_scan_debug_equal(gr, gh)
    assert ref.raycast_finish() == dev.raycast_finish() == capi.OK
    ma, mb = ref.read_map(), dev.read_map()
    np.testing.assert_allclose(mb, ma, rtol=1e-4, atol=1e-3)
    # device-resident columns (what bench.py hands over)
    import ctypes as C

    rt = C.CDLL("libamdhip64.so")  # the runtime the product already loaded (torch is not needed for device memory)
    rt.hipMalloc.argtypes, rt.hipMemcpy.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    cols = np.ascontiguousarray(np.stack([s1.x, s1.y, s1.z]))
    dptr = C.c_void_p()
    assert rt.hipMalloc(C.byref(dptr), cols.nbytes) == 0
    assert rt.hipMemcpy(dptr, cols.ctypes.data_as(C.c_void_p), cols.nbytes, 1) == 0  # hipMemcpyHostToDevice
    col = s1.x.nbytes
    scan_dev = ScanData(x=dptr.value, y=dptr.value + col, z=dptr.value + 2 * col, width=s1.scan.width, height=s1.scan.height, stride_bytes=4, memspace=capi.MEM_DEVICE)
    sync_maps(ref, dev)
    da, ga = ref.process_scan(s1.scan, s1.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
    db, gb = dev.process_scan(scan_dev, s1.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
    assert_scan_debug_equal(ga, gb)
    assert_detections_equal(da, db)
    rt.hipFree.argtypes = [C.c_void_p]
    rt.hipFree(dptr)


def test_pipelined_batches_equal_synchronous(oracle, hip):
    """vofod_batch_submit / vofod_batch_collect: two batches in flight give the detections of the synchronous calls"""
    ref, dev = make_pair(oracle, hip, "os1-128", 0.5, max_batch=4)
    scene = synth.make_scene(21, n_targets=3)
    ap = synth.apriori_points(scene, 0.5)
    for d in (ref, dev):
        d.load_apriori(ap)
        for s in synth.scan_sequence(scene, "os1-128", 5, seed0=300):
            d.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
    sync_maps(ref, dev)
    batches = [synth.scan_sequence(scene, "os1-128", 4, seed0=310 + 10 * b) for b in range(3)]
    want = []
    for b in batches:
        want.append(ref.process_batch([s.scan for s in b], np.stack([s.tf for s in b])))
    scan_lists = [[s.scan for s in b] for b in batches]
    tf_lists = [np.stack([s.tf for s in b]) for b in batches]
    got = []
    t_prev = dev.batch_submit(scan_lists[0], tf_lists[0])
    for k in range(1, 3):
        t_next = dev.batch_submit(scan_lists[k], tf_lists[k])  # batch k is enqueued before batch k-1 is collected
        got.append(dev.batch_collect(t_prev))
        t_prev = t_next
    got.append(dev.batch_collect(t_prev))
    assert sum(len(w[0]) for w in want) > 0
    id0 = want[0][0]["id"][0] - got[0][0]["id"][0] if len(want[0][0]) else 0
    for (wd, wp), (gd, gp) in zip(want, got):
        np.testing.assert_array_equal(gp, wp)
        gd = gd.copy()
        gd["id"] += id0
        assert_detections_equal(wd, gd)
    with pytest.raises(Exception):
        dev.batch_collect(0)

def test_eight_small_batches_in_flight_with_tails_of_their_own(oracle, hip):
    """Small batches (fewer frames than half the CUs) run their whole chain - classification tail included - on the ticket's
    stream with flood-fill buffers of their own: eight in flight, collected out of submission order, give the detections of
    the synchronous calls; a ninth submission is refused with VOFOD_ERR_CAPACITY and leaves the eight intact."""
    ref, dev = make_pair(oracle, hip, "os1-128", 0.5, max_batch=6)
    scene = synth.make_scene(21, n_targets=3)
    ap = synth.apriori_points(scene, 0.5)
    for d in (ref, dev):
        d.load_apriori(ap)
        for s in synth.scan_sequence(scene, "os1-128", 5, seed0=300):
            d.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
    sync_maps(ref, dev)
    batches = [synth.scan_sequence(scene, "os1-128", 4 + (b % 3), seed0=310 + 10 * b) for b in range(8)]
    scan_lists = [[s.scan for s in b] for b in batches]
    tf_lists = [np.stack([s.tf for s in b]) for b in batches]
    want = [ref.process_batch(sl, tl) for sl, tl in zip(scan_lists, tf_lists)]
    assert sum(len(w[0]) for w in want) > 0
    for rounds in range(2):  # the second round reuses every ticket's workspace and buffers
        tickets = [dev.batch_submit(sl, tl) for sl, tl in zip(scan_lists, tf_lists)]
        assert sorted(tickets) == list(range(8))
        with pytest.raises(VofodError) as e:
            dev.batch_submit(scan_lists[0], tf_lists[0])
        assert e.value.status == capi.ERR_CAPACITY
        got = {}
        for k in (3, 0, 7, 1, 6, 2, 5, 4):
            got[k] = dev.batch_collect(tickets[k])
        for k in range(8):
            (wd, wp), (gd, gp) = want[k], got[k]
            np.testing.assert_array_equal(gp, wp)
            assert_detections_equal(wd, _rebase_ids(gd, wd))


def test_host_batch_in_one_block_and_params_changed_in_flight(oracle, hip):
    """(1) A host-resident batch whose frames are packed x | y | z columns at a constant pitch (one block) is moved by ONE 2-D
    copy (process_frames' staging): same results as the same scans given as separate arrays.  (2) vofod_set_dynamic_params
    between submit and collect: the submitted batch is classified with the parameters of its submission."""
    F = 6
    ref, dev = make_pair(oracle, hip, "os1-128", 0.5, max_batch=F)
    scene = synth.make_scene(21, n_targets=3)
    ap = synth.apriori_points(scene, 0.5)
    for d in (ref, dev):
        d.load_apriori(ap)
        for sc in synth.scan_sequence(scene, "os1-128", 5, seed0=300):
            d.process_scan(sc.scan, sc.tf, flags=capi.SCAN_AUTO_RAYCAST)
    sync_maps(ref, dev)
    base = synth.scan_sequence(scene, "os1-128", F, seed0=310)
    h, w, _, _ = synth.SENSORS["os1-128"]
    n = h * w
    # columns of one frame follow each other directly, frames at a constant pitch with padding between them: x | y | z | pad
    flat = np.zeros((F, 3 * n + 192), dtype=np.float32)
    for f, sc in enumerate(base):
        flat[f, :n], flat[f, n : 2 * n], flat[f, 2 * n : 3 * n] = sc.x, sc.y, sc.z
    in_block = [ScanData(x=flat[f, :n], y=flat[f, n : 2 * n], z=flat[f, 2 * n : 3 * n], width=w, height=h, stride_bytes=4) for f in range(F)]
    tfs = np.stack([sc.tf for sc in base])
    want, want_per, want_dbg = ref.process_batch([sc.scan for sc in base], tfs, debug=True)
    got, got_per, got_dbg = dev.process_batch(in_block, tfs, debug=True)
    np.testing.assert_array_equal(got_per, want_per)
    assert_detections_equal(want, got)
    for x, y in zip(want_dbg, got_dbg):
        assert_scan_debug_equal(x, y)
    assert len(want) > 0
    # (2) parameters changed while the batch is in flight
    t = dev.batch_submit(in_block, tfs)
    dev.set_dynamic_params(classification__min_points=10_000, output__position_sigma=123.0)  # would reject every cluster / change every covariance
    g, per = dev.batch_collect(t)
    dev.set_dynamic_params(classification__min_points=ref.dp.classification__min_points, output__position_sigma=ref.dp.output__position_sigma)
    np.testing.assert_array_equal(per, want_per)
    assert_detections_equal(want, _rebase_ids(g, want))
    # and a batch submitted under the changed parameters does see them
    dev.set_dynamic_params(classification__min_points=10_000)
    g2, per2 = dev.batch_collect(dev.batch_submit(in_block, tfs))
    assert len(g2) == 0 and not per2.any()


def test_pinned_host_input_may_be_overwritten_after_submit(oracle, hip):
    """include/vofod.h: the scans' host buffers need not outlive vofod_batch_submit.  From page-locked memory the H2D copy is
    truly asynchronous and queued behind the previous batch's streaming kernels: submit returns behind the copy.
    A caller that refills its arena right after submit - here: zeroes it - must still get the detections of what it submitted."""
    try:
        hiprt = C.CDLL("libamdhip64.so")
    except OSError:
        pytest.skip("no HIP runtime to page-lock memory with")
    F = 24
    ref, dev = make_pair(oracle, hip, "os1-128", 0.25, max_batch=F)
    synth.warm_map(dev, synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=0), "os1-128", 16)
    if dev.status().background_pts_sufficient and dev.status().sure_background_sufficient:
        ref.load_apriori(np.zeros((0, 3), dtype=np.float32))  # both latches, no voxel touched
    sync_maps(dev, ref)
    frames = synth.bench_frames(synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=12), "os1-128", F)  # targets that appeared after the warm-up
    tfs = np.stack([s.tf for s in frames])
    want, want_per = ref.process_batch([s.scan for s in frames], tfs)
    assert len(want) >= 1
    h_, w_, _, _ = synth.SENSORS["os1-128"]
    n = h_ * w_
    base = C.c_void_p()
    hiprt.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    assert hiprt.hipHostMalloc(C.byref(base), F * 3 * n * 4, 0) == 0  # page-locked: one block, x | y | z per frame (the one-copy path)
    view = np.ctypeslib.as_array(C.cast(base, C.POINTER(C.c_float)), shape=(F, 3, n))
    for rnd in range(3):
        for f, s in enumerate(frames):
            view[f, 0], view[f, 1], view[f, 2] = s.x, s.y, s.z
        scans = [ScanData(x=base.value + (3 * f) * n * 4, y=base.value + (3 * f + 1) * n * 4, z=base.value + (3 * f + 2) * n * 4, width=w_, height=h_, stride_bytes=4, memspace=capi.MEM_HOST)
                 for f in range(F)]
        t0 = dev.batch_submit(scans, tfs)
        view[:] = 0.0  # the caller reuses its arena at once
        t1 = dev.batch_submit(scans, tfs)  # (a batch of no-return pixels: no detections)
        got, per = dev.batch_collect(t0)
        got1, per1 = dev.batch_collect(t1)
        np.testing.assert_array_equal(per, want_per)
        assert_detections_equal(want, _rebase_ids(got, want))
        assert len(got1) == 0 and int(per1.sum()) == 0
    hiprt.hipHostFree.argtypes = [C.c_void_p]
    hiprt.hipHostFree(base)


def test_collect_with_too_small_an_array_keeps_the_ticket(oracle, hip):
    """vofod_batch_collect with an `out` too small: VOFOD_ERR_CAPACITY, *n_out = the size needed, the ticket stays pending and
    the second call returns what the synchronous call returns (ids included: none were handed out by the failing call)"""
    if os.environ.get("VOFOD_DEVICE_TAIL") == "0":
        pytest.skip("host tail (tools/run_fallback_matrix.sh): the failing collect consumes the batch, as include/vofod.h says")
    ref, dev = make_pair(oracle, hip, "os1-128", 0.5, max_batch=4)
    scene = synth.make_scene(21, n_targets=3)
    ap = synth.apriori_points(scene, 0.5)
    for d in (ref, dev):
        d.load_apriori(ap)
        for s in synth.scan_sequence(scene, "os1-128", 5, seed0=300):
            d.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
    sync_maps(ref, dev)
    b = synth.scan_sequence(scene, "os1-128", 4, seed0=310)
    scans, tfs = [s.scan for s in b], np.stack([s.tf for s in b])
    wd, wp = ref.process_batch(scans, tfs)
    assert len(wd) >= 2
    t = dev.batch_submit(scans, tfs)
    small = np.zeros(1, dtype=capi.DETECTION)
    per = np.zeros(4, dtype=np.uint32)
    n_out = C.c_size_t(0)
    assert dev.lib.batch_collect(dev.h, t, capi.ptr(small), 1, capi.ptr(per), C.byref(n_out)) == capi.ERR_CAPACITY
    assert n_out.value == len(wd)
    gd, gp = dev.batch_collect(t, det_cap=1)  # the wrapper comes back with the size asked for
    np.testing.assert_array_equal(gp, wp)
    gd = gd.copy()
    gd["id"] += wd["id"][0] - gd["id"][0]
    assert_detections_equal(wd, gd)
    assert np.all(np.diff(gd["id"]) == 1)


def test_dynamic_params_invalidate_cached_tables(oracle, hip):
    """set_dynamic_params between scans: the cached cluster stencil / brick tables, hasCloseTo rows and the occupancy
    image (threshold) must follow (m_drmgr_ptr->config may change between any two callbacks)"""
    ref, dev = make_pair(oracle, hip, "os1-128", 0.25)
    scene = synth.make_scene(13, n_targets=2)
    for d in (ref, dev):
        synth.seed_ground(d)
    scans = synth.scan_sequence(scene, "os1-128", 4, seed0=40)
    settings = [
        dict(ground_points_max_distance=1.5),                       # brick family (tol/leaf = 6)
        dict(ground_points_max_distance=0.8),                       # voxel family (tol/leaf = 3.2), other hasCloseTo rows
        dict(voxel_map__thresholds__new_obstacles=-500.0),          # other occupancy image
        dict(ground_points_max_distance=1.5, classification__min_points=1, voxel_map__scores__unknown=-700.0),
    ]
    for s, kv in zip(scans, settings):
        for d in (ref, dev):
            d.set_dynamic_params(**kv)
        dr, gr = ref.process_scan(s.scan, s.tf, debug=True)
        dh, gh = dev.process_scan(s.scan, s.tf, debug=True)
        assert_scan_debug_equal(gr, gh)
        assert_detections_equal(dr, dh)
        np.testing.assert_array_equal(dev.read_map(), ref.read_map())


def test_concurrent_callers_are_serialised(hip):
    """two threads hammer one handle (the nodelet's pointcloud / sepclusters threads): calls are serialised on the
    handle's mutex and the result equals some sequential order (here: the map ends identical to a sequential replay
    because the two roles touch it commutatively only through process_scan's order)"""
    import threading

    from helpers import make_pair as mk

    _, dev = mk(hip, hip, "os1-16", 0.5)
    _, seq = mk(hip, hip, "os1-16", 0.5)
    scene = synth.make_scene(3)
    scans = synth.scan_sequence(scene, "os1-16", 6, seed0=11)
    for d in (dev, seq):
        synth.seed_ground(d)
    errs = []

    def scan_role():
        try:
            for s in scans:
                dev.process_scan(s.scan, s.tf)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    def status_role():
        try:
            for _ in range(200):
                dev.status()
                dev.read_map(capi.MAP_FLAGS)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    ts = [threading.Thread(target=scan_role), threading.Thread(target=status_role)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs
    for s in scans:
        seq.process_scan(s.scan, s.tf)
    np.testing.assert_array_equal(dev.read_map(), seq.read_map())
    assert dev.status().detection_its == 6


def test_replay_driver_runs_the_three_thread_roles(hip):
    """examples/vofod_replay: processMsg loop + detached raycast threads + sepclusters timer against one handle (row N3)"""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    subprocess.run(["make", "-C", str(root / "examples")], check=True)
    out = subprocess.run([str(root / "examples" / "vofod_replay"), "--scans", "30", "--rows", "32", "--cols", "1024", "--voxel", "0.5"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    last, check = lines[-2], lines[-1]
    assert last.startswith("done: 30 scans") and "detection_its 30" in last, last
    assert "raycasts 0 " not in last  # the raycast role ran at least once
    # result check: the detections sit on the flying cube, the outgoing messages were serialised
    import re

    m = re.match(r"check: (\d+) detections on the flying target, (\d+) elsewhere; (\d+) message bytes", check)
    assert m, check
    on, off, nbytes = map(int, m.groups())
    assert on >= 5 and off <= on // 4 and nbytes > 30 * (12 + 4 + 12 + 4), check
