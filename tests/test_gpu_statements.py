"""The HIP library against the numpy / scipy statements of tests/statements.py - written from the cited reference lines without
looking at either implementation, and until now only ever run on the oracle (tests/test_properties.py).  Every other GPU test
compares the product with the oracle, which shares its author and some host skeletons with it: a misreading of the reference
that went into both is invisible there.  Here nothing of the oracle takes part (only the empty-block regression at the end uses
it, in addition).

(a) the debug route: every shared statement on `hip`, fixed seeds in place of hypothesis;
(b) the production route of a sensor stream - a single map-updating scan WITHOUT debug output: kernels_far.h + k_tail_far;
(c) the production route of a read-only batch: k_frame_lds_far + k_tail_far;
(d) the rank of a neighbour window that starts in the last word of an all-empty bitmap block (kernels_far.h, k_far_edges).

Bit-exact statements stay bit-exact.  Statements with a tolerance of their own get the project's existing HIP-vs-oracle
tolerance of the quantity added to it (HIP_TOL); nothing was measured to choose them."""
import os

import numpy as np
import pytest

import statements as st
from helpers import assert_detections_equal, make_pair
from vofod_amd import capi, synth
from vofod_amd.detector import voxel_grid_weighted

pytestmark = pytest.mark.gpu

HIP_TOL = st.Tol(
    # raycast accumulator: the statement's rtol 2e-5 / atol 1e-3 + _run_sequence's 2e-5 / 2e-6 (float-atomic order)
    ray_rtol=2e-5, ray_atol=2e-6,
    # map behind a raycast update: the sweep statement's 2e-6 / 1e-6 + _run_sequence's / test_sensor_stream_with_auto_raycast's 1e-4 / 1e-3
    sweep_rtol=1e-4, sweep_atol=1e-3,
    # confidence (also covariance, detection probability): the statement's 2e-6 (1e-6, 1e-9) + assert_detections_equal's 1e-5
    conf_rtol=1e-5,
    # position against the OBB centre of a debug call: the statement's 0 + assert_scan_debug_equal's / assert_detections_equal's 1e-3 m
    pos_atol=1e-3,
)


def _selfcheck():
    return bool(os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"))  # `hip` is the oracle then: no kernels, no routes


def _route_checked():
    from test_gpu_parity import _fallback_switch_set

    return not _selfcheck() and not _fallback_switch_set()


def _profiled(det, call):
    """run `call()` under the library's profiler: (its result, {kernel: launches})"""
    from test_gpu_stream_route import profiled_calls

    det.lib.profile_enable(det.h, 1)
    try:
        out = call()
        ran = profiled_calls(det.lib, det)
    finally:
        det.lib.profile_enable(det.h, 0)
    return out, ran


@pytest.fixture(scope="module")
def grid_handle(hip):
    """the stateless entry points of the HIP library run on a handle's device and stream"""
    det, *_ = st.sensor_detector(hip, "os1-16", 0.5)
    yield det.h
    det.close()


# ------------------------------------------------------------------------------------------------------- (a) the debug route
# fixed draws of the CPU tests' strategies: leaves 0.1 / 0.25 / 0.5 / 1.0 (and 3.0), aligned and not, n = 1 and n in the thousands,
# seeds divisible by three (test_weighted_grid_against_numpy_unique: points ON cell boundaries)
@pytest.mark.parametrize("seed,n,leaf,aligned", [(0, 1, 0.25, False), (1, 3000, 0.1, True), (2, 1500, 0.5, False), (3, 2999, 1.0, True), (4, 2000, 3.0, False),
                                                 (10_000, 17, 3.0, True), (5, 2500, 0.1, False), (6, 1, 1.0, True)])
def test_weighted_grid_conserves_points_and_is_permutation_invariant(hip, grid_handle, seed, n, leaf, aligned):
    st.weighted_grid_conserves_points_and_is_permutation_invariant(hip, seed, n, leaf, aligned, handle=grid_handle)


@pytest.mark.parametrize("seed,n,thr", [(0, 1, -100.0), (1, 2000, -0.1), (2, 1234, 0.5), (3, 1, 0.5), (10_000, 1999, -100.0), (4, 777, -0.1)])
def test_counted_grid_total_is_the_true_total(hip, grid_handle, seed, n, thr):
    st.counted_grid_total_is_the_true_total(hip, seed, n, thr, handle=grid_handle)


@pytest.mark.parametrize("seed,n,tol", [(0, 2, 0.7), (1, 600, 1.5), (2, 333, 2.0), (3, 600, 0.7), (4, 100, 1.5), (5, 599, 2.0), (10_000, 450, 0.7)])
def test_cluster_labels_match_scipy_components(hip, grid_handle, seed, n, tol):
    st.cluster_labels_match_scipy_components(hip, seed, n, tol, handle=grid_handle)


@pytest.mark.parametrize("seed,n,leaf,aligned", [(0, 1, 0.1, True), (3, 4999, 0.1, False), (6, 3000, 0.25, True), (7, 2500, 0.25, False), (9, 4000, 0.5, False),
                                                 (10, 1, 0.5, True), (12, 5000, 1.0, True), (13, 777, 1.0, False), (99_999, 3511, 0.25, False), (100_000, 2, 0.1, True),
                                                 (30, 4321, 0.5, True), (33, 1, 0.25, False), (36, 2048, 1.0, False), (39, 5000, 0.1, True)])
def test_weighted_grid_against_numpy_unique(hip, grid_handle, seed, n, leaf, aligned):
    st.weighted_grid_against_numpy_unique(hip, seed, n, leaf, aligned, handle=grid_handle)


@pytest.mark.parametrize("sensor,vs,seed", [("os1-16", 0.5, 3), ("os1-16", 0.25, 4), ("os1-128", 0.5, 5)])
def test_far_clusters_are_the_untainted_components_of_the_far_voxels(hip, sensor, vs, seed):
    st.far_clusters_are_the_untainted_components_of_the_far_voxels(hip, sensor, vs, seed)


def test_whole_scan_raycast_map_is_segment_voxel_geometry(hip):
    """The one number of this file that is a measurement: the statement allows < 50 voxels beyond 1e-4 + 2e-5 |want| (the drift of the
    reference's running `tmax`).  Counted on the same input: oracle 4, HIP library 4 (MI355X; float-atomic order changes sums by
    ~1e-5 relative, it does not move length between voxels) - within a factor of two, so the cap of 50 stays."""
    st.whole_scan_raycast_map_is_segment_voxel_geometry(hip, HIP_TOL)


@pytest.mark.parametrize("new_rule", [1, 0])
def test_raycast_update_sweep_is_the_voxelwise_formula(hip, new_rule):
    st.raycast_update_sweep_is_the_voxelwise_formula(hip, new_rule, HIP_TOL)


@pytest.mark.parametrize("sensor,vs", [("os1-16", 0.5), ("os1-128", 0.25)])
def test_map_update_of_a_scan_is_the_voxelwise_formula(hip, sensor, vs):
    st.map_update_of_a_scan_is_the_voxelwise_formula(hip, sensor, vs)


@pytest.mark.parametrize("sensor,vs,seed", [("os1-16", 0.5, 300), ("os1-128", 0.25, 301)])
def test_filter_and_transform_of_a_scan_against_numpy_crops(hip, sensor, vs, seed):
    st.filter_and_transform_of_a_scan_against_numpy_crops(hip, sensor, vs, seed)


def test_detection_records_against_the_formulas_in_numpy(hip):
    st.detection_records_against_the_formulas_in_numpy(hip, HIP_TOL)


def test_classification_of_a_scan_against_scipy_fills_in_cluster_order(hip):
    st.classification_of_a_scan_against_scipy_fills_in_cluster_order(hip)


@pytest.mark.parametrize("sensor,vs", [("os1-16", 0.5), ("os1-128", 0.25)])
def test_close_far_split_and_clusters_of_a_scan_against_scipy(hip, sensor, vs):
    st.close_far_split_and_clusters_of_a_scan_against_scipy(hip, sensor, vs)


@pytest.mark.parametrize("seed,max_bg", [(1, 0.8), (2, 0.8), (3, 1.6), (4, 2.2), (5, 0.8)])
def test_sepclusters_role_against_numpy(hip, seed, max_bg):
    st.sepclusters_role_against_numpy(hip, seed, max_bg)


# ------------------------------------------------------------------------------------------ (b) the production stream route
def test_production_scan_without_debug_output_against_numpy(hip):
    """A single map-updating scan WITHOUT debug output - the call a sensor stream makes, on the HIP side kernels_far.h (k_far_edges /
    k_far_final / k_finalize_far) and the one-kernel tail k_tail_far instead of the full clustering and the host tail the debug
    statements see.  State: the classification statement's (apriori map, six VOFOD_SCAN_AUTO_RAYCAST scans, both latches set).  A
    read-only debug call fetches the scan's weighted cloud, labels and cluster table (themselves held to the clustering and
    close/far statements); the call under test must then leave the map the update formula and the scipy fills in cluster order
    give - frontier voxels included, bit for bit -, flags 2 / 3, and return the records of the clusters the numpy classification
    calls MAV."""
    sensor, vs = "os1-128", 0.5
    det, sp, dp, h, w, scans = st.apriori_stream_state(hip, sensor, vs, n_warm=6)
    assert not det.status().raycast_pending  # (begin / finish three times: the checked scans see no raycast role)
    off = np.array(det.map_offset, dtype=np.float32)
    sx, sy, sz = (int(x) for x in det.map_size)
    tol = np.float32(dp.ground_points_max_distance)
    thr = np.float32(dp.voxel_map__thresholds__new_obstacles)
    seen = {capi.CLASS_MAV: 0, capi.CLASS_UNKNOWN: 0, capi.CLASS_INVALID: 0}
    n_frontier = n_records = 0
    ran_all = {}
    for s in scans[6:]:
        m0 = det.read_map(capi.MAP_VOXELS).reshape(sz, sy, sx).copy()
        f0 = det.read_map(capi.MAP_FLAGS).reshape(sz, sy, sx).copy()
        # 1: the scan's cloud, labels and cluster table from a read-only debug call
        _, g = det.process_scan(s.scan, s.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
        np.testing.assert_array_equal(det.read_map(capi.MAP_VOXELS).reshape(sz, sy, sx).view(np.uint32), m0.view(np.uint32))  # read-only
        st_ = det.status()
        assert st_.background_pts_sufficient and st_.sure_background_sufficient
        pts, lab, cl = g["weighted"], g["labels"], g["clusters"]
        P = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float32)
        cell = st.map_cells(pts, off, vs)
        img = st.close_image(m0, thr, tol, vs)
        want_close, _ = st.assert_clusters_and_close_far(P, cell, tol, img, lab, cl)
        assert want_close.any() and (~want_close).any()
        st.assert_far_clusters_are_untainted_components(P, tol, img[cell[:, 2], cell[:, 1], cell[:, 0]], lab, cl)
        # 2: the call under test
        dets, ran = _profiled(det, lambda: det.process_scan(s.scan, s.tf))
        for k, v in ran.items():
            ran_all[k] = ran_all.get(k, 0) + v
        # 3: the same in numpy
        is_close = st.voxel_is_close(lab, cl)
        wgt, score = st.update_weights_and_scores(pts, is_close, dp)
        iz, iy, ix = cell[:, 2], cell[:, 1], cell[:, 0]
        m = m0.copy()
        m[iz, iy, ix] = wgt * m0[iz, iy, ix] + (np.float32(1.0) - wgt) * score  # updateVMaps :946-948
        tpos = np.asarray(s.tf, dtype=np.float32).reshape(3, 4)[:, 3]
        far_cl = cl[cl["is_close"] == 0]
        classes, nf = st.classify_far_clusters(m, far_cl, lab, cell, tpos, dp, vs)
        n_frontier += nf
        for c in classes:
            seen[c] += 1
        got = det.read_map(capi.MAP_VOXELS).reshape(sz, sy, sx)
        np.testing.assert_array_equal(got.view(np.uint32), m.view(np.uint32))
        want_f = f0.copy()
        want_f[iz, iy, ix] = np.where(is_close, np.float32(2.0), np.float32(3.0))  # m_vflags_point / m_vflags_unknown, :2335-2337
        np.testing.assert_array_equal(det.read_map(capi.MAP_FLAGS).reshape(sz, sy, sx), want_f)
        mav = [c for c, k in zip(far_cl, classes) if k == capi.CLASS_MAV]  # cluster order
        assert len(dets) == len(mav), (len(dets), len(mav), classes)
        m64 = got.astype(np.float64)
        for d, c in zip(dets, mav):
            st.assert_detection_record(d, c, pts[lab == c["first_member"]], m64, tpos, off, vs, sp, dp, h, w, HIP_TOL)
            n_records += 1
    assert seen[capi.CLASS_MAV] >= 2 and seen[capi.CLASS_UNKNOWN] >= 1 and n_frontier > 0 and n_records >= 2, (seen, n_frontier, n_records)
    # 4: the route (the fallback switches of tools/run_fallback_matrix.sh and the harness self-check take other ones)
    if _route_checked():
        for k in ("k_far_edges", "k_far_final", "k_finalize_far", "k_tail_far"):
            assert ran_all.get(k, 0) == 2, (k, ran_all)
        assert "k_pack" not in ran_all, ran_all  # the debug read-back never ran
    det.close()


# ------------------------------------------------------------------------------------------- (c) the production batch route
def test_production_batch_without_debug_output_against_scipy(hip):
    """A read-only batch of eight OS1-16 frames at 0.25 m on a map warmed without the targets: the close-first frame kernel
    k_frame_lds_far and k_tail_far.  Per frame, from the far-only debug view: the voxels that carry a label are exactly the
    untainted components of the far voxels (close bit: the dilated occupancy image of the map), the same member sets, sizes,
    smallest members and table order.  The detections of the production call and of a batch_submit / batch_collect pair are the
    numpy records of the clusters the scipy fills call MAV - the fills run on a per-frame copy of the unchanged map, the "per-scan
    overlay" of VOFOD_SCAN_NO_MAP_UPDATE (include/vofod.h) -, and the map is bit-identical afterwards."""
    sensor, vs, n = "os1-16", 0.25, 8
    det, sp, dp, h, w = st.sensor_detector(hip, sensor, vs, max_batch=n)
    warm_scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=0)
    scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=8)
    synth.warm_map(det, warm_scene, sensor, 8)
    # (eight scans do not collect sepclusters' sure background: both latches from an empty apriori cloud, no voxel touched - without
    # them nothing is explored and nothing is detected, :1694)
    m_warm = det.read_map(capi.MAP_VOXELS).copy()
    det.load_apriori(np.zeros((0, 3), dtype=np.float32))
    np.testing.assert_array_equal(det.read_map(capi.MAP_VOXELS).view(np.uint32), m_warm.view(np.uint32))
    # At 0.25 m the raycast role has not carved the unknown space after eight scans (every fill would run into its depth limit:
    # class UNKNOWN, no detection).  Stand-in for the passes that follow: every voxel that is not background becomes free air, three
    # in ten stay unknown (just below the site-percolation threshold of the 6-neighbourhood, 0.31: pockets of all sizes, some reach
    # the depth limit) - the fills then meet all their outcomes.  The background, and with it every close bit and the route, is untouched.
    rng = np.random.default_rng(8)
    free = m_warm <= np.float32(dp.voxel_map__thresholds__new_obstacles)
    m_warm[free] = np.where(rng.random(int(free.sum())) < 0.3,np.float32(dp.voxel_map__scores__unknown), np.float32(dp.voxel_map__scores__ray))
    det.write_map(capi.MAP_VOXELS, m_warm)
    del m_warm, free
    st_ = det.status()
    assert st_.background_pts_sufficient and st_.sure_background_sufficient and not st_.raycast_pending
    frames = synth.bench_frames(scene, sensor, n)
    scans, tfs = [s.scan for s in frames], np.stack([s.tf for s in frames])
    off = np.array(det.map_offset, dtype=np.float32)
    sx, sy, sz = (int(x) for x in det.map_size)
    tol = np.float32(dp.ground_points_max_distance)
    thr = np.float32(dp.voxel_map__thresholds__new_obstacles)
    m0 = det.read_map(capi.MAP_VOXELS).reshape(sz, sy, sx).copy()
    f0 = det.read_map(capi.MAP_FLAGS).copy()
    img = st.close_image(m0, thr, tol, vs)

    d_dbg, per_dbg, gs = det.process_batch(scans, tfs, debug=True, far_only=True)
    want = []  # per frame: (cluster record, members, overlay map, sensor position) of every MAV cluster, in cluster order
    n_far = []
    seen = {capi.CLASS_MAV: 0, capi.CLASS_UNKNOWN: 0, capi.CLASS_INVALID: 0}
    n_frontier = 0
    for f, g in enumerate(gs):
        pts, lab, cl = g["weighted"], g["labels"], g["clusters"]
        assert (cl["is_close"] == 0).all()  # the far-only view lists the far clusters only
        P = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float32)
        cell = st.map_cells(pts, off, vs)
        close = img[cell[:, 2], cell[:, 1], cell[:, 0]]
        assert close.any() and (~close).any()
        n_far.append(st.assert_far_clusters_are_untainted_components(P, tol, close, lab, cl))
        mf = m0.copy()  # the per-scan overlay
        tpos = np.asarray(tfs[f], dtype=np.float32).reshape(3, 4)[:, 3]
        classes, nf = st.classify_far_clusters(mf, cl, lab, cell, tpos, dp, vs)
        n_frontier += nf
        for k in classes:
            seen[k] += 1
        m64 = mf.astype(np.float64)
        want.append([(c, pts[lab == c["first_member"]], m64, tpos) for c, k in zip(cl, classes) if k == capi.CLASS_MAV])
    assert max(n_far) >= 2 and seen[capi.CLASS_MAV] >= 2 and seen[capi.CLASS_UNKNOWN] >= 1 and n_frontier > 0, (n_far, seen, n_frontier)

    def check(dets, per):
        np.testing.assert_array_equal(per, [len(x) for x in want])
        k = 0
        for f, recs in enumerate(want):
            for c, mem, m64, tpos in recs:
                assert int(dets[k]["frame"]) == f
                st.assert_detection_record(dets[k], c, mem, m64, tpos, off, vs, sp, dp, h, w, HIP_TOL)
                k += 1
        assert k == len(dets)

    check(d_dbg, per_dbg)
    (dets, per), ran = _profiled(det, lambda: det.process_batch(scans, tfs))  # no debug output: the production call
    check(dets, per)
    tickets = [det.batch_submit(scans, tfs) for _ in range(2)]
    for t in tickets:
        check(*det.batch_collect(t))
    np.testing.assert_array_equal(det.read_map(capi.MAP_VOXELS).reshape(sz, sy, sx).view(np.uint32), m0.view(np.uint32))
    np.testing.assert_array_equal(det.read_map(capi.MAP_FLAGS), f0)
    if _route_checked():
        assert "k_frame_lds_far" in ran and "k_tail_far" in ran and "k_frame_lds_full" not in ran, ran
    det.close()


# ------------------------------------------------------------------- (d) regression: the empty-block rank of k_far_edges
def test_far_edge_window_that_starts_in_the_last_word_of_an_empty_bitmap_block(oracle, hip):
    """kernels_far.h, k_far_edges: the rank of a neighbour window's first set bit is wprefix[wi] + popcount(bits of word wi below the
    window).  At 0.25 m voxels / tolerance 1.5 m the brick family emits the cloud and leaves the prefix entries of all-empty 65 536-
    cell bitmap blocks unwritten (GridParams::sparse_prefix): a window that STARTS in the last word of such a block with all its
    bits in the next block must take that next word's own entry - wprefix[wi] is stale memory there.

    Hand-placed returns on a lattice of 300 x 300 cells per layer (two anchor returns fix it): a two-voxel far cluster {v, n} with n
    straight above v (stencil row dj = 0, dk = 1, a forward row), n in cell 1 of a bitmap block, the whole block before it empty.
    With classification__min_points = 2 the detection exists only if that one edge is found.  A denser scan of the same lattice
    runs first and leaves a voxel in that block, so the stale entry holds its count, not n's rank.  The geometry is asserted in
    host arithmetic on the lattice vofod_voxel_grid_weighted reports for the same points before the library sees the scan.  (No
    run with the fix reverted: a wrong rank indexes the voxel array out of range.)"""
    from test_gpu_close_first import _cells_scan
    from test_gpu_stream_route import profiled_calls

    vs, tol_m = 0.25, 1.5
    ref, dev = make_pair(oracle, hip, "os1-16", vs, classification__min_points=2, ground_points_max_distance=tol_m)
    ox, oy, oz = dev.map_offset
    sx, sy, sz = dev.map_size
    # background sheet in map layer 8 (apriori: both latches), free air everywhere else: nothing for the flood fills to explore
    ix, iy = np.meshgrid(np.arange(20, sx - 20), np.arange(20, sy - 20), indexing="ij")
    sheet = np.stack([ox + (ix.ravel() + 0.5) * vs, oy + (iy.ravel() + 0.5) * vs, np.full(ix.size, oz + 8.5 * vs)], axis=1).astype(np.float32)
    for d in (ref, dev):
        d.load_apriori(sheet)
        m = d.read_map(capi.MAP_VOXELS).copy()
        assert np.isinf(m).sum() == ix.size
        m[np.isfinite(m)] = np.float32(d.dp.voxel_map__scores__ray)
        d.write_map(capi.MAP_VOXELS, m)
    a0 = np.array([40, 40, 30])  # map cell of lattice cell (0, 0, 0): 22 layers above the sheet, everything here is far
    DX = DY = 300
    anchors = [(0, 0, 0), (DX - 1, DY - 1, 1)]
    v_ijk, n_ijk = (273, 136, 0), (273, 136, 1)  # (1 * 300 + 136) * 300 + 273 = 2 * 65 536 + 1
    sparse = anchors[:1] + [v_ijk, n_ijk] + anchors[1:]
    dense = anchors + [(i, j, 0) for i in range(20, 40) for j in range(20, 35)] + [(251, 136, 1)]  # the last one: block 1, its last word
    t = np.float32([55.0, 14.0, 9.0])
    tf = np.float32([[1, 0, 0, t[0]], [0, 1, 0, t[1]], [0, 0, 1, t[2]]])

    def world(ijk):
        c = np.asarray(ijk) + a0
        return np.stack([ox + (c[:, 0] + 0.5) * vs, oy + (c[:, 1] + 0.5) * vs, oz + (c[:, 2] + 0.5) * vs], axis=1)

    def lattice(ijk):
        """the scan's weighted cloud and lattice as the stand-alone grid reports them, for the points the library will see"""
        s = _cells_scan(world(ijk), t)
        k = len(ijk)
        q = [c[:k] + tt for c, tt in zip((s.x, s.y, s.z), t)]  # identity rotation: x + t in float
        align = np.array(dev.map_offset, dtype=np.float32) + np.float32(vs) / np.float32(2)  # idxToCoord(0, 0, 0), :664
        out, keys, grid, _ = voxel_grid_weighted(hip, q[0], q[1], q[2], vs, align, handle=dev.h)
        return s, out, keys.astype(np.int64), grid

    def rank_of(out, ijk):
        p = world([ijk])[0]
        hit = np.flatnonzero((np.abs(out["x"] - p[0]) < 0.01) & (np.abs(out["y"] - p[1]) < 0.01) & (np.abs(out["z"] - p[2]) < 0.01))
        assert len(hit) == 1
        return int(hit[0])

    s_sparse, out, L, grid = lattice(sparse)
    s_dense, out_d, L_d, grid_d = lattice(dense)
    dx, dy, dz = (int(x) for x in grid.div_b)
    assert (dx, dy, dz) == (DX, DY, 2) and list(grid_d.div_b) == [dx, dy, dz] and list(grid_d.min_b) == list(grid.min_b)
    assert len(L) == 4 and len(L_d) == len(dense)
    rv, rn = rank_of(out, v_ijk), rank_of(out, n_ijk)
    # the key of a voxel is its linear cell index i + j*dx + k*dx*dy = its bit in the occupancy bitmap: 64 cells per word, 1 024 words
    # (65 536 cells) per block of the emission
    ijk_of = lambda key: (int(key % dx), int(key // dx % dy), int(key // (dx * dy)))
    (i_v, j_v, k_v), (i_n, j_n, k_n) = ijk_of(L[rv]), ijk_of(L[rn])
    assert (i_n, j_n, k_n) == (i_v, j_v, k_v + 1)  # stencil row (dj, dk) = (0, 1): a forward row of v
    # r_max of that row: at least 5 (25 + 1 < 36 = (tol / leaf)^2 in exact arithmetic), at most the stencil's bound ceil(tol / leaf) + 1
    wi = None
    for r_max in range(5, int(np.ceil(tol_m / vs)) + 2):
        lo, hi = max(i_v - r_max, 0), min(i_v + r_max, dx - 1)
        L_lo = (k_n * dy + j_n) * dx + lo
        wi, blk = L_lo >> 6, L_lo >> 16
        assert wi % 1024 == 1023 and not ((L >> 16) == blk).any()  # 1: the window starts in the last word of a block without any voxel
        in_window = (L >= L_lo) & (L <= L_lo + (hi - lo))
        assert in_window.sum() == 1 and in_window[rn]              # 2: n is the only set bit of the window
        assert L[rn] >> 6 == wi + 1 and L[rn] >> 16 == blk + 1    # 3: ... in the first word of the next block
    # the denser scan occupies that block (its emission writes the block's prefix entries), and what it leaves in the last word's
    # entry - the number of its voxels in front of that word - is not n's rank
    assert ((L_d >> 16) == (wi >> 10)).any() and int((L_d < (wi << 6)).sum()) != rn

    a, b = ref.process_scan(s_dense, tf), dev.process_scan(s_dense, tf)
    assert_detections_equal(a, b)
    dev.lib.profile_enable(dev.h, 1)
    a, b = ref.process_scan(s_sparse, tf), dev.process_scan(s_sparse, tf)  # the production call under test
    ran = profiled_calls(dev.lib, dev)
    dev.lib.profile_enable(dev.h, 0)
    assert len(a) == 1 and int(a["n_points"][0]) == 2  # the oracle finds {v, n}
    assert_detections_equal(a, b)
    np.testing.assert_array_equal(dev.read_map(capi.MAP_VOXELS), ref.read_map(capi.MAP_VOXELS))
    np.testing.assert_array_equal(dev.read_map(capi.MAP_FLAGS), ref.read_map(capi.MAP_FLAGS))
    if _route_checked():
        assert ran.get("k_far_edges", 0) == 1 and ran.get("k_tail_far", 0) == 1, ran
    # the membership, independently: scipy's components of the cloud a read-only debug call reports (the stand-alone grid's, bit for bit)
    _, g = dev.process_scan(s_sparse, tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
    np.testing.assert_array_equal(g["weighted"].view(np.uint32), out.view(np.uint32))
    P = np.stack([out["x"], out["y"], out["z"]], axis=1).astype(np.float32)
    comp, first, _, _ = st.euclidean_components(P, np.float32(tol_m))
    assert set(np.flatnonzero(comp == comp[rv]).tolist()) == {rv, rn} and comp.max() + 1 == 3
    np.testing.assert_array_equal(g["labels"], first[comp])
    far = g["clusters"][g["clusters"]["is_close"] == 0]
    assert len(far) == 3 and int(far["first_member"][0]) == rv and int(far["n_points"][0]) == 2
    ref.close()
    dev.close()
