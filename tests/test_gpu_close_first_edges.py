"""The close-first capacities and the retry latch at their edges.  Both production routes cluster close first and each has a hard
capacity with a retry behind it:
  single scan      k_closefar / k_closefar_sweep / k_far_edges / k_far_final / k_finalize_far (kernels_far.h) take at most FAR_MAX far voxels;
                   with one more k_far_final raises CF_RETRY_STATUS, k_finalize_far leaves the map alone and the scan runs again through
                   the full clustering;
  read-only batch  k_frame_lds_far (kernels_frame.h) takes at most CF_MAX pure-far bricks per frame; with one more in any frame the
                   whole batch runs again as k_frame_lds_full;
  latch            either retry sets cf_off / cf_off_bg (check_close_first_overflow, frames_collect.h): every call goes straight to the
                   full clustering until n_bg_voxels > cf_off_bg + cf_off_bg / 4 + 1000 or n_bg_voxels < cf_off_bg (launch_frames), or
                   vofod_reset.
The scenes (tests/close_first_edges.py) sit exactly at FAR_MAX - 1 / FAR_MAX / FAR_MAX + 1 far voxels and CF_MAX - 1 / CF_MAX / CF_MAX + 1
pure-far bricks; tests/test_close_first_edges_cpu.py proves that without the product library.

Every result is compared with the oracle's: detection records through assert_detections_equal (ids, frames and point counts exactly),
voxel map and flags bit for bit, the status counters exactly.  Both sides make the same calls, so their id counters stay in step.  Only
what lies behind a raycast pass takes the project's tolerance for float-atomic ray sums (test_gpu_stream_route.compare_cycle).  Routes are
asserted through vofod_profile_read under the default switches only: with a switch of frame_geometry.FALLBACK_SWITCHES or
VOFOD_LDS_MAX_BRICKS set, a call may take other kernels, the results hold all the same."""
import os

import numpy as np
import pytest

import close_first_edges as ce
import detection_points_cases as dpc
import frame_geometry as fg
import tail_edges as te
from helpers import assert_detections_equal, assert_scan_debug_equal, far_view, make_pair
from test_gpu_tail_edges import Bench, _profiled
from vofod_amd import capi

pytestmark = pytest.mark.gpu

VS = ce.VS
CAP = ce.capacities()
FAR_MAX, CF_MAX = CAP["FAR_MAX"], CAP["CF_MAX"]
FAR_KERNELS = ("k_far_edges", "k_far_final", "k_finalize_far")
FULL_CLUSTERING = ("k_brick", "k_union", "k_flatten")  # the general clustering kernels of a single scan (launch_cluster)


def _selfcheck():
    return bool(os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"))  # `hip` is the oracle: the tests' own logic, on any machine


def _route_checked():
    return not _selfcheck() and not any(k in os.environ for k in fg.FALLBACK_SWITCHES + ("VOFOD_LDS_MAX_BRICKS",))


def _full_clustering_ran(ran):
    return any(k.startswith(FULL_CLUSTERING) for k in ran)


@pytest.fixture
def bench(oracle, hip):
    """a fresh pair for every test: no latch, no ids, no raycast pass left over"""
    b = Bench(oracle, hip)
    yield b
    b.close()


def _state(d):
    s = d.status()
    return dict(detection_its=s.detection_its, last_detection_id=s.last_detection_id, raycast_pending=s.raycast_pending)


def _assert_same_state(bench, maps=True):
    assert _state(bench.dev) == _state(bench.ref)
    if maps:
        np.testing.assert_array_equal(bench.dev.read_map(capi.MAP_VOXELS).view(np.uint32), bench.ref.read_map(capi.MAP_VOXELS).view(np.uint32))
        np.testing.assert_array_equal(bench.dev.read_map(capi.MAP_FLAGS), bench.ref.read_map(capi.MAP_FLAGS))


def _small_scan(bench, k=1):
    return ce.cells_scan(bench.world(np.vstack([s.cells for s in ce.small_frame(k)])), bench.t)


# ------------------------------------------------------------------------------------------------------ a. single scan at the edge
@pytest.mark.parametrize("filler", ["block", "singles"])
@pytest.mark.parametrize("dk", [-1, 0, 1])
def test_single_scan_at_the_edge(bench, dk, filler):
    """S(FAR_MAX + dk, filler) as the first production scan of a fresh handle: all PT = FAR_MAX / 1024 slots per thread of k_far_final live,
    a chain of 204 far voxels tainted from its lowest member, and with `singles` 3 880 components whose records are written behind the five
    candidates' (table[ncc + atomicAdd(&s_C, 1)]).  FAR_MAX + 1: CF_RETRY, the full clustering behind it, the latch set - the next, small
    scan does not take kernels_far.h; after FAR_MAX it does."""
    checked = _route_checked()
    ref, dev = bench.ref, bench.dev
    scene = ce.single_scan(FAR_MAX + dk, filler)
    bench.load(scene)
    s = bench.scans[0]
    a = ref.process_scan(s, bench.tf)
    b, ran = _profiled(dev, lambda: dev.process_scan(s, bench.tf))
    print(f"\n[close-first edges] S({FAR_MAX + dk}, {filler}): {len(b)} detections, route {sorted(ran)}")
    assert_detections_equal(a, b)
    assert len(a) == scene.claims["detections"]
    _assert_same_state(bench)
    if checked:
        assert ran.get("k_far_final", 0) == 1, ran
        if dk <= 0:
            assert all(ran.get(k, 0) == 1 for k in FAR_KERNELS + ("k_tail_far",)) and not _full_clustering_ran(ran) and "k_tail_prep" not in ran, ran
        else:
            assert _full_clustering_ran(ran) and ran.get("k_tail_prep", 0) == 1, ran
    small = _small_scan(bench)
    a2 = ref.process_scan(small, bench.tf)
    b2, ran2 = _profiled(dev, lambda: dev.process_scan(small, bench.tf))
    assert_detections_equal(a2, b2)
    assert len(a2) >= 1
    _assert_same_state(bench)
    if checked:
        if dk <= 0:
            assert all(ran2.get(k, 0) == 1 for k in FAR_KERNELS) and not _full_clustering_ran(ran2), ran2
        else:
            assert not any(k in ran2 for k in FAR_KERNELS) and _full_clustering_ran(ran2), ran2  # latched


# ------------------------------------------------------------------------------------- b. a scan that runs twice moves state once
def _with_rays(scan, n_rays=512):
    """the scan with range and intensity columns: `n_rays` rays of the sensor's LUT above the intensity gate, 4 .. 13 m long"""
    n = scan.width * scan.height
    scan.intensity = np.full(n, -1.0, dtype=np.float32)  # below raycast__min_intensity = 0: not cast
    scan.range = np.zeros(n, dtype=np.uint32)
    idx = np.arange(0, n, n // n_rays)
    scan.intensity[idx] = 100.0
    scan.range[idx] = 4000 + 1500 * (idx % 7).astype(np.uint32)
    return scan


def _assert_behind_a_raycast(bench, exact=False):
    """state, flags and voxel map of both sides, and the raycast map while a pass is pending - what test_gpu_stream_route.compare_cycle
    compares: the accumulator means something between begin and finish only (the reference clears it at the next begin, the library's
    sweep leaves it zeroed).  The exact pass's float view of its units is held to the twin handle instead."""
    ref, dev = bench.ref, bench.dev
    assert _state(dev) == _state(ref)
    np.testing.assert_array_equal(dev.read_map(capi.MAP_FLAGS), ref.read_map(capi.MAP_FLAGS))
    ma, mb = ref.read_map(capi.MAP_VOXELS), dev.read_map(capi.MAP_VOXELS)
    fin = np.isfinite(ma)
    np.testing.assert_array_equal(np.isfinite(mb), fin)
    # tolerance: float-atomic accumulation order of the ray lengths behind a raycast update (test_gpu_stream_route.compare_cycle)
    np.testing.assert_allclose(mb[fin], ma[fin], rtol=1e-4, atol=1e-3)
    ra, rb = ref.read_map(capi.MAP_RAYCAST), dev.read_map(capi.MAP_RAYCAST)
    if not exact and ref.status().raycast_pending:
        np.testing.assert_allclose(rb, ra, rtol=2e-5, atol=2e-6)  # tolerance: float atomics (compare_cycle)
    return ma, mb, ra


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("pending", [False, True])
def test_a_scan_that_runs_twice_moves_state_once(bench, oracle, hip, monkeypatch, pending, exact):
    """S(FAR_MAX + 1, block) with VOFOD_SCAN_AUTO_RAYCAST: raycast_ahead_of_tail reads the scan's status before it moves the raycast state,
    so the first, abandoned run begins / finishes no pass and counts no detection iteration.  Afterwards the raycast map, the pending
    state, detection_its, the voxel map and the next scan's ids are the oracle's.  With exact accumulation the sums are order independent:
    a second HIP handle that makes the same calls under VOFOD_CLOSE_FIRST=0 - the scan runs once - ends bit-identical (units, raycast map,
    voxel map)."""
    if exact and _selfcheck():
        pytest.skip("oracle against oracle: the oracle has no exact accumulation")
    checked = _route_checked()
    ref, dev = bench.ref, bench.dev
    scene = ce.single_scan(FAR_MAX + 1, "block")
    # a pocket of unknown voxels beside the sensor, 80 cells from every candidate: where a finished pass shows in the voxel map (free air
    # already holds scores/ray, the scans' own voxels are flagged and skipped)
    scene.unknown = pocket = te.block(9, 9, 9) + (352, 196, 18)
    bench.load(scene)
    big, small, nxt = _with_rays(bench.scans[0]), _with_rays(_small_scan(bench, 1), 256), _with_rays(_small_scan(bench, 2), 128)
    twin = None
    if exact:
        twin = make_pair(oracle, hip, "os1-16", VS, max_batch=4)
        twin[0].close()
        twin = twin[1]
        twin.load_apriori(bench.world(np.stack(np.nonzero(np.isinf(bench.base))[::-1], axis=1)).astype(np.float32))
        twin.set_dynamic_params(**{**bench.defaults, **scene.dyn})
        twin.write_map(capi.MAP_VOXELS, bench.map0)
        twin.write_map(capi.MAP_FLAGS, bench.flags0)
        assert dev.set_raycast_exact(True) == capi.OK and twin.set_raycast_exact(True) == capi.OK
    try:
        seq = ([small] if pending else []) + [big]
        n_before = 0
        for i, s in enumerate(seq):
            a = ref.process_scan(s, bench.tf, flags=capi.SCAN_AUTO_RAYCAST)
            b, ran = _profiled(dev, lambda: dev.process_scan(s, bench.tf, flags=capi.SCAN_AUTO_RAYCAST))
            assert_detections_equal(a, b)
            n_before += len(a)
            if twin is not None:
                monkeypatch.setenv("VOFOD_CLOSE_FIRST", "0")
                t = twin.process_scan(s, bench.tf, flags=capi.SCAN_AUTO_RAYCAST)
                monkeypatch.undo()
                assert_detections_equal(a, t)
        assert len(a) == scene.claims["detections"]
        if checked:
            assert ran.get("k_far_final", 0) == 1 and _full_clustering_ran(ran), ran  # the scan did run twice
            assert sum(v for k, v in ran.items() if k.startswith("k_raycast")) == (0 if pending else 1), ran
            assert sum(v for k, v in ran.items() if k.startswith("k_ray_sweep")) == (1 if pending else 0), ran
        assert bool(ref.status().raycast_pending) == (not pending)
        ma, mb, ra = _assert_behind_a_raycast(bench, exact)
        assert np.count_nonzero(ra) > 1000 if not pending else (ma[pocket[:, 2], pocket[:, 1], pocket[:, 0]] != bench.map0[pocket[:, 2], pocket[:, 1], pocket[:, 0]]).sum() > 50
        if not pending:
            np.testing.assert_array_equal(mb.view(np.uint32), ma.view(np.uint32))  # no raycast update applied yet
        if twin is not None:
            np.testing.assert_array_equal(mb.view(np.uint32), twin.read_map(capi.MAP_VOXELS).view(np.uint32))
            np.testing.assert_array_equal(dev.read_map(capi.MAP_RAYCAST).view(np.uint32), twin.read_map(capi.MAP_RAYCAST).view(np.uint32))
            if not pending:
                (u, su), (v, sv) = dev.raycast_units(), twin.raycast_units()
                assert su == sv and u.any()
                np.testing.assert_array_equal(u, v)
            else:
                assert dev.raycast_units(allow=(capi.ERR_NOT_PENDING,)) == (None, capi.ERR_NOT_PENDING)
        # the next scan: its first detection id, and the pass it finishes / begins
        a = ref.process_scan(nxt, bench.tf, flags=capi.SCAN_AUTO_RAYCAST)
        b = dev.process_scan(nxt, bench.tf, flags=capi.SCAN_AUTO_RAYCAST)
        assert len(a) >= 1 and int(a["id"][0]) == n_before
        assert_detections_equal(a, b)
        _assert_behind_a_raycast(bench, exact)
    finally:
        if twin is not None:
            twin.close()


# ---------------------------------------------------------------------------------------------------------- c. batches at the edge
def _production_batch(bench, scans, tfs):
    """the production call on both sides, compared; returns the kernels the HIP side launched"""
    da, pa = bench.ref.process_batch(scans, tfs)
    (db, pb), ran = _profiled(bench.dev, lambda: bench.dev.process_batch(scans, tfs))
    np.testing.assert_array_equal(pb, pa)
    assert_detections_equal(da, db)
    return ran, da, pa


def _assert_frame_kernel(ran, far, full):
    assert ("k_frame_lds_far" in ran) == far and ("k_frame_lds_full" in ran) == full, ran


@pytest.mark.parametrize("dp_,edge_frame,fallback", [(d, f, "") for f in (0, 3) for d in (-1, 0, 1)] + [(0, 0, "VOFOD_LEAN_EMIT=0"), (0, 3, "VOFOD_LEAN_EMIT=0")])
def test_batches_at_the_edge(bench, monkeypatch, dp_, edge_frame, fallback):
    """B(CF_MAX + dp_) in frame 0 or in frame 3 of a four-frame batch on a fresh handle: pos < CF_MAX against s_npf > CF_MAX, the 10-bit list
    index of an open pair up to 1023 (every filler voxel has a neighbour at exactly the tolerance), a candidate across two bricks, a
    pure-far component with an edge to a close brick.  The production call first (CF_MAX + 1: k_frame_lds_far, then k_frame_lds_full),
    then the far-only debug view, then two submitted batches - latched by then after CF_MAX + 1, the results the oracle's all the same."""
    checked = _route_checked()
    if fallback:
        k, v = fallback.split("=")
        monkeypatch.setenv(k, v)
    ref, dev = bench.ref, bench.dev
    scene = ce.batch(CF_MAX + dp_, edge_frame)
    bench.load(scene)
    scans, tfs = bench.scans, bench.tfs
    ran, da, pa = _production_batch(bench, scans, tfs)
    print(f"\n[close-first edges] B({CF_MAX + dp_}) in frame {edge_frame} {fallback}: {pa.tolist()} detections, route {sorted(ran)}")
    np.testing.assert_array_equal(pa, scene.claims["detections"])
    if checked:
        _assert_frame_kernel(ran, far=True, full=dp_ > 0)
    da, pa, ga = ref.process_batch(scans, tfs, debug=True)
    db, pb, gb = dev.process_batch(scans, tfs, debug=True, far_only=True)
    np.testing.assert_array_equal(pb, pa)
    assert_detections_equal(da, db)
    for f, (x, y) in enumerate(zip(ga, gb)):
        try:
            assert_scan_debug_equal(far_view(x), y)
        except AssertionError as e:
            raise AssertionError(f"frame {f}: {e}") from e
    tickets = [dev.batch_submit(scans, tfs) for _ in range(2)]
    for tk in tickets:
        dr, pr = ref.process_batch(scans, tfs)
        dd, pd = dev.batch_collect(tk)
        np.testing.assert_array_equal(pd, pr)
        assert_detections_equal(dr, dd)
    _assert_same_state(bench)
    np.testing.assert_array_equal(dev.read_map(capi.MAP_VOXELS).view(np.uint32), bench.map0.view(np.uint32))  # read-only


# -------------------------------------------------------------------------------------------------------------------- d. the latch
def test_the_latch_sets_and_releases_at_its_bounds(bench):
    """B(CF_MAX + 1) sets the latch at b0 = n_bg_voxels.  With background voxels written into a far corner of the map, B(CF_MAX - 1) runs as
    k_frame_lds_full at b0 + b0 / 4 + 1000 background voxels and as k_frame_lds_far at one more; from a latched state one background voxel
    less than b0 releases it, and so does vofod_reset.

    Regression: launch_frames tested the release bound against the count of the map image it had just queued for rebuilding - the
    previous map's - so that after vofod_write_map the latch was released one call late (B(CF_MAX - 1) at b0 + b0 / 4 + 1001 still ran
    k_frame_lds_full).  The count is fetched before the test now."""
    checked = _route_checked()
    ref, dev = bench.ref, bench.dev
    over, under = ce.batch(CF_MAX + 1), ce.batch(CF_MAX - 1)
    bench.load(over)
    over_scans, tfs = bench.scans, bench.tfs
    under_scans = [ce.cells_scan(bench.world(np.vstack([s.cells for s in f])), bench.t) for f in under.frames]
    dp = dev.dp
    bg = np.float32(dp.voxel_map__scores__point)
    assert bg > np.float32(dp.voxel_map__thresholds__new_obstacles)

    def write(m):
        for d in (ref, dev):
            d.write_map(capi.MAP_VOXELS, m)

    def latch():
        write(bench.map0)
        ran, _, _ = _production_batch(bench, over_scans, tfs)
        if checked:
            _assert_frame_kernel(ran, far=True, full=True)

    def small(far):
        ran, da, pa = _production_batch(bench, under_scans, tfs)
        np.testing.assert_array_equal(pa, under.claims["detections"])
        if checked:
            _assert_frame_kernel(ran, far=far, full=not far)

    latch()
    _, _, gb = dev.process_batch(over_scans, tfs, debug=True, far_only=True)
    ref.process_batch(over_scans, tfs)  # (the ids stay in step)
    b0 = gb[0]["n_bg_voxels"]
    assert b0 == int((bench.map0 > np.float32(dp.voxel_map__thresholds__new_obstacles)).sum()) > 100_000
    small(far=False)  # latched
    n = b0 // 4 + 1000
    corner = ce.background_corner(n + 1, dev.map_size)
    m = bench.map0.copy()
    m[corner[:n, 2], corner[:n, 1], corner[:n, 0]] = bg
    write(m)
    small(far=False)  # b0 + b0 / 4 + 1000: not more than the bound
    m[corner[n, 2], corner[n, 1], corner[n, 0]] = bg
    write(m)
    small(far=True)  # one more: released
    small(far=True)
    # from a latched state: one background voxel less
    latch()
    m = bench.map0.copy()
    zz, yy, xx = np.nonzero(np.isinf(m))
    assert xx[0] < 40 and yy[0] < 40  # (a corner of the sheet, 100 cells from every voxel of the scene)
    m[zz[0], yy[0], xx[0]] = np.float32(dp.voxel_map__scores__ray)
    write(m)
    small(far=True)
    # from a latched state: vofod_reset, the apriori sheet and the maps again
    latch()
    for d in (ref, dev):
        d.reset()
        d.load_apriori(bench.world(np.stack([xx, yy, zz], axis=1)).astype(np.float32))
        d.write_map(capi.MAP_VOXELS, bench.map0)
        d.write_map(capi.MAP_FLAGS, bench.flags0)
    small(far=True)
    _assert_same_state(bench)


# ------------------------------------------------------------------------------------- e. retries at collect, tickets in flight
def test_retries_at_collect_with_tickets_in_flight(bench):
    """Three submits of B(CF_MAX + 1) on an unlatched handle: every one is launched close first and runs again - from the descriptors and
    the parameters its workspace kept (job_scans, job_dp) - when it is collected, in the order 2, 0, 1.  By then the caller has overwritten
    its host arrays with another scene's points (include/vofod.h: host buffers need not outlive the submit) and raised
    classification__min_points to 3, which would drop the pairs: every ticket still returns the detections of the submitted points under
    the submit-time parameters."""
    checked = _route_checked()
    ref, dev = bench.ref, bench.dev
    over, under = ce.batch(CF_MAX + 1), ce.batch(CF_MAX - 1, edge_frame=3)
    bench.load(over)
    tfs = bench.tfs
    mk = lambda scene: [ce.cells_scan(bench.world(np.vstack([s.cells for s in f])), bench.t) for f in scene.frames]
    other = mk(under)
    dev.reserve(3)
    want = [ref.process_batch(bench.scans, tfs) for _ in range(2)]
    d3, p3, g3 = ref.process_batch(bench.scans, tfs, debug=True)
    want.append((d3, p3))
    assert int(p3.sum()) == 6 and (d3["n_points"] == 2).sum() == 5  # five pairs: gone at min_points = 3
    dev.lib.profile_enable(dev.h, 1)
    tickets = []
    for i in range(3):
        scans = mk(over)
        tickets.append(dev.batch_submit(scans, tfs))
        for s, o in zip(scans, other):  # the submit has returned: the arrays are the caller's again
            s.x[:], s.y[:], s.z[:] = o.x, o.y, o.z
    for d in (ref, dev):
        d.set_dynamic_params(classification__min_points=3)
    from test_gpu_stream_route import profiled_calls

    for (da, pa), tk in zip(want, (2, 0, 1)):
        dd, pd = dev.batch_collect(tickets[tk])
        np.testing.assert_array_equal(pd, pa)
        assert_detections_equal(da, dd)
    ran = profiled_calls(dev.lib, dev)
    dev.lib.profile_enable(dev.h, 0)
    if checked:
        assert ran.get("k_frame_lds_far", 0) == 3 and ran.get("k_frame_lds_full", 0) == 3, ran
    if not _selfcheck():
        ext, pts, idx = dev.detection_points(tickets[1])
        dpc.assert_points(ext, pts, idx, dd, [dpc.expected_frame(g) for g in g3])
    # the latch is set: a batch below the capacity takes the full kernel
    da, pa = ref.process_batch(other, tfs)
    dev.lib.profile_enable(dev.h, 1)
    dd, pd = dev.batch_collect(dev.batch_submit(other, tfs))
    ran = profiled_calls(dev.lib, dev)
    dev.lib.profile_enable(dev.h, 0)
    np.testing.assert_array_equal(pd, pa)
    assert_detections_equal(da, dd)
    assert int(pa.sum()) == 1  # (the L triple: the pairs are below min_points now)
    if checked:
        _assert_frame_kernel(ran, far=False, full=True)
    _assert_same_state(bench)


# ------------------------------------------------------------------------------------ f. single-scan capacity meets the tail's
def test_single_scan_capacity_meets_the_tails(bench):
    """S(FAR_MAX, singles) at classification__min_points = 1: n_far stays at its cap while every single is a candidate - 3 880 candidate
    clusters and 3 892 members, beyond TAIL_MAXC and TAIL_MAXM: the unordered branch of k_far_final (records and members past the staged
    ones) and the tail's fallback flags together; the host tail redoes the scan from the full tables."""
    checked = _route_checked()
    ref, dev = bench.ref, bench.dev
    scene = ce.single_scan(FAR_MAX, "singles", min_points=1)
    assert scene.claims["cand_clusters"] > CAP["TAIL_MAXC"] and scene.claims["cand_members"] > CAP["TAIL_MAXM"]
    bench.load(scene)
    s = bench.scans[0]
    a = ref.process_scan(s, bench.tf, det_cap=8192)
    b, ran = _profiled(dev, lambda: dev.process_scan(s, bench.tf, det_cap=8192))
    print(f"\n[close-first edges] S({FAR_MAX}, singles) at min_points 1: {len(b)} detections, route {sorted(ran)}")
    assert len(a) > 1000
    assert_detections_equal(a, b)
    _assert_same_state(bench)
    if checked:
        assert all(ran.get(k, 0) == 1 for k in FAR_KERNELS + ("k_tail_far", "k_pack")) and not _full_clustering_ran(ran), ran


# ------------------------------------------------------------------- g. the frame kernel's second retry: the open-pair list
def test_open_pair_list_beyond_a_tiny_workspace(oracle, hip):
    """k_frame_lds_far raises CF_RETRY_STATUS a second way: more open pairs than its scratch list holds, five words per voxel slot of the
    workspace (s_no > hcap).  The workspace is sized by the sensor, a public create parameter: a 20-ray sensor gives 20 voxel slots, a list
    of 100.  Frame 0 holds 20 voxels in four columns of five stacked bricks, the columns two bricks apart along x and y, one voxel per
    brick at the brick's corner nearest the middle: the voxels of a column lie 4 cells apart (one component after the pass over adjacent
    bricks), a voxel and the voxel of the neighbour column's brick at the same height 5 cells (an edge), at the height above or below
    sqrt(41) cells (none).  For the octant matrices all of these are open (5 .. 7 cells along one axis): 4 x (5 + 2 x 4) = 52 pairs, listed
    from both ends: 104 > 100.  The batch runs again as k_frame_lds_full; the 20 voxels are one far cluster, the oracle's."""
    from vofod_amd.detector import VoFOD, default_params

    W, H = 10, 2
    dets = []
    for lib in (oracle, hip):
        sp, dp = default_params(lib)
        sp.voxel_size = VS
        sp.oparea_offset[:] = (4.0, 4.0, 0.0)
        sp.oparea_size[:] = (8.0, 8.0, 8.0)
        sp.sensor_hrays, sp.sensor_vrays = W, H
        sp.max_batch_frames = 4
        dp.classification__max_size = 6.0  # (the cluster of frame 0 is 4 m tall)
        dets.append(VoFOD(lib, sp, dp))
    ref, dev = dets
    try:
        assert dev.map_size == (33, 33, 33) and tuple(dev.map_offset) == (0.0, 0.0, 0.0)
        assert (fg.ref_lattice((4.0, 4.0, 0.0), (8.0, 8.0, 8.0), VS)["off"] == 0).all()  # bricks of the lattice = bricks of map cells
        ix, iy = np.meshgrid(np.arange(2, 31), np.arange(2, 31), indexing="ij")
        sheet = np.stack([(ix.ravel() + 0.5) * VS, (iy.ravel() + 0.5) * VS, np.full(ix.size, 2.5 * VS)], axis=1).astype(np.float32)
        for d in (ref, dev):
            d.load_apriori(sheet)  # background in map layer 2: everything from layer 9 up is far
        m = ref.read_map(capi.MAP_VOXELS).copy()
        m[np.isfinite(m)] = np.float32(dev.dp.voxel_map__scores__ray)  # free air everywhere else: a far cluster is floating
        for d in (ref, dev):
            d.write_map(capi.MAP_VOXELS, m)
        slabs = [(x, y, z) for x in (11, 16) for y in (11, 16) for z in (12, 16, 20, 24, 28)]  # bricks x 2 | 4, y 2 | 4, z 3 .. 7
        assert len({(x // 4, y // 4, z // 4) for x, y, z in slabs}) == W * H
        t = (1.0, 1.0, 7.5)
        frames = [slabs] + [[(12 + 2 * f, 10, 22), (13 + 2 * f, 10, 22), (22, 20 + f, 12), (22, 21 + f, 12)] for f in (1, 2, 3)]
        scans = [ce.cells_scan([((a + 0.5) * VS, (b + 0.5) * VS, (c + 0.5) * VS) for a, b, c in cells], t, w=W, h=H) for cells in frames]
        tfs = np.stack([np.float32([[1, 0, 0, t[0]], [0, 1, 0, t[1]], [0, 0, 1, t[2]]])] * 4)
        da, pa, ga = ref.process_batch(scans, tfs, debug=True)
        assert len(ga[0]["weighted"]) == W * H and len(ga[0]["clusters"]) == 1 and not ga[0]["clusters"]["is_close"].any()
        assert pa.tolist() == [1, 2, 2, 2]
        (db, pb), ran = _profiled(dev, lambda: dev.process_batch(scans, tfs))
        np.testing.assert_array_equal(pb, pa)
        db["id"] += np.uint32(len(da))  # (the oracle's debug call came first)
        da["id"] += np.uint32(len(da))
        assert_detections_equal(da, db)
        if _route_checked():
            _assert_frame_kernel(ran, far=True, full=True)
    finally:
        ref.close()
        dev.close()
