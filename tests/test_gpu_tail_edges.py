"""The classification tail at its capacities and gate boundaries: the device tail (kernels_tail.h: k_tail_far, or k_tail_prep +
k_explore + k_tail_finish) and, on the gate scenes, the host tail (frames_collect.h) - the three callers of vt::classify_gates
(host_tail.h), the one statement of boxes, gates and explore job.  The scenes are placed by hand (tests/tail_edges.py) - the random scenes of the other files cross these limits by wide
margins or stay far below them, and none of them says which overflow branch a scan took.

The recipe is the one of test_far_edge_window_that_starts_in_the_last_word_of_an_empty_bitmap_block: OS1-16, 0.25 m voxels, an apriori
background sheet in map layer 8 (both latches), every other voxel free air (scores/ray), the returns of a scan are the centres of
chosen map cells (_cells_scan), 20 layers or more above the sheet and 11 cells or more apart (tolerance: 6 cells).  With no
unknown space around it a cluster that reaches its flood fill is floating: a detection.  Every scene stays far below FAR_MAX far
voxels and CF_MAX pure-far bricks: the clustering never falls back, only the tail can.

Every scene runs through three device routes and is compared with the oracle by the existing helpers, tolerances unchanged:
  batch   read-only batch of four frames, k_frame_lds_far + k_tail_far (process_batch, then batch_submit / batch_collect twice);
  full    the same under VOFOD_CLOSE_FIRST=0: k_frame_lds_full + k_tail_prep / k_explore / k_tail_finish;
  scan    single map-updating scans without debug output, k_far_final + k_tail_far; map and flags compared bit for bit afterwards.
The gate scenes (cases 5 and 6) run through a fourth, with the same comparisons and statements:
  host    the batch under VOFOD_DEVICE_TAIL=0: k_frame_lds_far, then k_pack (read-back of the full tables) and the host tail
          (prep_frame_tail, k_explore for the fills); no kernel of the device tail runs.  The capacity cases are not run on it:
          the host tail has none of the device's capacities.
Ids, frames, point counts and per-frame counts are compared exactly (both sides make the same calls: their id counters stay in step).

Statements of the scene itself, so that a misreading shared by product and oracle does not hide:
  honesty    from the oracle's debug view (cloud, labels, cluster table) numpy recounts the candidate clusters (far, n_points >=
             min_points, every lattice extent * leaf <= max_size * (1 + 1e-4) + 1e-3 * voxel_size) and their members: they equal the
             numbers the scene was built for, and the detections are those the placed geometry says (where it says: a 13-voxel line,
             exactly max_size long, and the run exactly on the radius boundary are held to the oracle only);
  symmetric  shapes (axis-aligned lines, squares, cubes, blocks, a plus, diagonal pairs and triples): the reported position is the
             float64 centroid of the placed cells within 16 * np.spacing(np.float32(largest |coordinate| of the scene)) - a few float32
             roundings of a mean and a shift; any orthonormal basis gives the centroid, a wrong one moves the centre by centimetres;
  skew       shapes (tetrahedron, L triple, random sub-blocks of 3 x 3 x 3): the position lies inside the cluster's AABB widened by
             1e-3 m, the margin of test_obb_gates_on_degenerate_lattice_clusters.

Routes are asserted from the profiler's kernel list under the default switches only (_fallback_switch_set; with
VOFOD_TEST_HARNESS_SELFCHECK=1 `hip` is the oracle: the scenes are then checked for what they claim, on any machine).  The kernels
relied on: k_frame_lds_far / k_frame_lds_full (frame kernel of a batch), k_far_final (single scan), k_tail_far, k_tail_prep, and the
kernels only the host tail launches behind a device tail: k_pack (read-back of the full tables) and, after it, k_explore (k_tail_far
runs its fills itself).  Every test prints one line: the counts its scene produced and the route observed."""
import os

import numpy as np
import pytest

import statements as st
import tail_edges as te
from helpers import assert_detections_equal, make_pair
from test_gpu_close_first import _cells_scan
from vofod_amd import capi

pytestmark = pytest.mark.gpu

VS = te.VS
ROUTES = ["batch", "full", "scan"]
GATE_ROUTES = ROUTES + ["host"]


def _selfcheck():
    return bool(os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"))


def _route_checked():
    from test_gpu_parity import _fallback_switch_set

    return not _selfcheck() and not _fallback_switch_set()


def _profiled(det, call):
    from test_gpu_stream_route import profiled_calls

    det.lib.profile_enable(det.h, 1)
    try:
        out = call()
        ran = profiled_calls(det.lib, det)
    finally:
        det.lib.profile_enable(det.h, 0)
    return out, ran


class Bench:
    """an oracle detector, a HIP detector and the base map of the recipe"""

    def __init__(self, oracle, hip):
        self.ref, self.dev = make_pair(oracle, hip, "os1-16", VS, max_batch=4)
        dev = self.dev
        self.off = np.array(dev.map_offset, dtype=np.float64)
        sx, sy, sz = dev.map_size
        ix, iy = np.meshgrid(np.arange(20, sx - 20), np.arange(20, sy - 20), indexing="ij")
        sheet = np.stack([self.off[0] + (ix.ravel() + 0.5) * VS, self.off[1] + (iy.ravel() + 0.5) * VS, np.full(ix.size, self.off[2] + (te.SHEET_LAYER + 0.5) * VS)], axis=1)
        self.defaults = {}
        for d in (self.ref, dev):
            d.load_apriori(sheet.astype(np.float32))
        m = self.ref.read_map(capi.MAP_VOXELS).copy()
        assert np.isinf(m).sum() == ix.size and np.isinf(m[te.SHEET_LAYER]).sum() == ix.size
        m[np.isfinite(m)] = np.float32(dev.dp.voxel_map__scores__ray)
        self.base = m
        self.flags0 = np.zeros_like(m)
        for k in ("classification__min_points", "classification__max_size", "classification__max_distance", "classification__max_explore_distance"):
            self.defaults[k] = getattr(dev.dp, k)
        self.t = self.off + te.SENSOR_CELL * VS
        assert (self.t == self.t.astype(np.float32)).all()
        self.tf = np.float32([[1, 0, 0, self.t[0]], [0, 1, 0, self.t[1]], [0, 0, 1, self.t[2]]])
        self.clean = True

    def world(self, cells):
        return self.off + (np.asarray(cells, dtype=np.float64) + 0.5) * VS

    def load(self, scene):
        m = self.base.copy()
        if len(scene.unknown):
            u = scene.unknown
            assert np.isfinite(m[u[:, 2], u[:, 1], u[:, 0]]).all()
            m[u[:, 2], u[:, 1], u[:, 0]] = np.float32(self.dev.dp.voxel_map__scores__unknown)
        self.map0 = m
        for d in (self.ref, self.dev):
            d.set_dynamic_params(**{**self.defaults, **scene.dyn})
        self.reset_maps()
        self.scans = [_cells_scan(self.world(np.vstack([s.cells for s in f])), self.t) for f in scene.frames]
        self.tfs = np.stack([self.tf] * len(scene.frames))
        coords = np.vstack([self.world(s.cells) for f in scene.frames for s in f])
        self.pos_tol = 16 * float(np.spacing(np.float32(np.abs(coords).max())))

    def reset_maps(self):
        for d in (self.ref, self.dev):
            d.write_map(capi.MAP_VOXELS, self.map0)
            d.write_map(capi.MAP_FLAGS, self.flags0)

    def close(self):
        self.ref.close()
        self.dev.close()


@pytest.fixture(scope="module")
def bench_holder(oracle, hip):
    """one detector pair for the file (a map of 19.5 M voxels on each side); a test that did not end cleanly leaves ids and maps of
    the two sides in an unknown state, the next test then gets a fresh pair"""
    holder = {"b": None}
    yield holder, oracle, hip
    if holder["b"] is not None:
        holder["b"].close()


@pytest.fixture
def bench(bench_holder):
    holder, oracle, hip = bench_holder
    b = holder["b"]
    if b is None or not b.clean:
        if b is not None:
            b.close()
        b = holder["b"] = Bench(oracle, hip)
    b.clean = False
    yield b


# ------------------------------------------------------------------------------------------------------ the scene's statements
def _frame_counts(bench, g, dp):
    """(candidate clusters, candidate members, canonical list of (n_points, first_member) of the candidates) of a debug view"""
    pts, lab, cl = g["weighted"], g["labels"], g["clusters"]
    cell = st.map_cells(pts, bench.off.astype(np.float32), VS)
    lim = dp.classification__max_size * (1 + 1e-4) + 1e-3 * VS
    cands = []
    for c in cl:
        if c["is_close"] or int(c["n_points"]) < dp.classification__min_points:
            continue
        mem = cell[lab == c["first_member"]]
        assert len(mem) == int(c["n_points"])
        if (((mem.max(0) - mem.min(0)) * np.float32(VS)) <= lim).all():
            cands.append((int(c["n_points"]), int(c["first_member"])))
    cands.sort(key=lambda x: (-x[0], x[1]))  # canonical order: size descending, smallest member ascending
    return len(cands), sum(n for n, _ in cands), cands


def _check_honesty(bench, scene, gs, dets, per):
    """the oracle's debug view of every frame against the numbers the scene was built for; returns the counts of frame 0"""
    dp = bench.ref.dp
    out = None
    for f, (g, shapes) in enumerate(zip(gs, scene.frames)):
        assert len(g["weighted"]) == sum(len(s.cells) for s in shapes) and len(g["clusters"]) == len(shapes), f  # nothing joined, nothing lost
        assert not g["clusters"]["is_close"].any(), f
        nc, nm, cands = _frame_counts(bench, g, dp)
        assert nc == sum(s.cand for s in shapes), (f, nc)
        assert nm == sum(len(s.cells) for s in shapes if s.cand), (f, nm)
        sure, open_ = sum(s.det is True for s in shapes), sum(s.det is None for s in shapes)
        assert sure <= int(per[f]) <= sure + open_, (f, int(per[f]), sure, open_)
        if f == 0:
            out = dict(candidates=nc, members=nm, detections=int(per[f]), cands=cands)
    assert int(np.sum(per)) == len(dets)
    return out


def _check_positions(bench, scene, dets, per, frames=None):
    """every detection lies in the widened AABB of exactly one placed cluster of its frame; the clusters found are those the
    geometry says; positions of symmetric shapes are centroids"""
    frames = range(len(scene.frames)) if frames is None else frames
    k = 0
    for i, f in enumerate(frames):
        shapes = scene.frames[f]
        lo = np.array([bench.world(s.cells).min(0) for s in shapes]) - 1e-3
        hi = np.array([bench.world(s.cells).max(0) for s in shapes]) + 1e-3
        found = set()
        for d in dets[k : k + int(per[i])]:
            p = d["position"].astype(np.float64)
            hit = np.flatnonzero(((p >= lo) & (p <= hi)).all(1))
            assert len(hit) == 1, (f, p)  # (the skew statement, and the match for the others)
            s = shapes[hit[0]]
            assert hit[0] not in found and s.det is not False and int(d["n_points"]) == len(s.cells), (f, s.name)
            found.add(int(hit[0]))
            if s.kind == "sym":
                err = np.abs(p - bench.world(s.cells).mean(0)).max()
                assert err <= bench.pos_tol, (f, s.name, err, bench.pos_tol)
        missing = [s.name for j, s in enumerate(shapes) if s.det is True and j not in found]
        assert not missing, (f, missing)
        k += int(per[i])
    assert k == len(dets)


def _equal(a, b, pa=None, pb=None):
    if pa is not None:
        np.testing.assert_array_equal(pb, pa)
    assert_detections_equal(a, b)


HOST_TAIL_KERNELS = ("k_pack", "k_explore", "k_gather_members")  # what only the host tail launches behind k_tail_far


def _assert_tail(ran, tail, host_tail, host_fill=False):
    """`tail` ran; the host tail followed it (k_pack: the read-back of the full tables it starts with) or did not.  Behind
    k_tail_far a host tail launches k_explore for its fills - unless the radius sent it there: then the fills run on the host"""
    assert ran.get(tail, 0) == 1, ran
    if host_tail is None:
        return
    if host_tail:
        assert ran.get("k_pack", 0) == 1, ran
        if tail == "k_tail_far":
            assert ran.get("k_explore", 0) == (0 if host_fill else 1), ran
    else:
        extra = [k for k in HOST_TAIL_KERNELS if k in ran and not (k == "k_explore" and tail == "k_tail_prep")]
        assert not extra, ran


def _observed(ran):
    return "+".join(k for k in ("k_frame_lds_far", "k_frame_lds_full", "k_far_final", "k_tail_far", "k_tail_prep", "k_explore", "k_tail_finish", "k_pack") if k in ran) or "-"


# ------------------------------------------------------------------------------------------------------------------ the routes
def _run_batch(bench, scene, route, checked, label):
    full = route == "full"
    ref, dev = bench.ref, bench.dev
    scans, tfs = bench.scans, bench.tfs
    da, pa, gs = ref.process_batch(scans, tfs, debug=True)
    counts = _check_honesty(bench, scene, gs, da, pa)
    _check_positions(bench, scene, da, pa)
    (db, pb), ran = _profiled(dev, lambda: dev.process_batch(scans, tfs))  # the production call
    print(f"\n[tail edges] {label}: candidates {counts['candidates']} members {counts['members']} detections {counts['detections']} R {scene.R} route {_observed(ran)}")
    _equal(da, db, pa, pb)
    _check_positions(bench, scene, db, pb)
    if checked:
        host_tail = None if scene.trips == "open" else scene.trips is not None
        if route == "host":
            assert "k_frame_lds_far" in ran and "k_frame_lds_full" not in ran, ran
            assert ran.get("k_pack", 0) == 1 and [k for k in ran if k.startswith(("k_tail", "k_pack"))] == ["k_pack"], ran
        elif full:
            assert "k_frame_lds_full" in ran and "k_frame_lds_far" not in ran and "k_tail_far" not in ran, ran
            assert ran.get("k_tail_finish", 0) == 1 and ran.get("k_explore", 0) >= 1, ran
            _assert_tail(ran, "k_tail_prep", host_tail)  # (k_explore is part of this chain: who ran the fills cannot be told here)
        else:
            assert "k_frame_lds_far" in ran and "k_frame_lds_full" not in ran and "k_tail_prep" not in ran, ran
            _assert_tail(ran, "k_tail_far", host_tail, host_fill=scene.trips == "radius")
    # the pipelined form
    tickets = [dev.batch_submit(scans, tfs) for _ in range(2)]
    for tk in tickets:
        dr, pr = ref.process_batch(scans, tfs)
        dd, pd = dev.batch_collect(tk)
        _equal(dr, dd, pr, pd)
        _check_positions(bench, scene, dd, pd)
    if scene.trips not in (None, "open"):
        # the frame over the capacity rides with three ordinary frames: they come out as if it were not there - as in a batch
        # that holds frame 1 in its place and, where the capacity is one of a frame, stays on the device (the ids count on)
        other = [scans[1]] + list(scans[1:])
        dr, pr = ref.process_batch(other, tfs)
        (dd, pd), ran2 = _profiled(dev, lambda: dev.process_batch(other, tfs))
        _equal(dr, dd, pr, pd)
        if checked:
            # (the radius is a parameter of the whole batch: every frame of that scene exceeds it, this batch takes the host tail too)
            _assert_tail(ran2, "k_tail_prep" if full else "k_tail_far", scene.trips == "radius", host_fill=scene.trips == "radius")
        x, y = db[db["frame"] >= 1].copy(), dd[dd["frame"] >= 1].copy()
        assert len(x) == len(y) and len(x) == int(pb[1:].sum())
        x["id"] -= x["id"][0]
        y["id"] -= y["id"][0]
        assert_detections_equal(x, y)  # (the host tail's boxes against the device's: the helper's tolerances)
    # a read-only batch leaves the map alone, whatever its fills explored
    np.testing.assert_array_equal(dev.read_map(capi.MAP_VOXELS).view(np.uint32), bench.map0.view(np.uint32))
    return counts


def _run_scans(bench, scene, checked, label):
    ref, dev = bench.ref, bench.dev
    counts = None
    for f in scene.scan_frames:
        s = bench.scans[f]
        one = te.Scene([scene.frames[f]], dyn=scene.dyn, unknown=scene.unknown, trips=scene.trips, R=scene.R)
        # the frame's debug view from a read-only call of both sides (on the HIP side: full clustering + host tail)
        da, ga = ref.process_scan(s, bench.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
        dh, gh = dev.process_scan(s, bench.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
        c = _check_honesty(bench, one, [ga], da, [len(da)])
        _equal(da, dh)
        # the call under test
        a = ref.process_scan(s, bench.tf)
        b, ran = _profiled(dev, lambda: dev.process_scan(s, bench.tf))
        if f == scene.scan_frames[0]:
            counts = c
            print(f"\n[tail edges] {label}: candidates {c['candidates']} members {c['members']} detections {len(a)} R {scene.R} route {_observed(ran)}")
        _equal(a, b)
        assert len(a) == len(da)  # (the member voxels' own update does not change a fill's outcome)
        _check_positions(bench, one, a, [len(a)])
        _check_positions(bench, one, b, [len(b)])
        ma, mb = ref.read_map(capi.MAP_VOXELS), dev.read_map(capi.MAP_VOXELS)
        np.testing.assert_array_equal(mb.view(np.uint32), ma.view(np.uint32))
        np.testing.assert_array_equal(dev.read_map(capi.MAP_FLAGS), ref.read_map(capi.MAP_FLAGS))
        c["frontiers"] = int(((ma == np.float32(ref.dp.voxel_map__thresholds__frontiers)) & (bench.map0 != ma)).sum())
        if checked:
            assert ran.get("k_far_final", 0) == 1 and "k_tail_prep" not in ran, ran
            trips = scene.trips if f == 0 or scene.trips in ("radius", "open") else None  # (the radius is a parameter of every frame)
            # more detections than record slots: the fills have written the map, the records are rebuilt from what is on the
            # device (device_tail_overflow_records) - no host-tail kernel follows k_tail_far; the other capacities are noticed
            # before any fill has run and go to the host tail
            _assert_tail(ran, "k_tail_far", None if trips == "open" else trips in ("clusters", "members", "radius"), host_fill=trips == "radius")
        bench.reset_maps()
    return counts


def _run(bench, scene, route, monkeypatch, label):
    checked = _route_checked()  # (before this test's own switch is set)
    if route == "full":
        monkeypatch.setenv("VOFOD_CLOSE_FIRST", "0")  # switches are read on every call
    if route == "host":
        monkeypatch.setenv("VOFOD_DEVICE_TAIL", "0")
    bench.load(scene)
    counts = _run_scans(bench, scene, checked, label) if route == "scan" else _run_batch(bench, scene, route, checked, label)
    bench.clean = True
    return counts


# ------------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n", [63, 64, 65])
def test_candidate_clusters_at_the_capacity(bench, monkeypatch, n, route):
    """case 1, TAIL_MAXC = 64 candidate clusters per frame: 63 and 64 stay on the device, 65 raises TAIL_FB_CLUSTERS alone (192 to
    261 candidate members, 8 detections) and the host tail redoes the batch / the scan"""
    c = _run(bench, te.scene_candidate_clusters(n), route, monkeypatch, f"candidate clusters {n} {route}")
    assert c["candidates"] == n and c["members"] < 512 and c["detections"] == 8
    sizes = [s for s, _ in c["cands"]]
    assert len(set(sizes)) < len(sizes) // 4  # sizes repeat: the canonical order breaks ties by the smallest member


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_candidate_members_at_the_capacity(bench, monkeypatch, n, route):
    """case 2, TAIL_MAXM = 1024 candidate members per frame in 16 candidate clusters: 1025 raises TAIL_FB_MEMBERS alone"""
    c = _run(bench, te.scene_candidate_members(n), route, monkeypatch, f"candidate members {n} {route}")
    assert c["members"] == n and c["candidates"] == 16 and c["detections"] == 8


@pytest.mark.parametrize("route", ROUTES)
def test_cluster_across_member_512(bench, monkeypatch, route):
    """case 2, TAIL_STAGE = 512: k_tail_far keeps the first 512 member centres in LDS and reads the others from global memory.  720
    members in 11 blocks; in the canonical order one block's run starts before list position 512 and ends behind it.  Every block
    is a detection and its position the centroid: a stale or shifted entry on either side of member 512 moves a centre."""
    c = _run(bench, te.scene_member_512(), route, monkeypatch, f"member 512 {route}")
    assert 600 <= c["members"] <= 900 and c["candidates"] == 11 and c["detections"] == 11
    ends = np.cumsum([s for s, _ in c["cands"]])
    starts = ends - np.array([s for s, _ in c["cands"]])
    assert ((starts < 512) & (ends > 512 + 1)).sum() == 1, (starts, ends)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n", [15, 16, 17])
def test_detections_at_the_record_slots(bench, monkeypatch, n, route):
    """case 3, TP_MAXD = 16 detection records per frame, n + 6 candidates.  17 in a batch: TAIL_FB_DETS, the host tail redoes the
    batch with identical records.  17 in a map-updating scan: the fills have already written their frontier voxels (the pockets
    of unknown voxels around six clusters) - device_tail_overflow_records rebuilds the records from d_tailc, no host-tail kernel
    follows k_tail_far; ids, positions, confidences and the map equal the oracle's."""
    c = _run(bench, te.scene_detections(n), route, monkeypatch, f"detections {n} {route}")
    assert c["detections"] == n and c["candidates"] == n + 6 < 64
    if route == "scan":
        assert c["frontiers"] >= 20, c["frontiers"]  # the fills did write the map


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("max_explore,R,open_", [(7.85, 32, False), (8.10, 33, False), (7.75, None, True)])
def test_fill_radius_at_the_limit(bench, monkeypatch, max_explore, R, open_, route):
    """case 4, EX_MAX_R = 32: R = int((obb_size + max_explore_distance) / voxel_size) of 2-voxel clusters (obb_size 0.25 m; the
    planar diagonal pairs: 0.354 m, the same R) at max_explore_distance 7.85 (32.4 / 32.8 -> 32: the device keeps the frame) and
    8.10 (33.4 / 33.8 -> 33: TAIL_FB_RADIUS, host tail); 7.75 is exactly on the boundary for obb_size 0.25 (32.0: float rounding
    decides) and is held to the oracle only.  One cluster sits in a pocket unknown out to Manhattan radius 34 (its fill meets the
    rim: class unknown, no detection, nothing written), one in a pocket unknown out to radius 29: the fill explores all of it - 33 k
    voxels on the work list, the most a fill of R = 32 can take without meeting its rim - writes it to the map as frontier voxels
    and the cluster is a detection.  At R = 32 the device route is kept: "a work list overflow cannot happen for radii the device
    accepts" (frames_collect.h)."""
    c = _run(bench, te.scene_radius(max_explore, R, open_), route, monkeypatch, f"fill radius {max_explore} {route}")
    assert c["candidates"] == 7
    if not open_:
        assert c["detections"] == 6
        assert int((0.25 + max_explore) / 0.25) == R and int((0.25 * np.sqrt(2) + max_explore) / 0.25) == R
        if route == "scan":
            assert c["frontiers"] == len(te.diamond(*te.POCKET_FULL)), c["frontiers"]


@pytest.mark.parametrize("route", GATE_ROUTES)
def test_gates_on_the_device(bench, monkeypatch, route):
    """case 5, the three gates at min_points = 2: obb_size > max_size on lines of 12 / 13 / 14 voxels along every axis (the 13-voxel
    line is exactly 3.0 m long: held to the oracle only) and on the diagonal lines; size >= min_points on single voxels and
    pairs; dist > max_distance on two identical pairs 0.5 m inside and outside.  Which clusters are detections follows from
    the placed geometry."""
    c = _run(bench, te.scene_gates(), route, monkeypatch, f"gates {route}")
    assert c["candidates"] == 17 and 7 <= c["detections"] <= 10


@pytest.mark.parametrize("route", GATE_ROUTES)
def test_min_points_4_on_the_device(bench, monkeypatch, route):
    """case 5, size >= min_points at min_points = 4: clusters of 2 and 3 voxels are dropped, clusters of 4 are detections"""
    c = _run(bench, te.scene_min_points_4(), route, monkeypatch, f"min_points 4 {route}")
    assert c["candidates"] == 6 and c["detections"] == 6


@pytest.mark.parametrize("route", GATE_ROUTES)
def test_degenerate_lattice_shapes_on_the_device(bench, monkeypatch, route):
    """case 6: the shapes of test_obb_gates_on_degenerate_lattice_clusters (repeated eigenvalues everywhere: eigsolve3.h) through the
    device copy of vt::boxes_of_n, at map x above 62 m where float32 is coarse.  55 floating shapes cannot share a frame on the
    device routes (TP_MAXD = 16: the host tail would compute the boxes): 14 / 14 / 14 / 13 in the four frames of the batch, each
    also a single scan.  Route host: the same four frames through the host's call of the same function."""
    scene = te.scene_degenerate()
    assert min(s.cells[:, 0].min() for f in scene.frames for s in f) >= 330 and sum(len(f) for f in scene.frames) == 55
    c = _run(bench, scene, route, monkeypatch, f"degenerate shapes {route}")
    assert c["candidates"] == 14 and c["detections"] == 14


def test_degenerate_lattice_shapes_in_one_scan_beyond_the_record_slots(bench, monkeypatch):
    """case 6 in one frame, on the one device route that can take it: a single map-updating scan with 55 floating shapes.  The record
    slots overflow, device_tail_overflow_records rebuilds all 55 records from d_tailc - positions from the device's boxes, held to
    the two position statements and the oracle."""
    c = _run(bench, te.scene_degenerate_one_scan(), "scan", monkeypatch, "degenerate shapes, one scan")
    assert c["candidates"] == 55 and c["detections"] == 55 and c["members"] < 512
