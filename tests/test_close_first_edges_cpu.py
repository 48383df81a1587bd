"""The scenes of tests/close_first_edges.py hold what they claim: exactly FAR_MAX - 1 / FAR_MAX / FAR_MAX + 1 far-by-themselves voxels, exactly
CF_MAX - 1 / CF_MAX / CF_MAX + 1 pure-far bricks.  Checked twice, without the product library: by a numpy statement of hasCloseTo's stencil on
the base map and the placed cells (statements.close_at), and against the oracle's debug view - clusters, close flags, sizes, candidates and
detections; the tainted chain sits in a close cluster, the filler never yields a candidate.  Without this file the GPU tests could miss the
edge by a voxel and still pass."""
import numpy as np
import pytest

import close_first_edges as ce
import statements as st
import tail_edges as te
from test_gpu_tail_edges import Bench
from vofod_amd import capi

VS = ce.VS
CAP = ce.capacities()
FAR_MAX, CF_MAX = CAP["FAR_MAX"], CAP["CF_MAX"]


@pytest.fixture(scope="module")
def bench(oracle):
    b = Bench(oracle, oracle)
    yield b
    b.close()


def test_capacities_are_read_from_the_headers():
    assert CAP == {"FAR_MAX": 4096, "FR_THREADS": 1024, "CF_MAX": 1024, "TAIL_MAXC": 64, "TAIL_MAXM": 1024}, CAP


def test_close_at_is_close_image_at_the_cells():
    """the stencil read at single cells against the dilation of the whole (small) map, faces and corners included"""
    rng = np.random.default_rng(3)
    m = np.full((20, 24, 28), -1000.0, dtype=np.float32)
    m[rng.random(m.shape) < 0.002] = 0.0
    zz, yy, xx = np.meshgrid(*(np.arange(n) for n in m.shape), indexing="ij")
    cells = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1)
    want = st.close_image(m, np.float32(-300.0), np.float32(1.5), 0.25)
    got = st.close_at(m, np.float32(-300.0), np.float32(1.5), 0.25, cells).reshape(m.shape)
    assert want.any() and not want.all()
    np.testing.assert_array_equal(got, want)


def _frame_statements(bench, shapes, g, dp):
    """one frame: the placed cells are the oracle's voxels; numpy's close bits give the oracle's far clusters; returns the counts"""
    ref = bench.ref
    thr = np.float32(dp.voxel_map__thresholds__new_obstacles)
    placed = np.vstack([s.cells for s in shapes])
    assert len(np.unique(placed, axis=0)) == len(placed)
    pts, lab, cl = g["weighted"], g["labels"], g["clusters"]
    assert len(pts) == len(placed) and (pts["range"] == 1).all()  # nothing dropped by the exclude box or the crop, one return per cell
    cell = st.map_cells(pts, bench.off.astype(np.float32), VS)
    key = lambda c: (c[:, 2] * 1024 + c[:, 1]) * 1024 + c[:, 0]
    np.testing.assert_array_equal(np.sort(key(cell)), np.sort(key(placed)))
    far = ce.far_by_itself(bench.map0, thr, cell)
    # the claim of every role, from the stencil alone
    lut = dict(zip(key(cell).tolist(), far.tolist()))
    for s in shapes:
        f = np.array([lut[k] for k in key(s.cells).tolist()])
        assert f.all() if ce.role(s) != "close" else not f.any(), s.name
    # numpy's close bits and the oracle's clustering agree: far clusters = untainted components of the far voxels
    P = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float32)
    n_far_clusters = st.assert_far_clusters_are_untainted_components(P, np.float32(dp.ground_points_max_distance), ~far, lab, cl)
    close_of_root = dict(zip(cl["first_member"].tolist(), cl["is_close"].tolist()))
    idx_of = dict(zip(key(cell).tolist(), range(len(cell))))
    for s in shapes:
        roots = {int(lab[idx_of[k]]) for k in key(s.cells).tolist()}
        assert len(roots) == 1, s.name  # a shape is in one cluster
        assert bool(close_of_root[roots.pop()]) == (ce.role(s) in ("close", "chain", "taint")), s.name
    # candidates as the tail counts them (test_gpu_tail_edges._frame_counts)
    lim = dp.classification__max_size * (1 + 1e-4) + 1e-3 * VS
    cands = []
    for c in cl:
        if c["is_close"] or int(c["n_points"]) < dp.classification__min_points:
            continue
        mem = cell[lab == c["first_member"]]
        if (((mem.max(0) - mem.min(0)) * np.float32(VS)) <= lim).all():
            cands.append(mem)
    want = sorted(key(s.cells).tolist() for s in shapes if s.cand)
    assert sorted(sorted(key(m).tolist()) for m in cands) == [sorted(w) for w in want]  # the candidates are the shapes built as such: no filler among them
    return dict(n_far=int(far.sum()), far_clusters=n_far_clusters, close_clusters=int(cl["is_close"].sum()), cand_clusters=len(cands), cand_members=sum(len(m) for m in cands),
                pure_far_bricks=ce.pure_far_bricks(cell, far, bench.off, ref.sp))


def _detections_are_the_claimed_shapes(bench, shapes, dets):
    lo = np.array([bench.world(s.cells).min(0) for s in shapes if s.det]) - 1e-3
    hi = np.array([bench.world(s.cells).max(0) + 1e-3 for s in shapes if s.det])
    hit = [np.flatnonzero(((d["position"] >= lo) & (d["position"] <= hi)).all(1)) for d in dets]
    assert all(len(h) == 1 for h in hit) and len({int(h[0]) for h in hit}) == len(dets)


@pytest.mark.parametrize("filler", ["block", "singles"])
@pytest.mark.parametrize("dk", [-1, 0, 1])
def test_single_scan_scenes_sit_at_the_edge(bench, dk, filler):
    scene = ce.single_scan(FAR_MAX + dk, filler)
    bench.load(scene)
    s, shapes, c = bench.scans[0], scene.frames[0], scene.claims
    dets, g = bench.ref.process_scan(s, bench.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
    got = _frame_statements(bench, shapes, g, bench.ref.dp)
    print(f"\n[close-first edges] S({FAR_MAX + dk}, {filler}): {got}, detections {len(dets)}")
    assert c["n_far"] == FAR_MAX + dk
    for k in ("n_far", "far_clusters", "close_clusters", "cand_clusters", "cand_members"):
        assert got[k] == c[k], (k, got[k], c[k])
    assert len(dets) == c["detections"] == 5
    _detections_are_the_claimed_shapes(bench, shapes, dets)
    if filler == "singles":
        assert c["far_clusters"] > 3800
    # the map-updating scan finds the same detections and pulls the chain to scores/point with flag 2, the filler to scores/unknown with flag 3
    d2 = bench.ref.process_scan(s, bench.tf)
    assert len(d2) == 5
    m, fl = bench.ref.read_map(capi.MAP_VOXELS), bench.ref.read_map(capi.MAP_FLAGS)
    ch, fi = ce.cells_of(shapes, "chain"), ce.cells_of(shapes, "filler")
    dp = bench.ref.dp
    half = lambda score: np.float32(0.5) * np.float32(dp.voxel_map__scores__ray) + np.float32(0.5) * np.float32(score)
    assert (fl[ch[:, 2], ch[:, 1], ch[:, 0]] == 2).all() and (m[ch[:, 2], ch[:, 1], ch[:, 0]] == half(dp.voxel_map__scores__point)).all()
    assert (fl[fi[:, 2], fi[:, 1], fi[:, 0]] == 3).all() and (m[fi[:, 2], fi[:, 1], fi[:, 0]] == half(dp.voxel_map__scores__unknown)).all()


def test_singles_become_candidates_at_min_points_1(bench):
    """the scene of test_single_scan_capacity_meets_the_tails: FAR_MAX far voxels, and with classification__min_points = 1 more candidate
    clusters than TAIL_MAXC and more candidate members than TAIL_MAXM"""
    scene = ce.single_scan(FAR_MAX, "singles", min_points=1)
    bench.load(scene)
    dets, g = bench.ref.process_scan(bench.scans[0], bench.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True, det_cap=8192)
    got = _frame_statements(bench, scene.frames[0], g, bench.ref.dp)
    c = scene.claims
    print(f"\n[close-first edges] S({FAR_MAX}, singles) at min_points 1: {got}, detections {len(dets)}")
    assert got["n_far"] == c["n_far"] == FAR_MAX
    assert got["cand_clusters"] == c["cand_clusters"] > CAP["TAIL_MAXC"] and got["cand_members"] == c["cand_members"] > CAP["TAIL_MAXM"]
    assert len(dets) > 1000


@pytest.mark.parametrize("edge_frame", [0, 3])
@pytest.mark.parametrize("dp_", [-1, 0, 1])
def test_batch_scenes_sit_at_the_edge(bench, dp_, edge_frame):
    scene = ce.batch(CF_MAX + dp_, edge_frame)
    bench.load(scene)
    dets, per, gs = bench.ref.process_batch(bench.scans, bench.tfs, debug=True)
    c = scene.claims
    np.testing.assert_array_equal(per, c["detections"])
    k = 0
    for f, (shapes, g) in enumerate(zip(scene.frames, gs)):
        got = _frame_statements(bench, shapes, g, bench.ref.dp)
        _detections_are_the_claimed_shapes(bench, shapes, dets[k : k + int(per[f])])
        k += int(per[f])
        if f == edge_frame:
            print(f"\n[close-first edges] B({CF_MAX + dp_}) in frame {edge_frame}: {got}")
            assert c["pure_far_bricks"] == CF_MAX + dp_
            for name in ("pure_far_bricks", "far_clusters", "close_clusters", "cand_clusters", "cand_members"):
                assert got[name] == c[name], (name, got[name], c[name])
            # every filler voxel but the odd one of a broken row has a neighbour at exactly the tolerance: 36 < 36 is false, no edge
            fi = ce.cells_of(shapes, "filler")
            d = fi[:, None, :] - fi[None, :, :]
            assert ((d * d).sum(-1) == ce.TOL_CELLS**2).any(1).sum() >= len(fi) - 1
        else:
            assert got["pure_far_bricks"] == c["small_pure_far_bricks"] and got["cand_clusters"] == 1
