"""Scenes and expected values of the vofod_detection_points tests (test_detection_points_cpu.py, test_gpu_detection_points.py).

The expected values come from the oracle's debug view alone.  For frame f of `process_batch(..., debug=True)` or of
`process_scan(..., SCAN_NO_MAP_UPDATE, debug=True)`, mav = clusters[cclass == CLASS_MAV] in table order; detection k of the frame
belongs to mav[k] and
    index    == flatnonzero(labels == mav[k].first_member)
    points   == weighted[index]               (bit for bit)
    aabb_min == mav[k].aabb_min, aabb_max == mav[k].aabb_max   (exactly: float min / max of values that are bit-equal on both sides)
The CPU file checks this construction on the oracle itself for every scene below (detections and MAV clusters correspond in
order, n_points is the member count, the first index is first_member, numpy's min / max of the members is the table's AABB), so
that the GPU file's expectations stand on a machine without a GPU."""
from __future__ import annotations

import numpy as np

import tail_edges as te
from vofod_amd import capi


def _big(block_dims, **dyn):
    """frame 0: one block and a pair; the other frames ordinary"""
    pl = te.Placer()
    f = [te.Shape("block %dx%dx%d" % block_dims, pl.take(te.block(*block_dims)), "sym", True, True), te.Shape("pair x", pl.take(te.PAIRS["pair x"]), "sym", True, True)]
    return te.Scene(te._with_ordinary(f), dyn=dyn, trips="open")


def scene_weights():
    """a 3 x 3 x 3 block, a 2 x 2 x 2 cube, a plus and two pairs in frame 0; how often each cell is hit: weights_scans"""
    pl = te.Placer()
    shapes = [("block 3x3x3", te.block(3, 3, 3)), ("2x2x2 cube", te._norm(te.ALIGNED["2x2x2 cube"])), ("plus", te._norm(te.ALIGNED["plus"])), ("pair x", te.PAIRS["pair x"]), ("pair yz", te.PAIRS["pair yz"])]
    return te.Scene(te._with_ordinary([te.Shape(n, pl.take(c), "sym", True, True) for n, c in shapes]), trips="open")


HEAVY = 300  # hits of one member cell: beyond the byte counters of the lean emission (test_gpu_lean_emit.py::test_counters_beyond_255)


def weights_hits(scene):
    """(cells of frame 0, hits per cell): cell i is hit 1 + (i % 5) times, cell 4 of the block HEAVY times"""
    cells = np.vstack([s.cells for s in scene.frames[0]])
    hits = 1 + (np.arange(len(cells)) % 5)
    hits[4] = HEAVY
    return cells, hits


# name -> builder.  The first six are the scenes of test 1 (three routes), the blocks those of the large-member test.
SCENES = {
    "member_512": te.scene_member_512,
    "detections_16": lambda: te.scene_detections(16),
    "detections_17": lambda: te.scene_detections(17),
    "members_1025": lambda: te.scene_candidate_members(1025),
    "clusters_65": lambda: te.scene_candidate_clusters(65),
    "degenerate": te.scene_degenerate,
    "block_7x7x7": lambda: _big((7, 7, 7)),                               # 343 voxels: more than one tile of 256
    "block_8x8x9": lambda: _big((8, 8, 9), classification__max_size=4.0),  # 576: more than the kernel's LDS list of 512
    "block_9x9x9": lambda: _big((9, 9, 9), classification__max_size=4.0),  # 729: a second pass with a remainder
    "gates": te.scene_gates,
    "weights": scene_weights,
}
ROUTE_SCENES = ["member_512", "detections_16", "detections_17", "members_1025", "clusters_65", "degenerate"]
LARGE_SCENES = ["block_7x7x7", "block_8x8x9", "block_9x9x9"]
# detections per frame of the batch, from the placed geometry (the CPU file holds the oracle to them)
PER_FRAME = {"member_512": [11, 3, 4, 5], "detections_16": [16, 3, 4, 5], "detections_17": [17, 3, 4, 5], "members_1025": [8, 3, 4, 5], "clusters_65": [8, 3, 4, 5],
             "degenerate": [14, 14, 14, 13], "block_7x7x7": [2, 3, 4, 5], "block_8x8x9": [2, 3, 4, 5], "block_9x9x9": [2, 3, 4, 5], "gates": [10, 3, 4, 5], "weights": [5, 3, 4, 5]}
LARGEST = {"member_512": 80, "block_7x7x7": 343, "block_8x8x9": 576, "block_9x9x9": 729}


def load(bench, name):
    """the scene `name` loaded into a Bench of test_gpu_tail_edges.py (maps, dynamic parameters, scans); returns the scene"""
    scene = SCENES[name]()
    bench.load(scene)
    if name == "weights":
        from test_gpu_close_first import _cells_scan

        cells, hits = weights_hits(scene)
        bench.scans[0] = _cells_scan(bench.world(np.repeat(cells, hits, axis=0)), bench.t)
    return scene


def expected_frame(g):
    """[(first_member, index, points, aabb_min, aabb_max)] of one frame's debug view, MAV clusters in table order"""
    cl = g["clusters"]
    out = []
    for c in cl[cl["cclass"] == capi.CLASS_MAV]:
        idx = np.flatnonzero(g["labels"] == c["first_member"]).astype(np.uint32)
        out.append((int(c["first_member"]), idx, g["weighted"][idx].copy(), c["aabb_min"].copy(), c["aabb_max"].copy()))
    return out


def self_check(dets, per, gs):
    """the construction on the side that produced `gs`: detections and MAV clusters correspond in order"""
    k = 0
    for f, g in enumerate(gs):
        exp = expected_frame(g)
        assert len(exp) == int(per[f]), (f, len(exp), int(per[f]))
        for first, idx, pts, lo, hi in exp:
            d = dets[k]
            assert int(d["frame"]) == f and int(d["n_points"]) == len(idx) and len(idx) > 0 and int(idx[0]) == first, (f, k)
            xyz = np.stack([pts["x"], pts["y"], pts["z"]], axis=1)
            np.testing.assert_array_equal(xyz.min(0), lo)
            np.testing.assert_array_equal(xyz.max(0), hi)
            assert (np.diff(idx.astype(np.int64)) > 0).all()
            k += 1
    assert k == len(dets)


def assert_points(ext, pts, idx, dets, exp_frames):
    """what detection_points returned for the detections `dets` (frame order) against the expectation of their frames"""
    assert len(ext) == len(dets)
    np.testing.assert_array_equal(ext["id"], dets["id"])
    np.testing.assert_array_equal(ext["frame"], dets["frame"])
    np.testing.assert_array_equal(ext["count"], dets["n_points"].astype(np.uint32))
    np.testing.assert_array_equal(ext["first"], np.concatenate([[0], np.cumsum(ext["count"])[:-1]]).astype(np.uint32) if len(ext) else ext["first"])
    assert len(pts) == len(idx) == int(ext["count"].sum())
    k = 0
    for f, exp in enumerate(exp_frames):
        for first, eidx, epts, lo, hi in exp:
            e = ext[k]
            assert int(e["frame"]) == f, (k, f)
            a, b = int(e["first"]), int(e["first"]) + int(e["count"])
            np.testing.assert_array_equal(idx[a:b], eidx, err_msg=f"index of detection {k} (frame {f})")
            np.testing.assert_array_equal(pts[a:b].view(np.uint32), epts.view(np.uint32), err_msg=f"points of detection {k} (frame {f})")
            np.testing.assert_array_equal(e["aabb_min"], lo)
            np.testing.assert_array_equal(e["aabb_max"], hi)
            k += 1
    assert k == len(ext)
