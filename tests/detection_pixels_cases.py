"""The statement of vofod_detection_pixels in numpy, and the scenes of its tests (test_detection_pixels_cpu.py,
test_gpu_detection_pixels.py).  Independent of the kernel: nothing here calls the product's new entry point.

Pixel i of a frame belongs to detection d iff the pipeline kept its point and the point's VoxelGridWeighted cell is the cell of a
member voxel of d.  Per frame:
  columns    the x, y, z the pipeline consumed (for range images and col_tfs scans: what range_to_points / deskew_points return);
  survivors  the two crops and the transform exactly as statements.filter_and_transform_of_a_scan_against_numpy_crops;
  lattice    grid.offset and div_b the stand-alone voxel_grid_weighted reports for the survivors (its output is the frame's
             weighted cloud bit for bit, in the same order - asserted - so its keys are the keys of the frame's voxels);
  keys       each survivor's key in float32, as statements.weighted_grid_against_numpy_unique;
  members    of each detection from the oracle's debug view: labels == first_member of the detection's (MAV) cluster, as
             detection_points_cases.expected_frame.
From these: the expected pixels per detection (ascending), the member rank of each (position of its voxel in the detection's list
as vofod_detection_points returns it: ascending weighted-cloud index) and xyz (the transformed point)."""
from __future__ import annotations

import numpy as np

import detection_points_cases as dpc
import tail_edges as te
from vofod_amd import capi
from vofod_amd.detector import voxel_grid_weighted

f32 = np.float32


def _box(off, size):
    o, sz = np.array(list(off), dtype=f32), np.array(list(size), dtype=f32)
    c = o.copy()
    c[2] = o[2] + sz[2] / f32(2)  # the yaml's z offset is the bottom of the box (vofod_nodelet.cpp:204, :212)
    return c - sz / f32(2), c + sz / f32(2)


def survivors(sp, x, y, z, tf):
    """(mask of the pixels the pipeline keeps, q [n, 3] float32: the transformed points, and whether q lies ON a face of the area)"""
    x, y, z = (np.asarray(a, dtype=f32).reshape(-1) for a in (x, y, z))
    lo, hi = _box(sp.exclude_offset, sp.exclude_size)
    with np.errstate(invalid="ignore"):
        inside_ex = (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
        keep = ~inside_ex & np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        tf = np.asarray(tf, dtype=f32).reshape(3, 4)
        q = np.stack([tf[r, 0] * x + (tf[r, 1] * y + (tf[r, 2] * z + tf[r, 3])) for r in range(3)], axis=1).astype(f32)  # every operation rounded to float
        lo, hi = _box(sp.oparea_offset, sp.oparea_size)
        keep = keep & (q >= lo).all(1) & (q <= hi).all(1)
        on_face = keep & ((q == lo).any(1) | (q == hi).any(1))
    return keep, q, on_face


def expected_frame(lib, det, cols, tf, g):
    """[(pixels, member, xyz)] of one frame, detections in the order returned.  `det` is a detector of `lib` with the frame's
    parameters (its handle runs the stand-alone grid), `g` the frame's debug view from the oracle."""
    sp, vs = det.sp, det.sp.voxel_size
    keep, q, _ = survivors(sp, *cols, tf)
    assert int(keep.sum()) == g["n_input_after_crop"]
    px = np.flatnonzero(keep).astype(np.uint32)
    qs = q[keep]
    align = np.array(det.map_offset, dtype=f32) + f32(vs) / f32(2)  # idxToCoord(0, 0, 0) (:664)
    pts, keys, grid, _ = voxel_grid_weighted(lib, qs[:, 0], qs[:, 1], qs[:, 2], vs, align, handle=det.h)
    np.testing.assert_array_equal(pts.view(np.uint32), g["weighted"].view(np.uint32))
    off, div = f32(list(grid.offset)), np.int64(list(grid.div_b))
    inv = f32(1.0) / f32(vs)
    cell = np.floor(((qs - off).astype(f32) * inv).astype(f32)).astype(np.int64)
    k = cell[:, 0] + cell[:, 1] * div[0] + cell[:, 2] * div[0] * div[1]
    out = []
    cl = g["clusters"]
    for c in cl[cl["cclass"] == capi.CLASS_MAV]:
        idx = np.flatnonzero(g["labels"] == c["first_member"])
        mk = keys[idx].astype(np.int64)
        assert (np.diff(mk) > 0).all()  # (the weighted cloud is in key order: ascending index is ascending key)
        sel = np.isin(k, mk)
        member = np.searchsorted(mk, k[sel]).astype(np.uint32)
        out.append((px[sel], member, qs[sel].copy()))
        # the invariant, on the oracle's numbers: every member voxel gets exactly its weight in pixels
        np.testing.assert_array_equal(np.bincount(member, minlength=len(idx)), g["weighted"]["range"][idx].astype(np.int64))
    return out


def boundary_fraction(xyz, vs, origin):
    """per point: whether a coordinate lies exactly on a multiple of the voxel size from `origin` (a cell boundary of the map)"""
    r = (xyz.astype(np.float64) - np.asarray(origin, dtype=np.float64)) / vs
    return (r == np.round(r)).any(1)


def assert_pixels(span, px, member, xyz, dets, exp_frames):
    """what detection_pixels returned for the detections `dets` (frame order) against the expectation of their frames: span, pixels
    and member exact, xyz bit for bit"""
    assert len(span) == len(dets)
    np.testing.assert_array_equal(span["id"], dets["id"])
    np.testing.assert_array_equal(span["frame"], dets["frame"])
    np.testing.assert_array_equal(span["first"], np.concatenate([[0], np.cumsum(span["count"])[:-1]]).astype(np.uint32) if len(span) else span["first"])
    assert len(px) == len(member) == len(xyz) == int(span["count"].sum())
    k = 0
    for f, exp in enumerate(exp_frames):
        for epx, emem, exyz in exp:
            s = span[k]
            assert int(s["frame"]) == f, (k, f)
            a, b = int(s["first"]), int(s["first"]) + int(s["count"])
            assert int(s["count"]) == len(epx), (k, f, int(s["count"]), len(epx))
            np.testing.assert_array_equal(px[a:b], epx, err_msg=f"pixels of detection {k} (frame {f})")
            np.testing.assert_array_equal(member[a:b], emem, err_msg=f"member of detection {k} (frame {f})")
            np.testing.assert_array_equal(np.ascontiguousarray(xyz[a:b]).view(np.uint32), np.ascontiguousarray(exyz).view(np.uint32), err_msg=f"xyz of detection {k} (frame {f})")
            k += 1
    assert k == len(span)


# ---------------------------------------------------------------------------------------------------------------- the scenes
def scene_boundary():
    """the shapes of the weights scene; load() gives every cell of frame 0 two returns: its centre, and its lower corner - a point
    on exact multiples of the voxel size in the world frame, on the boundary of eight cells, which float rounding of the frame's own
    lattice (not the map's) puts into one of them.  The corner may land in a neighbour of the shape's cells: such a voxel joins
    the shape's cluster (tolerance: 6 cells), so the detections are the oracle's to count."""
    return dpc.scene_weights()


SCENES = {**dpc.SCENES, "boundary": scene_boundary}
# the scenes the GPU file runs through the routes, and those of the large detections
ROUTE_SCENES = ["weights", "boundary", "detections_17"]
LARGE_SCENES = dpc.LARGE_SCENES
ALL_SCENES = ROUTE_SCENES + LARGE_SCENES + ["degenerate", "member_512"]


def load(bench, name):
    """the scene `name` loaded into a Bench of test_gpu_tail_edges.py; returns the scene"""
    if name != "boundary":
        return dpc.load(bench, name)
    from test_gpu_close_first import _cells_scan

    scene = SCENES[name]()
    bench.load(scene)
    cells = np.vstack([s.cells for s in scene.frames[0]])
    corners = bench.off + cells.astype(np.float64) * te.VS
    bench.scans[0] = _cells_scan(np.vstack([bench.world(cells), corners]), bench.t)
    return scene


def columns(scan):
    return scan.x, scan.y, scan.z


def expected_batch(lib, ref, scans, tfs, cols=None):
    """(detections, per-frame counts, [expected_frame]) of the oracle's read-only batch over `scans` (host point scans)"""
    da, pa, gs = ref.process_batch(scans, tfs, debug=True)
    cols = [columns(s) for s in scans] if cols is None else cols
    return da, pa, [expected_frame(lib, ref, c, tf, g) for c, tf, g in zip(cols, tfs, gs)], gs
