"""Lean emission of the close-first frame kernel (k_frame_lds<1, *> with `lean`, kernels_frame.h): a production batch - read-only,
no debug output - reads the voxel records of the candidates' members only, voxels of pure-far bricks, so the kernel stores (and,
built with FR_LEAN_WEIGHTS, counts the points of) those bricks' voxels alone, at the ranks of the whole frame.  VOFOD_LEAN_EMIT=0 keeps the full emission;
the far-only debug view always has it.

The pattern is test_gpu_close_first.py's: OS1-16 scans at 0.25 m, batches of 4-6 frames (4 is the smallest batch that takes the
frame kernel), a map warmed with 8 scans and handed to the oracle, 8 floating targets.  What a production call returns - detection
records, per-frame counts - equals the oracle's; the hazard that is new with lean emission is a reader that touches a record
this batch did not write, so the cases put stale, plausible records of OTHER frames under the production batch first, and run
the full emission again behind lean launches.  Every production call asserts from the profiler's kernel list that
k_frame_lds_far ran and k_frame_lds_full did not (not under a VOFOD_* switch set from outside, nor oracle against oracle)."""
import os

import numpy as np
import pytest

from vofod_amd import synth
from vofod_amd.detector import ScanData

from helpers import assert_detections_equal, assert_scan_debug_equal, far_view, make_pair, sync_maps

pytestmark = pytest.mark.gpu

SENSOR, VS = "os1-16", 0.25
SELFCHECK = bool(os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"))  # oracle against oracle: no kernels, no device memory
# (read at import: the cases set switches of their own later)
ROUTE_CHECKED = not SELFCHECK and not any(k.startswith("VOFOD_") and k != "VOFOD_TEST_HARNESS_SELFCHECK" for k in os.environ)


def _rebase(got, want):
    got = got.copy()
    if len(got) and len(want):
        got["id"] = (got["id"].astype(np.int64) + int(want["id"][0]) - int(got["id"][0])).astype(got["id"].dtype)
    return got


def _production(dev, scans, tfs, label="k_frame_lds_far", tail=("k_tail_far",)):
    """the production call (no debug output) and the kernels it launched; the frame kernel's label is asserted"""
    from test_gpu_stream_route import profiled_calls

    dev.lib.profile_enable(dev.h, 1)
    try:
        out = dev.process_batch(scans, tfs)
        ran = profiled_calls(dev.lib, dev)
    finally:
        dev.lib.profile_enable(dev.h, 0)
    if ROUTE_CHECKED:
        assert label in ran and not any(k.startswith("k_frame_lds") and k != label for k in ran), ran
        assert any(k in ran for k in tail), ran
    return out


def _assert_same(want, got):
    (da, pa), (db, pb) = want, got
    np.testing.assert_array_equal(pb, pa)
    assert_detections_equal(da, _rebase(db, da))


def _assert_far_views(ga, gb):
    for f, (x, y) in enumerate(zip(ga, gb)):
        try:
            assert_scan_debug_equal(far_view(x), y)
        except AssertionError as e:
            raise AssertionError(f"frame {f}: {e}") from e


class Case:
    """one warmed pair and twelve frames with targets, shared by the cases: batches are read-only, the map stays as warmed, and the
    oracle's answers are computed once per batch"""

    def __init__(self, oracle, hip):
        self.ref, self.dev = make_pair(oracle, hip, SENSOR, VS, max_batch=6)
        self.warm_scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=0)
        self.scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=8)
        from test_gpu_frame_inputs import warm_both

        # surveyed background (both latches), the ground patch below the sensor, 8 map-updating scans before the targets appear, free
        # space surveyed: a target that appears afterwards is floating - a detection
        warm_both(self.ref, self.dev, self.warm_scene, (0.0, 0.0), shape=SENSOR, n_scans=8)
        sync_maps(self.dev, self.ref)
        self.frames = synth.bench_frames(self.scene, SENSOR, 12)
        self._oracle = {}

    def batch(self, lo, hi):
        fr = self.frames[lo:hi]
        return [s.scan for s in fr], np.stack([s.tf for s in fr])

    def oracle(self, key, scans, tfs):
        """(detections, per-frame counts, full debug view) of the oracle, once per key"""
        if key not in self._oracle:
            self._oracle[key] = self.ref.process_batch(scans, tfs, debug=True)
        return self._oracle[key]


@pytest.fixture(scope="module")
def case(oracle, hip):
    return Case(oracle, hip)


def test_lean_equals_full_equals_oracle(case, monkeypatch):
    """the production call, two tickets in flight, and the same batch under VOFOD_LEAN_EMIT=0 (read on every call: same kernel
    label, full emission): detections and per-frame counts are the oracle's in all of them"""
    scans, tfs = case.batch(0, 6)
    da, pa, ga = case.oracle("A6", scans, tfs)
    n_far = [int((g["clusters"]["is_close"] == 0).sum()) for g in ga]
    print(f"lean=full=oracle: {len(da)} detections, per frame {pa.tolist()}, far clusters {n_far}, voxels {[len(g['weighted']) for g in ga]}")
    assert max(n_far) >= 2 and len(da) >= 1, (n_far, len(da))  # (the oracle's own output: the batch has candidates to read)
    _assert_same((da, pa), _production(case.dev, scans, tfs))
    tickets = [case.dev.batch_submit(scans, tfs) for _ in range(2)]
    for t in tickets:
        _assert_same((da, pa), case.dev.batch_collect(t))
    monkeypatch.setenv("VOFOD_LEAN_EMIT", "0")
    _assert_same((da, pa), _production(case.dev, scans, tfs))
    monkeypatch.delenv("VOFOD_LEAN_EMIT")
    _assert_same((da, pa), _production(case.dev, scans, tfs))


def test_stale_records_of_other_frames(case, monkeypatch):
    """One handle, in order: production batch A; the far-only debug view of OTHER frames C - the full emission: it leaves complete,
    plausible records in every slot; production batch B with other poses through the device tail, and again under
    VOFOD_DEVICE_TAIL=0, where k_pack reads the same records for the host tail - and more of them: the far clusters' table and
    up to 768 candidate members with their voxel records, all of them in pure-far bricks, which B's lean launch writes.  A reader
    that touched a record B did not write would now see C's.  Then C's view once more: bit-exact against the oracle's far view, weights included - a lean launch
    leaves nothing behind (extras list, parked bitmap) that a full launch trips over."""
    A, C_, B = case.batch(0, 4), case.batch(4, 8), case.batch(8, 12)
    oa, oc, ob = case.oracle("A4", *A), case.oracle("C4", *C_), case.oracle("B4", *B)
    assert len(ob[0]) >= 1 and len(oa[0]) >= 1  # (the oracle's own output)
    _assert_same(oa[:2], _production(case.dev, *A))
    dc, pc, gc = case.dev.process_batch(*C_, debug=True, far_only=True)
    _assert_same(oc[:2], (dc, pc))
    _assert_far_views(oc[2], gc)
    _assert_same(ob[:2], _production(case.dev, *B))
    monkeypatch.setenv("VOFOD_DEVICE_TAIL", "0")
    from test_gpu_stream_route import profiled_calls

    case.dev.lib.profile_enable(case.dev.h, 1)
    try:
        got = case.dev.process_batch(*B)
        ran = profiled_calls(case.dev.lib, case.dev)
    finally:
        case.dev.lib.profile_enable(case.dev.h, 0)
    monkeypatch.delenv("VOFOD_DEVICE_TAIL")
    if ROUTE_CHECKED:
        assert "k_frame_lds_far" in ran and "k_pack" in ran and "k_tail_far" not in ran, ran
    _assert_same(ob[:2], got)
    dc2, pc2, gc2 = case.dev.process_batch(*C_, debug=True, far_only=True)
    _assert_same(oc[:2], (dc2, pc2))
    _assert_far_views(oc[2], gc2)


def _with_copies(s, world_pts):
    """frame `s` with its first returns replaced by the given world points (as the sensor at the frame's pose sees them)"""
    R, t = s.tf[:, :3].astype(np.float64), s.tf[:, 3].astype(np.float64)
    p = ((np.asarray(world_pts, dtype=np.float64) - t) @ R).astype(np.float32)  # R^T (p - t)
    cols = [np.array(c, dtype=np.float32, copy=True) for c in (s.x, s.y, s.z)]
    for a in range(3):
        cols[a][: len(p)] = p[:, a]
    return ScanData(x=cols[0], y=cols[1], z=cols[2], width=s.scan.width, height=s.scan.height, stride_bytes=4)


def test_counters_beyond_255(case):
    """Frame 0 carries 300 copies of a point in a floating voxel (3 m beside the sensor, 1.5 m above it: a pure-far brick - its
    extra is applied to the written record) and 300 copies in the ground voxel under the sensor (a close brick: its extra must be
    dropped, not added at a rank nobody wrote).  A byte counter holds 255: both go through the extras list.  Production detections
    are the oracle's; the far-only debug view of the same batch, run afterwards with the full emission, is bit-exact, the two
    weights of 300 included.  That the two voxels are what the case says is read from the oracle's own view."""
    dev = case.dev
    s0 = case.frames[0]
    off = np.array(dev.map_offset, dtype=np.float64)
    t = s0.tf[:, 3].astype(np.float64)

    def centre(p):  # centre of the map cell that holds p (the frame's lattice is the map's, shifted by whole cells)
        return off + (np.floor((np.asarray(p) - off) / VS) + 0.5) * VS

    c_air = centre((t[0] + 3.0, t[1], t[2] + 1.5))
    c_air2 = c_air + (VS, 0.0, 0.0)  # (a second voxel: a cluster of two reaches min_points)
    c_gnd = centre((t[0], t[1], 0.0))
    pts = [c_air] * 300 + [c_gnd] * 300 + [c_air2]
    scans, tfs = case.batch(0, 4)
    scans = [_with_copies(s0, pts)] + scans[1:]
    da, pa, ga = case.oracle("X4", scans, tfs)
    w, lab, cl = ga[0]["weighted"], ga[0]["labels"], ga[0]["clusters"]
    heavy = np.flatnonzero(w["range"] >= 300)
    assert len(heavy) == 2, w["range"][heavy]
    close_of = {int(c["first_member"]): int(c["is_close"]) for c in cl}
    kinds = {}
    for v in heavy:
        d_air = max(abs(w["x"][v] - c_air[0]), abs(w["y"][v] - c_air[1]), abs(w["z"][v] - c_air[2]))
        kinds["air" if d_air < 0.01 else "ground"] = (int(w["range"][v]), close_of[int(lab[v])])
    assert kinds["air"] == (300, 0) and kinds["ground"][0] >= 300 and kinds["ground"][1] == 1, kinds
    print(f"counters beyond 255: {kinds}, {len(da)} detections, per frame {pa.tolist()}")
    _assert_same((da, pa), _production(dev, scans, tfs))
    db, pb, gb = dev.process_batch(scans, tfs, debug=True, far_only=True)
    _assert_same((da, pa), (db, pb))
    _assert_far_views(ga, gb)
    _assert_same((da, pa), _production(dev, scans, tfs))


def test_degenerate_frames_in_one_batch(case):
    """Four frames: no return at all (every pixel (0, 0, 0): the exclude box drops them - an empty frame), a frame whose pose puts
    every point outside the operation area (cropped away entirely), a frame of the scene without targets in which the oracle finds
    no far cluster (no candidate, nothing to read), and a frame with targets.  Counts and detections are the oracle's."""
    s = case.frames[1]
    n = s.scan.width * s.scan.height
    zeros = ScanData(x=np.zeros(n, np.float32), y=np.zeros(n, np.float32), z=np.zeros(n, np.float32), width=s.scan.width, height=s.scan.height, stride_bytes=4)
    away = s.tf.copy()
    away[:, 3] += np.float32([1000.0, 1000.0, 0.0])
    bare = synth.make_scan(case.warm_scene, case.frames[2].tf, SENSOR, seed=2)
    scans = [zeros, s.scan, bare.scan, case.frames[3].scan]
    tfs = np.stack([s.tf, away, bare.tf, case.frames[3].tf])
    da, pa, ga = case.oracle("D4", scans, tfs)
    nv = [len(g["weighted"]) for g in ga]
    n_far = [int((g["clusters"]["is_close"] == 0).sum()) for g in ga]
    print(f"degenerate frames: voxels {nv}, far clusters {n_far}, {len(da)} detections, per frame {pa.tolist()}")
    assert nv[0] == 0 and nv[1] == 0 and nv[2] > 1000 and nv[3] > 1000, nv
    assert n_far[2] == 0 and n_far[3] >= 1, n_far
    _assert_same((da, pa), _production(case.dev, scans, tfs))
    tk = case.dev.batch_submit(scans, tfs)
    _assert_same((da, pa), case.dev.batch_collect(tk))


@pytest.mark.skipif(SELFCHECK, reason="device memory: the oracle reads host memory only")
def test_strided_instantiation(case):
    """the frames of the first case as 48-byte structs in device memory, read where they lie: k_frame_lds_far_strided, lean, with
    the same detections"""
    from test_gpu_frame_inputs import DeviceBlocks, lay_aos48

    scans, tfs = case.batch(0, 6)
    da, pa, _ = case.oracle("A6", scans, tfs)
    blocks = DeviceBlocks()
    try:
        dscans = [blocks.scan(s, lay_aos48(s)) for s in case.frames[0:6]]
        assert all(d.stride_bytes == 48 for d in dscans)
        _assert_same((da, pa), _production(case.dev, dscans, tfs, label="k_frame_lds_far_strided"))
        tk = case.dev.batch_submit(dscans, tfs)
        _assert_same((da, pa), case.dev.batch_collect(tk))
    finally:
        blocks.free()
