"""The input pass of the frame kernel (k_frame_lds, kernels_frame.h, phase "in") at the edges of its rounds, and the lean counting
pass behind it.  A round is 16 pieces of 512 points (64 lane units of 8), one piece per wave; the clouds of the other input tests
hold exactly two rounds.  Here: one round, a second round of one quad or one point, three rounds with one of them all zero, and
eight rounds whose 65 536 points all survive - a wave's code segment then reaches beyond the three rounds of codes it keeps in
registers, and the passes behind the input (occupancy words, counting pass) read the rest back from the list in global memory.

Every comparison is HIP against the CPU oracle, bit for bit, in the three views of test_gpu_frame_inputs.three_views (full debug,
far-only, production synchronous and as two tickets), which also asserts from the profile that the frame kernel ran.  Batches of
4-5 frames at 0.25 m on the default area; one frame of every batch is the scene scan as it is, the others carry zero patterns,
and the host asserts that the frames hold the patterns.  No case says which wave takes which piece.

The counting pass of a production batch counts the points of pure-far bricks only (lean emission): the last cases put 300 points
into one voxel of a brick it must skip and into one voxel of a target it must keep."""
import numpy as np
import pytest

from vofod_amd.detector import ScanData

from test_gpu_frame_inputs import DEFAULT_AREA, host_scan, lay_aos48, lay_columns, make_area_pair, scene_frames, survivors, three_views, warm_both

pytestmark = pytest.mark.gpu
f32 = np.float32
UNIT = 8  # points of a lane unit (IN_PPT)
PIECE = 64  # units of a piece: one per lane
WAVES = 16  # pieces of a round
ROUND = UNIT * PIECE * WAVES
LAYOUTS = {"columns": (lay_columns, "packed"), "aos48": (lay_aos48, "strided")}


# (Frame, nonzero_points, live_units, densified, punched, all_surviving: as in test_gpu_input_compaction.py, for any sensor shape)
class Frame:
    """what lay_* / host_scan read of a synth scan, over points of our own"""

    def __init__(self, x, y, z, tf, shape):
        self.x, self.y, self.z = (np.ascontiguousarray(v, dtype=f32) for v in (x, y, z))
        self.intensity = self.range = None
        self.tf = tf
        self.scan = ScanData(x=self.x, y=self.y, z=self.z, width=shape[1], height=shape[0], stride_bytes=4)


def nonzero_points(x, y, z):
    return ((x.view(np.uint32) | y.view(np.uint32) | z.view(np.uint32)) & np.uint32(0x7FFFFFFF)) != 0


def live_units(fr):
    nz = nonzero_points(fr.x, fr.y, fr.z)
    pad = (-nz.size) % UNIT
    return np.concatenate([nz, np.zeros(pad, dtype=bool)]).reshape(-1, UNIT).any(axis=1)


def densified(s, only=None):
    x, y, z = s.x.copy(), s.y.copy(), s.z.copy()
    ok = nonzero_points(x, y, z) if only is None else only
    assert ok.any()
    src = np.maximum.accumulate(np.where(ok, np.arange(ok.size), -1))
    src[src < 0] = np.flatnonzero(ok)[0]
    return x[src], y[src], z[src]


def punched(s, unit_mask, shape, dev):
    """the scan densified to points that survive both crops, the units outside `unit_mask` set to zero in all three coordinates: a
    frame with a live unit has a point behind the crops"""
    fr = all_surviving(s, dev, shape)
    dead = ~np.repeat(np.asarray(unit_mask, dtype=bool), UNIT)[: fr.x.size]
    fr.x[dead] = fr.y[dead] = fr.z[dead] = f32(0.0)
    return fr


def all_surviving(s, dev, shape):
    x, y, z = s.x, s.y, s.z
    _, kept = survivors(np.stack([x, y, z], axis=1), s.tf, DEFAULT_AREA, dev=dev)
    kept &= nonzero_points(x, y, z)
    x, y, z = densified(s, only=kept)
    _, kept = survivors(np.stack([x, y, z], axis=1), s.tf, DEFAULT_AREA, dev=dev)
    assert kept.all()
    return Frame(x, y, z, s.tf, shape)


def units_of(n):
    return (n + UNIT - 1) // UNIT


def live_per_piece(fr):
    """live lane units of every 512-point piece, in scan order (the last piece may be partial)"""
    lu = live_units(fr)
    pad = (-lu.size) % PIECE
    return np.concatenate([lu, np.zeros(pad, dtype=bool)]).reshape(-1, PIECE).sum(axis=1)


def run(ref, dev, frames, layout, name):
    lay, want = LAYOUTS[layout]
    scans_dev = [host_scan(fr, lay(fr)) for fr in frames]
    tfs = np.stack([fr.tf for fr in frames])
    return three_views(ref, dev, [fr.scan for fr in frames], scans_dev, tfs, want, f"rounds/{name}/{layout}", 0, 0)


def warmed(oracle, hip, shape, n_frames):
    ref, dev = make_area_pair(oracle, hip, shape=shape, max_batch=8)
    warm_scene, _, frames = scene_frames(DEFAULT_AREA, (0.0, 0.0), n_frames, shape=shape, scene_seed=5, seed0=70)
    warm_both(ref, dev, warm_scene, (0.0, 0.0), shape=shape)
    return ref, dev, frames


def assert_not_empty(gb, frames):
    for f, (g, fr) in enumerate(zip(gb, frames)):
        if live_units(fr).any():
            assert g["n_input_after_crop"] > 0, f


# ---------------------------------------------------------------------------------------------- round counts at the edges
@pytest.mark.parametrize("vrays,hrays", [(8, 1024), (4, 2049), (3, 2731), (16, 1536)])
def test_round_counts(oracle, hip, vrays, hrays):
    """8 192 points: exactly one round, no next piece exists.  8 196 (n % 8 = 4): the second round is one quad.  8 193 (n % 4 = 1,
    strided only): the second round is one point.  24 576: three rounds, the middle one has a piece before and after it.
    Frames: the scan as it is; only the last round live; the last round all zero; every unit live."""
    shape = (vrays, hrays, 33.2, 120.0)
    n = vrays * hrays
    assert (n, n % UNIT, n % 4) in ((8192, 0, 0), (8196, 4, 0), (8193, 1, 1), (24576, 0, 0))
    ref, dev, frames = warmed(oracle, hip, shape, 4)
    units = units_of(n)
    rounds = (n + ROUND - 1) // ROUND
    in_last = np.arange(units) >= (rounds - 1) * PIECE * WAVES
    if rounds == 1:  # (one round: "only the last round" is the whole scan - a random half of the units instead)
        masks = [np.random.default_rng(8).random(units) < 0.5, np.arange(units) % (2 * PIECE) < PIECE]
    else:
        masks = [in_last, ~in_last]
    fs = [Frame(frames[0].x, frames[0].y, frames[0].z, frames[0].tf, shape)] + [punched(frames[k + 1], m, shape, dev) for k, m in enumerate(masks)]
    fs.append(punched(frames[3], np.ones(units, dtype=bool), shape, dev))
    for fr, m in zip(fs[1:], masks + [np.ones(units, dtype=bool)]):
        np.testing.assert_array_equal(live_units(fr), m)
    if rounds > 1:
        assert in_last.sum() == units - (rounds - 1) * PIECE * WAVES and in_last.sum() in (1, PIECE * WAVES)
    for layout in LAYOUTS if n % 4 == 0 else ["aos48"]:
        gb = run(ref, dev, fs, layout, f"n{n}")
        assert_not_empty(gb, fs)


# ---------------------------------------------------------------------------------------------- three rounds, one of them empty
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_three_round_patterns(oracle, hip, layout):
    """24 576 points.  Round 0 all zero; round 1 all zero (a skipped piece between two live ones); round 2 all zero (the flush
    directly behind a skipped round); every piece of every round 40 live units: each wave's queue takes 40, then 24 + a drain +
    16, then 24 more + a drain + 16, and a flush of 56."""
    shape = (16, 1536, 33.2, 120.0)
    n = shape[0] * shape[1]
    assert n == 3 * ROUND
    ref, dev, frames = warmed(oracle, hip, shape, 5)
    units = units_of(n)
    rnd = np.arange(units) // (PIECE * WAVES)
    rng = np.random.default_rng(9)
    forty = np.zeros((3 * WAVES, PIECE), dtype=bool)
    for p in range(3 * WAVES):
        forty[p, rng.choice(PIECE, 40, replace=False)] = True
    fs = [Frame(frames[0].x, frames[0].y, frames[0].z, frames[0].tf, shape)]
    fs += [punched(frames[1 + k], rnd != k, shape, dev) for k in range(3)]
    fs.append(punched(frames[4], forty.reshape(-1), shape, dev))
    for k in range(3):
        per = live_per_piece(fs[1 + k]).reshape(3, WAVES)
        assert (per[k] == 0).all() and (np.delete(per, k, axis=0) == PIECE).all(), (k, per)
    assert (live_per_piece(fs[4]) == 40).all()
    gb = run(ref, dev, fs, layout, "three")
    assert_not_empty(gb, fs)


# ---------------------------------------------------------------------------------------------- a segment beyond the register rounds
def with_points_at(fr, world_pts, at, shape):
    """frame `fr` with the points from index `at` on replaced by the given world points (as the sensor at the frame's pose sees them)"""
    R, t = fr.tf[:, :3].astype(np.float64), fr.tf[:, 3].astype(np.float64)
    p = ((np.asarray(world_pts, dtype=np.float64) - t) @ R).astype(f32)  # R^T (p - t)
    cols = [np.array(c, dtype=f32, copy=True) for c in (fr.x, fr.y, fr.z)]
    for a in range(3):
        cols[a][at : at + len(p)] = p[:, a]
    return Frame(cols[0], cols[1], cols[2], fr.tf, shape)


def cell_centre(dev, p):
    """centre of the map cell that holds p (the frame's lattice is the map's, shifted by whole cells)"""
    off = np.array(dev.map_offset, dtype=np.float64)
    vs = float(dev.sp.voxel_size)
    return off + (np.floor((np.asarray(p, dtype=np.float64) - off) / vs) + 0.5) * vs


def test_segment_beyond_the_register_rounds(oracle, hip):
    """(32, 2048): 65 536 points = 8 rounds, every point survives both crops: 65 536 codes, so some wave holds 4 096 or more - more
    than the 3 x 1 024 it keeps in registers, whichever wave took which piece.  Two voxels of a floating target next to the
    sensor are written into every piece, so that their codes also lie in the part of a segment that is read back
    from the list.  Production call (route asserted, detections and per-frame counts the oracle's), then the far-only view behind
    it: the counting pass on its global-list leg, lean and full."""
    from test_gpu_lean_emit import _assert_far_views, _assert_same, _production

    shape = (32, 2048, 33.2, 120.0)
    n = shape[0] * shape[1]
    assert n == 8 * ROUND and n // WAVES > 3 * 1024
    ref, dev, frames = warmed(oracle, hip, shape, 4)
    vs = float(dev.sp.voxel_size)
    pieces = n // (UNIT * PIECE)

    def build(rel):
        fs = []
        for s in frames:
            fr = all_surviving(s, dev, shape)
            c0 = cell_centre(dev, s.tf[:, 3].astype(np.float64) + rel)
            for piece in range(pieces):
                fr = with_points_at(fr, [c0, c0 + (vs, 0.0, 0.0), c0, c0 + (vs, 0.0, 0.0)], piece * UNIT * PIECE + 8 * (piece % PIECE), shape)
            _, kept = survivors(np.stack([fr.x, fr.y, fr.z], axis=1), fr.tf, DEFAULT_AREA, dev=dev)
            assert kept.all()
            fs.append(fr)
        return fs

    def target_is_far(g, fr, rel):  # the oracle's own view: the target's voxel holds two points of every piece, in a far cluster
        weight, is_close = heavy_voxels(g, cell_centre(dev, fr.tf[:, 3].astype(np.float64) + rel))
        assert weight >= 2 * pieces, weight
        return is_close == 0

    # where the target floats - next to the sensor, clear of the scene's buildings in every frame - is the oracle's to say
    for rel in ((3.0, 0.0, 1.5), (-3.0, 0.0, 2.0), (0.0, 3.0, 2.5), (0.0, -3.0, 2.5), (4.0, 4.0, 3.0), (-4.0, -4.0, 3.0)):
        fs = build(np.array(rel))
        scans, tfs = [fr.scan for fr in fs], np.stack([fr.tf for fr in fs])
        da, pa, ga = ref.process_batch(scans, tfs, debug=True)
        if all(target_is_far(g, fr, np.array(rel)) for g, fr in zip(ga, fs)):
            break
    else:
        raise AssertionError("no floating position for the target")
    assert all(g["n_input_after_crop"] == n for g in ga)
    print(f"beyond the register rounds: {len(da)} detections, per frame {pa.tolist()}, voxels {[len(g['weighted']) for g in ga]}")
    assert len(da) >= 1
    _assert_same((da, pa), _production(dev, scans, tfs))
    db, pb, gb = dev.process_batch(scans, tfs, debug=True, far_only=True)
    _assert_same((da, pa), (db, pb))
    _assert_far_views(ga, gb)
    _assert_same((da, pa), _production(dev, scans, tfs))


# ---------------------------------------------------------------------------------------------- weights the lean count skips and keeps
@pytest.fixture(scope="module")
def lean_case(oracle, hip):
    from test_gpu_lean_emit import Case

    return Case(oracle, hip)


def scan_with(s, world_pts, at):
    R, t = s.tf[:, :3].astype(np.float64), s.tf[:, 3].astype(np.float64)
    p = ((np.asarray(world_pts, dtype=np.float64) - t) @ R).astype(f32)
    cols = [np.array(c, dtype=f32, copy=True) for c in (s.x, s.y, s.z)]
    for a in range(3):
        cols[a][at : at + len(p)] = p[:, a]
    return ScanData(x=cols[0], y=cols[1], z=cols[2], width=s.scan.width, height=s.scan.height, stride_bytes=4)


def heavy_voxels(g, centre):
    """(weight, is_close of its cluster) of the voxel of the oracle's view whose centre is `centre`"""
    w, lab, cl = g["weighted"], g["labels"], g["clusters"]
    v = np.flatnonzero((np.abs(w["x"] - centre[0]) < 0.01) & (np.abs(w["y"] - centre[1]) < 0.01) & (np.abs(w["z"] - centre[2]) < 0.01))
    assert len(v) == 1, v
    close_of = {int(c["first_member"]): int(c["is_close"]) for c in cl}
    return int(w["range"][v[0]]), close_of[int(lab[v[0]])]


@pytest.mark.parametrize("which", ["skipped_brick", "kept_target"])
def test_weights_the_lean_count_skips_and_keeps(lean_case, which):
    """OS1-16 at 0.25 m, 4 frames, the warmed map of test_gpu_lean_emit.py.  skipped_brick: 300 points in the ground voxel under the
    sensor - a brick with a close voxel, which the lean counting pass skips - and a floating target of two voxels in the same
    frame.  kept_target: 300 points in one voxel of the target itself, from point 362 on, so that 150 lie in piece 0 and 150 in
    piece 1, every third of them 1e-5 m = 4e-5 cells from the cell's upper x face (the fragile band is at least 1e-4 cells wide:
    frame_geometry.ref_lattice).  The production result is the oracle's; the far-only view behind it, which keeps the full
    emission and the full count, shows the voxel with weight 300 (the oracle's view says what the voxel is)."""
    from test_gpu_lean_emit import VS, _assert_far_views, _assert_same, _production

    case, dev = lean_case, lean_case.dev
    s0 = case.frames[0]
    t = s0.tf[:, 3].astype(np.float64)
    c_air = cell_centre(dev, (t[0] + 3.0, t[1], t[2] + 1.5))
    c_air2 = c_air + (VS, 0.0, 0.0)
    c_gnd = cell_centre(dev, (t[0], t[1], 0.0))
    if which == "skipped_brick":
        pts, heavy, want_close = [c_gnd] * 300 + [c_air, c_air2], c_gnd, 1
    else:
        near_face = c_air + (VS / 2 - 1e-5, 0.0, 0.0)
        pts = [near_face if k % 3 == 0 else c_air for k in range(300)] + [c_air2]
        assert abs((near_face[0] - (c_air[0] + VS / 2)) / VS) < 1e-4 and near_face[0] < c_air[0] + VS / 2
        heavy, want_close = c_air, 0
    at = 362
    assert at < UNIT * PIECE < at + 300 and at + len(pts) < 2 * UNIT * PIECE  # two pieces
    scans, tfs = case.batch(0, 4)
    scans = [scan_with(s0, pts, at)] + scans[1:]
    da, pa, ga = case.oracle(f"rounds/{which}", scans, tfs)
    weight, is_close = heavy_voxels(ga[0], heavy)
    assert weight >= 300 and (weight == 300 or which == "skipped_brick") and is_close == want_close, (weight, is_close)
    print(f"lean count, {which}: weight {weight}, close {is_close}, {len(da)} detections, per frame {pa.tolist()}")
    assert len(da) >= 1
    _assert_same((da, pa), _production(dev, scans, tfs))
    db, pb, gb = dev.process_batch(scans, tfs, debug=True, far_only=True)
    _assert_same((da, pa), (db, pb))
    _assert_far_views(ga, gb)
    _assert_same((da, pa), _production(dev, scans, tfs))
