"""Lean ranks of the close-first frame kernel (k_frame_lds<1, *>, kernels_frame.h, pass 4): in a lean launch the rank tables nodeA /
rowT are built for the bricks of the pure-far list only - a walk over the brick row of every list entry - and pass c sums every
node's own layer counts.  VOFOD_LEAN_RANKS=0 (read on every call) keeps the frame-wide passes a / b / c, as does a frame whose
list is longer than FR_LEAN_RANKS_MAX.

A wrong rank reads or writes another voxel's record: it shows in the detections and in vofod_detection_points.  Every case
compares (a) the production call - k_frame_lds_far, asserted from the profiler's kernel list -, (b) the same batch under
VOFOD_LEAN_RANKS=0 and (c) the oracle: detection records, per-frame counts and the detections' points, bit for bit between (a) and
(b), within the helpers' tolerances against the oracle (points and indices: bit for bit).  The recipe is the hand-placed one of
tests/tail_edges.py / close_first_edges.py - OS1-16, 0.25 m, four frames, the returns of a scan are centres of chosen map cells,
both maps written from one array - because the cases are statements about bricks: which brick row a target shares with map-known
bricks, and where in the row it lies.  That a case holds what it says is read from the oracle's debug view alone."""
import re

import numpy as np
import pytest

import close_first_edges as ce
import detection_points_cases as dpc
import frame_geometry as fg
import statements as st
import tail_edges as te
from test_gpu_lean_emit import SELFCHECK, _assert_far_views, _assert_same, _production
from test_gpu_tail_edges import Bench

pytestmark = pytest.mark.gpu

VS = te.VS
BY, BZ = 60, 10   # the brick row of the cases: 10 m beside the sensor, 5 m above it, 32 layers above the background sheet
TBX = 80          # the target's brick: 7 m in front of the sensor (a candidate is classified out to 45 m)
BX0 = TBX - 12    # first brick of the short rows
GAP = 3           # empty bricks between a target and the surveyed bricks: 9 cells and more, beyond hasCloseTo's reach and the tolerance (6)


def _threshold():
    src = (ce.ROOT / "vofod_amd" / "csrc" / "kernels_frame.h").read_text()
    m = re.search(r"#define\s+FR_LEAN_RANKS_MAX_DEF\s+(\d+)", src)
    assert m and re.search(r"FR_LEAN_RANKS_MAX\s*=\s*FR_LEAN_RANKS_MAX_DEF\s*;", src)
    return int(m.group(1))


@pytest.fixture(scope="module")
def bench(oracle, hip):
    b = Bench(oracle, hip)
    lat = fg.ref_lattice(list(b.dev.sp.oparea_offset), list(b.dev.sp.oparea_size), float(b.dev.sp.voxel_size))
    b.shift = np.round((np.asarray(b.dev.map_offset, dtype=np.float64) - lat["off"].astype(np.float64)) / VS).astype(np.int64)
    yield b
    b.close()


def _cells(bench, brick, inb):
    """map cells at the positions `inb` (cells inside the brick, may reach into the next one) of brick `brick`"""
    return 4 * np.asarray(brick, dtype=np.int64) - bench.shift + np.asarray(inb, dtype=np.int64).reshape(-1, 3)


def _bricks(bench, cells):
    return ce.brick_of(cells, bench.dev.map_offset, bench.dev.sp)


def _wall(bench, bxs, by=BY, bz=BZ):
    """one voxel in every brick bx of the row (by, bz)"""
    return np.vstack([_cells(bench, (bx, by, bz), [(1, 1, 1)]) for bx in bxs]) if len(bxs) else np.zeros((0, 3), dtype=np.int64)


def _load(bench, frames, surveyed):
    """four frames of map cells (a cell may repeat: so many returns) on the base map with the cells `surveyed` written as apriori"""
    scene = te.Scene([[te.Shape("cells", np.unique(c, axis=0), "none", None, False)] for c in frames])
    bench.load(scene)
    if len(surveyed):
        bench.map0[surveyed[:, 2], surveyed[:, 1], surveyed[:, 0]] = np.float32(np.inf)
        bench.reset_maps()
    bench.scans = [ce.cells_scan(bench.world(c), bench.t) for c in frames]


def _small(k):
    return np.vstack([s.cells for s in ce.small_frame(k)])


def _view_cells(bench, g):
    """(cells of the voxels in far clusters, cells of the others) of a frame's debug view of the oracle"""
    cl = g["clusters"]
    far = np.isin(g["labels"], cl["first_member"][cl["is_close"] == 0])
    cell = st.map_cells(g["weighted"], bench.off.astype(np.float32), VS)
    return cell[far], cell[~far]


def _as_set(cells):
    return set(map(tuple, np.asarray(cells, dtype=np.int64).reshape(-1, 3).tolist()))


def _no_ids(a):
    a = a.copy()
    a["id"] = 0  # (the ids count on from call to call)
    return a


def _three_way(bench, monkeypatch, min_dets0=1):
    """(a) = (b) bit for bit, both the oracle's; returns the oracle's debug views"""
    dev, scans, tfs = bench.dev, bench.scans, bench.tfs
    da, pa, ga = bench.ref.process_batch(scans, tfs, debug=True)
    assert int(pa[0]) >= min_dets0, pa.tolist()  # (the oracle's own output: there are detections whose records can go wrong)
    exp = [dpc.expected_frame(g) for g in ga]
    got = []
    for sw in (None, "0"):
        if sw is not None:
            monkeypatch.setenv("VOFOD_LEAN_RANKS", sw)
        try:
            db, pb = _production(dev, scans, tfs)
            if not SELFCHECK:  # (oracle against oracle: the oracle has no vofod_detection_points)
                ext, pts, idx = dev.detection_points()
        finally:
            if sw is not None:
                monkeypatch.delenv("VOFOD_LEAN_RANKS")
        _assert_same((da, pa), (db, pb))
        if SELFCHECK:
            got.append((_no_ids(db), pb))
            continue
        dpc.assert_points(ext, pts, idx, db, exp)
        got.append((_no_ids(db), pb, _no_ids(ext), pts, idx))
    for x, y, k in zip(got[0], got[1], ("detections", "per frame", "extents", "points", "index")):
        assert x.tobytes() == y.tobytes(), k
    return ga


def _assert_row(bench, g, target, n_before, n_behind, by=BY, bz=BZ):
    """from the view: the target's voxels are far, its brick is node `n_before` of a brick row whose other bricks hold close voxels"""
    far, other = _view_cells(bench, g)
    assert _as_set(target) <= _as_set(far), "the target is not a far cluster"
    tb = np.unique(_bricks(bench, target), axis=0)
    assert len(tb) == 1 and tuple(tb[0][1:]) == (by, bz), tb
    ob = np.unique(_bricks(bench, other), axis=0)
    row = ob[(ob[:, 1] == by) & (ob[:, 2] == bz)][:, 0]
    fb = np.unique(_bricks(bench, far), axis=0)
    assert len(fb[(fb[:, 1] == by) & (fb[:, 2] == bz)]) == 1, "another pure-far brick in the row"
    assert int((row < tb[0][0]).sum()) == n_before and int((row > tb[0][0]).sum()) == n_behind, (row.tolist(), tb.tolist())


def _row_case(bench, n_before, n_behind, hits=1):
    """frame 0: `n_before` surveyed bricks, a gap, a pair along x inside one brick, a gap, `n_behind` surveyed bricks, all in one brick
    row; frame 1: the surveyed bricks alone (no pure-far brick at all); frames 2, 3: small frames with thirty pure-far bricks"""
    tbx = TBX
    before = list(range(tbx - GAP - n_before, tbx - GAP))
    behind = list(range(tbx + GAP + 1, tbx + GAP + 1 + n_behind))
    wall = _wall(bench, before + behind)
    target = _cells(bench, (tbx, BY, BZ), [(1, 1, 1), (2, 1, 1)])
    f0 = np.vstack([wall, np.repeat(target[:1], hits, axis=0), target[1:]])
    _load(bench, [f0, wall, _small(2), _small(3)], wall)
    return target


# (first, middle, last node of the row; the walk's 16-node steps: the nodes in front and behind fill a step exactly, or one more;
#  more than 64 bricks in the row with the target before, at and behind node 64)
ROWS = [(0, 9), (9, 9), (9, 0), (15, 15), (16, 16), (17, 15), (63, 8), (64, 8), (65, 8)]


@pytest.mark.parametrize("n_before,n_behind", ROWS)
def test_a_far_cluster_in_a_row_of_known_bricks(bench, monkeypatch, n_before, n_behind):
    """a long, thin, surveyed structure along x with a gap, and a new target in the gap: the target's pure-far brick shares its brick
    row with `n_before` map-known bricks in front of it and `n_behind` behind it; frame 1 of the batch has no pure-far brick at all"""
    target = _row_case(bench, n_before, n_behind)
    ga = _three_way(bench, monkeypatch)
    _assert_row(bench, ga[0], target, n_before, n_behind)
    far1, other1 = _view_cells(bench, ga[1])
    assert len(far1) == 0 and len(other1) == n_before + n_behind  # (s_npf == 0 beside frames that have a list)
    assert len(_view_cells(bench, ga[2])[0]) >= 30


def test_more_than_255_points_in_a_pure_far_voxel(bench, monkeypatch):
    """300 returns in the first voxel of the target (the construction of test_gpu_lean_emit.py::test_counters_beyond_255): the extras
    pass finds the voxel's rank through the same tables"""
    target = _row_case(bench, 9, 9, hits=300)
    ga = _three_way(bench, monkeypatch)
    _assert_row(bench, ga[0], target, 9, 9)
    w = ga[0]["weighted"]
    heavy = st.map_cells(w, bench.off.astype(np.float32), VS)[w["range"] >= 300]
    assert _as_set(heavy) == _as_set(target[:1]), heavy
    gb = bench.dev.process_batch(bench.scans, bench.tfs, debug=True, far_only=True)[2]
    _assert_far_views(ga, gb)  # (the full emission behind the lean launches: the weight of 300 bit for bit)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_two_pure_far_bricks_of_one_cluster(bench, monkeypatch, axis):
    """a pair that straddles two bricks: adjacent along x (two list entries of one brick row share its totals), y (rows of adjacent
    by) or z (adjacent slabs: row bases and slab constants), in the gap of a surveyed row"""
    before, behind = list(range(BX0, BX0 + 9)), list(range(BX0 + 9 + 2 * GAP + 2, BX0 + 9 + 2 * GAP + 11))
    wall = np.vstack([_wall(bench, before + behind, BY + d, BZ + e) for d in (0, 1) for e in (0, 1)])
    inb = np.array([(1, 1, 1), (1, 1, 1)])
    inb[0, axis], inb[1, axis] = 3, 4
    target = _cells(bench, (BX0 + 9 + GAP, BY, BZ), inb)
    _load(bench, [np.vstack([wall, target]), _small(1), _small(2), _small(3)], wall)
    ga = _three_way(bench, monkeypatch)
    far, other = _view_cells(bench, ga[0])
    assert _as_set(far) == _as_set(target) and len(other) == len(wall)
    tb = _bricks(bench, target)
    assert (tb[1] - tb[0]).tolist() == [int(a == axis) for a in range(3)], tb
    cl = ga[0]["clusters"]
    assert int((cl["is_close"] == 0).sum()) == 1  # one far cluster of two bricks


def test_an_empty_slab_between_occupied_ones(bench, monkeypatch):
    """frame 0: the surveyed row with its target in slab BZ, nothing in the three slabs above, a second row with a target in slab
    BZ + 4 (no frame of the recipe has a brick in slab 0: the first occupied slab is BZ)"""
    lo = _cells(bench, (BX0 + 9 + GAP, BY, BZ), [(1, 1, 1), (2, 1, 1)])
    before, behind = list(range(BX0, BX0 + 5)), list(range(BX0 + 5 + 2 * GAP + 1, BX0 + 5 + 2 * GAP + 6))
    wall_hi = _wall(bench, before + behind, BY + 2, BZ + 4)
    hi = _cells(bench, (BX0 + 5 + GAP, BY + 2, BZ + 4), [(1, 2, 3), (1, 3, 3)])
    wall = np.vstack([_wall(bench, list(range(BX0, BX0 + 9)) + list(range(BX0 + 9 + 2 * GAP + 1, BX0 + 9 + 2 * GAP + 10))), wall_hi])
    _load(bench, [np.vstack([wall, lo, hi]), _small(1), wall, _small(3)], wall)
    ga = _three_way(bench, monkeypatch, min_dets0=2)
    far, other = _view_cells(bench, ga[0])
    assert _as_set(far) == _as_set(np.vstack([lo, hi])) and len(other) == len(wall)
    slabs = np.unique(_bricks(bench, np.vstack([far, other]))[:, 2]).tolist()
    assert slabs == [BZ, BZ + 4], slabs


@pytest.mark.parametrize("over", [0, 1])
def test_a_list_at_the_threshold(bench, monkeypatch, over):
    """B(FR_LEAN_RANKS_MAX + over) of close_first_edges.py in frame 0: exactly as many pure-far bricks as the per-entry walk takes,
    and one more (that frame takes the frame-wide passes, the other three frames of the batch the walk): the same answers"""
    P = _threshold() + over
    scene = ce.batch(P, 0)
    bench.load(scene)
    ga = _three_way(bench, monkeypatch, min_dets0=3)
    cells0 = np.vstack([s.cells for s in scene.frames[0]])
    far, other = _view_cells(bench, ga[0])
    assert len(far) + len(other) == len(cells0)
    m = bench.map0
    thr = np.float32(bench.dev.dp.voxel_map__thresholds__new_obstacles)
    assert ce.pure_far_bricks(cells0, ce.far_by_itself(m, thr, cells0), bench.dev.map_offset, bench.dev.sp) == P == scene.claims["pure_far_bricks"]


def test_stale_tables_of_other_frames(bench, monkeypatch):
    """the far-only debug view of OTHER frames first - a full emission: it leaves complete, plausible nodeA / rowT / rowQ in every
    slot of the handle's scratch -, then the lean batch, whose walk writes the list's entries only"""
    bench.load(ce.batch(200, 1))
    other = list(bench.scans)
    target = _row_case(bench, 17, 15)
    bench.dev.process_batch(other, bench.tfs, debug=True, far_only=True)
    ga = _three_way(bench, monkeypatch)
    _assert_row(bench, ga[0], target, 17, 15)
