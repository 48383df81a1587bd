"""Lean count of the close-first frame kernel (k_frame_lds<1, *>, kernels_frame.h, pass 3b): in a lean launch the codes of the pure-far
bricks are filtered into a per-frame list - a lane's runs of one listed code merged into one entry, a round's entries of a wave
reserved with one atomic - and the weights are counted from that list.  VOFOD_LEAN_COUNT=0 (read on every call) keeps the walk over
every code, as does a frame whose list would be longer than FR_LEAN_COUNT_MAX.

A wrong weight shows in the voxel records of a detection's members: vofod_detection_points returns them bit for bit (centre and
weight).  Every case compares (a) the production call - k_frame_lds_far, asserted from the profiler's kernel list
(vofod_profile_read) -, (b) the same batch under VOFOD_LEAN_COUNT=0 and (c) the oracle: detection records, per-frame counts and the
detections' points, bit for bit between (a) and (b), within the helpers' tolerances against the oracle (points, weights and indices:
bit for bit).  Which of the two routes a frame took inside the kernel is read from the kernel's own diagnostics (VOFOD_LDS_PROF_JSON,
"lean_count") in the cases that are about the route - under the default switches only, like the kernels' labels.

The recipe is the hand-placed one of tests/test_gpu_lean_ranks.py - 0.25 m, four frames, the returns of a scan are points in chosen
map cells, a target in the gap of a surveyed brick row, frame 1 the surveyed bricks alone (an EMPTY list in every batch) - on an
OS1-128 (131 072 pixels, a few thousand of them returns), because the cases are statements about where a code lies in a wave's code
list, and only a scan of seven input rounds and more gives a wave the 3 072 codes behind which the list is read from global memory.
The input pass deals the 512-point pieces of a round of 8 192 points to the 16 waves in turn - wave w takes piece (w + r) % 16 of
round r - and a wave appends the codes of its returns in point order; the passes 3a / 3b give lane l of the wave the codes
[1 024 k + 16 l, + 16) of round k.  `Layout` places points by (wave, position in the wave's list); positions in front of a placed
point are filled with returns from surveyed bricks - codes of bricks that are not listed."""
import json
import re

import numpy as np
import pytest

import close_first_edges as ce
import detection_points_cases as dpc
import frame_geometry as fg
import statements as st
import tail_edges as te
import test_gpu_tail_edges as tge
from test_gpu_lean_emit import ROUTE_CHECKED, SELFCHECK, _assert_same, _production
from test_gpu_lean_ranks import BY, BZ, GAP, TBX, _as_set, _assert_row, _cells, _no_ids, _small, _view_cells, _wall
from vofod_amd.detector import ScanData

pytestmark = pytest.mark.gpu

VS = te.VS
W, H = 1024, 128                     # OS1-128
PIECE, ROUND, WAVES = 512, 8192, 16  # the input pass: points per piece and per round, waves (kernels_frame.h: IN_PPT * 64, IN_ROUND)
KPT, REG_CODES = 16, 3072            # codes per lane and round of the passes 3a / 3b; codes of a wave that stay in registers (FR_REG_ROUNDS)


def _cap():
    src = (ce.ROOT / "vofod_amd" / "csrc" / "kernels_frame.h").read_text()
    m = re.search(r"#define\s+FR_LEAN_COUNT_MAX_DEF\s+(\d+)", src)
    assert m and re.search(r"FR_LEAN_COUNT_MAX\s*=\s*FR_LEAN_COUNT_MAX_DEF\s*;", src)
    for name, val in (("IN_PPT", 8), ("FR_THREADS", 1024), ("FR_REG_ROUNDS_DEF", 3)):  # (what Layout's arithmetic assumes)
        assert re.search(r"(?:constexpr\s+int|#define)\s+" + name + r"\s*=?\s*" + str(val) + r"\b", src), name
    return int(m.group(1))


class BigBench(tge.Bench):
    """the pair of tests/test_gpu_tail_edges.py with an OS1-128's pixels"""

    def __init__(self, oracle, hip):
        orig = tge.make_pair
        tge.make_pair = lambda o, h, sensor, vs, **kw: orig(o, h, "os1-128", vs, **kw)
        try:
            super().__init__(oracle, hip)
        finally:
            tge.make_pair = orig


@pytest.fixture(scope="module")
def bench(oracle, hip):
    b = BigBench(oracle, hip)
    lat = fg.ref_lattice(list(b.dev.sp.oparea_offset), list(b.dev.sp.oparea_size), float(b.dev.sp.voxel_size))
    b.shift = np.round((np.asarray(b.dev.map_offset, dtype=np.float64) - lat["off"].astype(np.float64)) / VS).astype(np.int64)
    b.eps = float(lat["eps"])
    yield b
    b.close()


class Layout:
    """the pixels of one scan: world points at chosen places of the waves' code lists, the rest no return"""

    def __init__(self, bench, filler):
        self.bench = bench
        self.filler = np.asarray(filler, dtype=np.int64).reshape(-1, 3)  # map cells of surveyed bricks
        self.p = np.full((W * H, 3), np.nan)
        self.fill = [0] * WAVES  # positions of the wave's list that are taken
        self.k = 0

    @staticmethod
    def pixel(wave, pos):
        r = pos // PIECE
        return r * ROUND + ((wave + r) % WAVES) * PIECE + pos % PIECE

    def at(self, wave, pos, cells, frac=(0.5, 0.5, 0.5)):
        """the points `cells` (one return each, in this order) from position `pos` of wave `wave`'s list on; returns the position behind"""
        assert pos >= self.fill[wave], (wave, pos, self.fill[wave])
        while self.fill[wave] < pos:  # returns of surveyed bricks in front: every position of the list is a code
            self._put(wave, self.filler[self.k % len(self.filler)], (0.5, 0.5, 0.5))
            self.k += 1
        for c in np.asarray(cells, dtype=np.int64).reshape(-1, 3):
            self._put(wave, c, frac)
        return self.fill[wave]

    def _put(self, wave, cell, frac):
        px = self.pixel(wave, self.fill[wave])
        assert px < W * H
        self.p[px] = self.bench.off + (np.asarray(cell, dtype=np.float64) + np.asarray(frac, dtype=np.float64)) * VS
        self.fill[wave] += 1

    def scan(self):
        q = np.where(np.isnan(self.p), 0.0, self.p - np.asarray(self.bench.t, dtype=np.float64))  # (0, 0, 0): no return
        cols = [np.ascontiguousarray(q[:, a], dtype=np.float32) for a in range(3)]
        return ScanData(x=cols[0], y=cols[1], z=cols[2], width=W, height=H, stride_bytes=4)

    def cells(self):
        live = ~np.isnan(self.p[:, 0])
        return np.floor((self.p[live] - self.bench.off) / VS).astype(np.int64)


def _row(bench):
    """the surveyed bricks of the cases' brick row - nine in front of the target's brick, nine behind, a gap on either side - and the
    target's brick"""
    bxs = list(range(TBX - GAP - 9, TBX - GAP)) + list(range(TBX + GAP + 1, TBX + GAP + 10))
    return _wall(bench, bxs), (TBX, BY, BZ)


def _plain(bench, cells):
    """a frame whose returns are the given cells, one after the other from the first pixel on"""
    lay = Layout(bench, cells)
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    for w0 in range(0, len(c), PIECE):
        lay.at((w0 // PIECE) % WAVES, (w0 // ROUND) * PIECE, c[w0 : w0 + PIECE])
    return lay


def _load(bench, layouts, surveyed):
    """four scans on the base map with the cells `surveyed` written as apriori"""
    scene = te.Scene([[te.Shape("cells", np.unique(l.cells(), axis=0), "none", None, False)] for l in layouts])
    bench.load(scene)
    if len(surveyed):
        bench.map0[surveyed[:, 2], surveyed[:, 1], surveyed[:, 0]] = np.float32(np.inf)
        bench.reset_maps()
    bench.scans = [l.scan() for l in layouts]


def _batch(bench, lay0):
    """frame 0: the case; frame 1: the surveyed bricks alone - no pure-far brick, an empty list; frames 2, 3: thirty pure-far bricks"""
    wall, _ = _row(bench)
    lay0.at(8, lay0.fill[8], wall)  # (every surveyed brick of the row at least once in frame 0 - behind the list of a wave no case places points in)
    _load(bench, [lay0, _plain(bench, wall), _plain(bench, _small(2)), _plain(bench, _small(3))], wall)


def _routes(path):
    """per launch of the profiled call: (frames that counted from the list, frames that walked every code, the longest list, the entries
    of all lists, most counters of a frame)"""
    rows = [json.loads(l) for l in open(path) if l.strip()]
    return [(r["lean_count"]["from_list"], r["lean_count"]["walked"], int(r["lean_count"]["entries"]["max"]), round(r["lean_count"]["entries"]["mean"] * r["frames"]),
             int(r["lean_count"]["counters"]["max"])) for r in rows]


def _three_way(bench, monkeypatch, min_dets0=1, prof=None, frame1_empty=True):
    """(a) = (b) bit for bit, both the oracle's; returns the oracle's debug views.  `prof`: a file that receives the kernel's own
    account of launch (a) (under the default switches: ROUTE_CHECKED)"""
    dev, scans, tfs = bench.dev, bench.scans, bench.tfs
    da, pa, ga = bench.ref.process_batch(scans, tfs, debug=True)
    assert int(pa[0]) >= min_dets0, pa.tolist()  # (the oracle's own output: there are detections whose records can go wrong)
    exp = [dpc.expected_frame(g) for g in ga]
    got = []
    for sw in (None, "0"):
        env = {} if sw is None else {"VOFOD_LEAN_COUNT": sw}
        if sw is None and prof is not None and ROUTE_CHECKED:
            env.update(VOFOD_LDS_PROF="1", VOFOD_LDS_PROF_JSON=str(prof))
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            db, pb = _production(dev, scans, tfs)
            if not SELFCHECK:  # (oracle against oracle: the oracle has no vofod_detection_points)
                ext, pts, idx = dev.detection_points()
        finally:
            for k in env:
                monkeypatch.delenv(k)
        _assert_same((da, pa), (db, pb))
        if SELFCHECK:
            got.append((_no_ids(db), pb))
            continue
        dpc.assert_points(ext, pts, idx, db, exp)
        got.append((_no_ids(db), pb, _no_ids(ext), pts, idx))
    for x, y, k in zip(got[0], got[1], ("detections", "per frame", "extents", "points", "index")):
        assert x.tobytes() == y.tobytes(), k
    if frame1_empty:
        far1, other1 = _view_cells(bench, ga[1])
        assert len(far1) == 0 and len(other1) > 0  # (the empty list beside frames that have one)
    return ga


def _weights(bench, g, cells):
    """the oracle's weights of the given cells in a frame's view"""
    w = g["weighted"]
    cell = {tuple(c): float(r) for c, r in zip(np.asarray(st.map_cells(w, bench.off.astype(np.float32), VS)).tolist(), w["range"])}
    return [cell[tuple(c)] for c in np.asarray(cells, dtype=np.int64).reshape(-1, 3).tolist()]


def _listed_points(bench, g, lay):
    """returns of the layout that lie in voxels of far clusters (the cases hold no pure-far brick of a close cluster: the list's codes)"""
    far = _as_set(_view_cells(bench, g)[0])
    return sum(tuple(c) in far for c in lay.cells().tolist())


# ------------------------------------------------------------------------------------------------------------------- the cases
def _heavy(bench, spread):
    """300 returns in the first voxel of the target, one in the second"""
    wall, tb = _row(bench)
    a, b = _cells(bench, tb, [(1, 1, 1), (2, 1, 1)])
    lay = Layout(bench, wall)
    if spread == "full lanes":      # 18 lanes of wave 0 hold 16 each, one holds 12: entries of 16 points - the 16th entry finds the byte at 240
        lay.at(0, lay.at(0, 0, [a] * 300), [b])
    elif spread == "single codes":  # a and b in turn: every return an entry of its own, 8 of a per lane, 38 lanes of wave 0 (two pieces: two rounds of input)
        lay.at(0, 0, [a, b] * 300)
    else:                           # 75 at the head of the lists of four waves
        for w in (0, 5, 10, 15):
            lay.at(w, 0, [a] * 75 + [b])
    return lay, a, b


@pytest.mark.parametrize("spread", ["full lanes", "single codes", "four waves"])
def test_more_than_255_points_in_a_pure_far_voxel(bench, monkeypatch, spread, tmp_path):
    """the byte counter stops at 255 and the rest leaves as extras records with their point counts, whether the points arrive as a few
    entries of 16 (a lane holds 16 codes of a round: no more can lie in one lane), as 300 entries of one point in the lanes of one
    wave, or from four waves at once"""
    lay, a, b = _heavy(bench, spread)
    _batch(bench, lay)
    prof = tmp_path / "prof.jsonl"
    ga = _three_way(bench, monkeypatch, prof=prof)
    _assert_row(bench, ga[0], np.vstack([a, b]), 9, 9)
    n_b = 300 if spread == "single codes" else 4 if spread == "four waves" else 1
    assert _weights(bench, ga[0], [a, b]) == [300.0, float(n_b)]
    if ROUTE_CHECKED:
        (from_list, walked, longest, entries, counters), = _routes(prof)
        assert (from_list, walked) == (4, 0)
        want = {"full lanes": 19 + 1, "single codes": 600, "four waves": 4 * (5 + 1)}[spread]  # (lanes of 16: 75 = 4 x 16 + 11)
        assert entries == want + _listed_points(bench, ga[2], _plain(bench, _small(2))) + _listed_points(bench, ga[3], _plain(bench, _small(3))) and counters >= 2


def test_equal_codes_across_lane_and_round_boundaries(bench, monkeypatch):
    """eight returns of one voxel in the last four codes of lane 0 and the first four of lane 1; eight of a second voxel in the last four
    codes of round 0 (lane 63) and the first four of round 1 (lane 0); eight of a third that begin in the last lane of the wave's first
    piece of input: two entries each, neither merged with the other nor lost"""
    wall, tb = _row(bench)
    a, b, c = _cells(bench, tb, [(1, 1, 1), (2, 1, 1), (1, 2, 1)])
    lay = Layout(bench, wall)
    lay.at(0, KPT - 4, [a] * 8)
    lay.at(0, PIECE - 4, [c] * 8)
    lay.at(0, 64 * KPT - 4, [b] * 8)
    _batch(bench, lay)
    ga = _three_way(bench, monkeypatch)
    _assert_row(bench, ga[0], np.vstack([a, b, c]), 9, 9)
    assert _weights(bench, ga[0], [a, b, c]) == [8.0, 8.0, 8.0]


def test_fragile_points_inside_a_pure_far_brick(bench, monkeypatch):
    """returns half an eps from a cell boundary - the input pass keeps them aside as fragile points, their codes come from the side list -
    in a voxel that also holds solid returns, and in a voxel that holds nothing else"""
    wall, tb = _row(bench)
    a, b, c = _cells(bench, tb, [(1, 1, 1), (2, 1, 1), (1, 2, 1)])
    assert 1e-4 < bench.eps < 0.05
    lo, hi = 0.5 * bench.eps, 1.0 - 0.5 * bench.eps
    lay = Layout(bench, wall)
    p = lay.at(0, 0, [a] * 3 + [b])
    p = lay.at(0, p, [a] * 4, frac=(hi, 0.5, 0.5))
    p = lay.at(0, p, [b] * 2, frac=(0.5, lo, 0.5))
    p = lay.at(0, p, [c] * 2, frac=(0.5, 0.5, hi))
    lay.at(3, 0, [c], frac=(lo, lo, lo))
    _batch(bench, lay)
    ga = _three_way(bench, monkeypatch)
    _assert_row(bench, ga[0], np.vstack([a, b, c]), 9, 9)
    assert _weights(bench, ga[0], [a, b, c]) == [7.0, 3.0, 3.0]


def test_a_wave_with_more_than_3072_codes(bench, monkeypatch):
    """wave 0 holds 4 000 codes (eight pieces of input): the rounds behind the third are read from the code list in global memory.  Returns
    of the target's voxels lie in the register rounds, across the boundary between the two kinds of rounds, and in the global rounds"""
    wall, tb = _row(bench)
    a, b, c = _cells(bench, tb, [(1, 1, 1), (2, 1, 1), (1, 2, 1)])
    lay = Layout(bench, wall)
    lay.at(0, 100, [a] * 5)
    lay.at(0, REG_CODES - 4, [b] * 8)
    lay.at(0, REG_CODES + 200, [a] * 20 + [c] * 3)
    lay.at(0, 3990, [c] * 10)
    assert lay.fill[0] == 4000
    _batch(bench, lay)
    ga = _three_way(bench, monkeypatch)
    _assert_row(bench, ga[0], np.vstack([a, b, c]), 9, 9)
    assert _weights(bench, ga[0], [a, b, c]) == [25.0, 8.0, 13.0]


@pytest.mark.parametrize("over", [0, 1])
def test_a_list_at_its_capacity(bench, monkeypatch, over, tmp_path):
    """FR_LEAN_COUNT_MAX + over returns in the target's two voxels in turn, from the first pixel on: every return an entry of its own,
    exactly as many entries as the list holds, and one more - that frame walks every code, the others of the batch count from their
    lists: the same weights"""
    cap = _cap()
    P = cap + over
    wall, tb = _row(bench)
    a, b = _cells(bench, tb, [(1, 1, 1), (2, 1, 1)])
    pts = np.vstack([a, b] * (P // 2 + 1))[:P]
    lay = _plain(bench, np.vstack([pts, wall]))
    _batch(bench, lay)
    prof = tmp_path / "prof.jsonl"
    ga = _three_way(bench, monkeypatch, min_dets0=1 if P >= 2 else 0, prof=prof)
    assert _weights(bench, ga[0], [a, b][: min(P, 2)]) == [float((P + 1) // 2), float(P // 2)][: min(P, 2)]
    if ROUTE_CHECKED:
        n = [P, 0, _listed_points(bench, ga[2], _plain(bench, _small(2))), _listed_points(bench, ga[3], _plain(bench, _small(3)))]
        (from_list, walked, longest, entries, counters), = _routes(prof)
        assert walked == sum(x > cap for x in n) and from_list == 4 - walked and longest == max(n) and entries == sum(n), (n, from_list, walked, longest, entries)
        assert walked == over or cap < max(n[2:])  # (the header's capacity: frame 0 alone is at the edge)


def test_a_frame_beyond_lean_ranks_max(bench, monkeypatch, tmp_path):
    """B(FR_LEAN_RANKS_MAX + 1) of close_first_edges.py in frame 0: that frame keeps the frame-wide rank passes - which use the rank
    tables' carries in LDS - and still counts from its list"""
    from test_gpu_lean_ranks import _threshold

    scene = ce.batch(_threshold() + 1, 0)
    lays = [_plain(bench, np.vstack([s.cells for s in f])) for f in scene.frames]
    _load(bench, lays, np.zeros((0, 3), dtype=np.int64))
    prof = tmp_path / "prof.jsonl"
    _three_way(bench, monkeypatch, min_dets0=3, prof=prof, frame1_empty=False)  # (frame 1 of this recipe is a small frame, not an empty one)
    if ROUTE_CHECKED:
        (from_list, walked, longest, entries, counters), = _routes(prof)
        assert (from_list, walked) == (4, 0) and longest >= _threshold() + 1


def test_stale_lists_and_counters_of_a_larger_launch(bench, monkeypatch):
    """a batch whose frame 0 fills the list to its capacity and a counter to 255 first - LDS keeps what a workgroup left -, then the small
    batch of the boundary case on the same handle: its frames zero the counters they use and read the entries they wrote, nothing else"""
    cap = _cap()
    wall, tb = _row(bench)
    a, b = _cells(bench, tb, [(1, 1, 1), (2, 1, 1)])
    big = _plain(bench, np.vstack([np.vstack([a, b] * (cap // 2 + 1))[:cap], wall]))
    _batch(bench, big)
    for _ in range(2):
        _production(bench.dev, bench.scans, bench.tfs)
    lay = Layout(bench, wall)
    lay.at(0, KPT - 4, [a] * 8)
    lay.at(0, 64 * KPT - 4, [b] * 8)
    _batch(bench, lay)
    ga = _three_way(bench, monkeypatch)
    _assert_row(bench, ga[0], np.vstack([a, b]), 9, 9)
    assert _weights(bench, ga[0], [a, b]) == [8.0, 8.0]
