"""Hand-placed scenes for tests/test_gpu_close_first_edges.py: a scan or a frame that holds exactly as many far voxels (FAR_MAX,
kernels_far.h) or pure-far bricks (CF_MAX, kernels_frame.h) as a close-first path takes, one less, or one more.  The recipe is the one
of tests/tail_edges.py: OS1-16, 0.25 m voxels, the default operation area, an apriori background sheet in map layer 8 (both latches),
every other voxel free air, the returns of a scan are the centres of chosen map cells (cells_scan).  Everything here is host
arithmetic on map cells; the numbers a scene claims (`claims`) follow from the placed cells alone and are checked against a numpy
statement of "far by itself" and the oracle's debug view by tests/test_close_first_edges_cpu.py.

Single-scan scenes S(K, filler), K far-by-themselves voxels:
  close    five voxels 1 .. 5 layers above the sheet and an anchor 6 layers above it (hasCloseTo's truncated norm: 6 <= 6.0);
  chain    204 far voxels, a snake of five rows 7 layers apart joined at their ends, each voxel within the tolerance of the next; its
           lowest voxel lies 2 cells above the anchor: the whole component is a close cluster (scores/point, flag 2);
  cand     five floating clusters (pairs along x, y, z, a 2 x 2 x 2 cube, an L triple), 16 cells apart: the detections;
  filler   `block`: one dense box 16 x 16 cells wide (3.75 m: the extent prefilter rejects it) - or `singles`: single voxels on a grid
           of 7 cells (49 >= 36: none join), thousands of components below min_points.
Batch scenes B(P), P pure-far bricks (4 x 4 x 4 cells of the reference lattice) in one frame of four:
  filler   one voxel per brick, bricks two apart along every axis; along x the voxels sit at brick cells 3 and 1 in turn, so that every
           one of them has a neighbour at exactly 6 cells (36 < 36 is false: no edge) - a pair the octant matrices leave open, for the
           exact test of the open-pair list, whichever list index the brick got;
  close    four bricks that hold a voxel 4 layers above the sheet;
  taint    three voxels in three pure-far bricks above the anchor, 4 cells apart: enough voxels for a candidate, but a close cluster;
  cand     a pair inside one brick, an L triple that straddles two adjacent bricks, a pair 5 cells apart in bricks two apart (joined
           by the exact test); the other frames hold thirty singles, two close voxels and one pair each."""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

import frame_geometry as fg
import statements as st
import tail_edges as te
from vofod_amd.detector import ScanData

VS = te.VS
ROOT = Path(__file__).resolve().parent.parent
TOL_CELLS = 6  # ground_points_max_distance 1.5 m / 0.25 m: the clustering tolerance and hasCloseTo's reach


def cells_scan(pts_world, t, w=1024, h=16):
    """a scan whose returns are the given world points, seen from a sensor at `t` (pose = pure translation)"""
    n = w * h
    p = np.asarray(pts_world, dtype=np.float64) - np.asarray(t, dtype=np.float64)
    assert len(p) <= n
    cols = [np.zeros(n, dtype=np.float32) for _ in range(3)]  # (0,0,0) = no return: dropped by the exclude box
    for a in range(3):
        cols[a][: len(p)] = p[:, a]
    return ScanData(x=cols[0], y=cols[1], z=cols[2], width=w, height=h, stride_bytes=4)


def capacities():
    """the capacities of the close-first paths and of the device tail, read from the kernel headers: a change there moves the scenes
    with it or fails here"""
    csrc = ROOT / "vofod_amd" / "csrc"
    src = "".join((csrc / n).read_text() for n in ("kernels_far.h", "kernels_frame.h", "common.h"))
    out = {}
    for name in ("FAR_MAX", "FR_THREADS", "TAIL_MAXC", "TAIL_MAXM"):
        m = re.search(r"constexpr\s+(?:int|uint32_t)\s+" + name + r"\s*=\s*(\d+)\s*;", src)
        assert m, name
        out[name] = int(m.group(1))
    assert re.search(r"constexpr\s+int\s+CF_MAX\s*=\s*FR_THREADS\s*;", src), "CF_MAX"
    out["CF_MAX"] = out["FR_THREADS"]
    assert re.search(r"constexpr\s+int\s+PT\s*=\s*FAR_MAX\s*/\s*1024\s*;", src), "k_far_final: slots per thread"
    return out


@dataclass
class EdgeScene(te.Scene):
    claims: dict = field(default_factory=dict)  # what the placed cells say: see single_scan / batch
    edge_frame: int = 0                          # the frame at the edge


def _shape(name, cells, cand=False, det=False):
    return te.Shape(name, np.asarray(cells, dtype=np.int64).reshape(-1, 3), "none", det, cand)


def role(shape):
    return shape.name.split(" ", 1)[0]


def cells_of(frame, *roles):
    sel = [s.cells for s in frame if role(s) in roles]
    return np.vstack(sel) if sel else np.zeros((0, 3), dtype=np.int64)


# ----------------------------------------------------------------------------------------------- numpy statements of a frame
def far_by_itself(m, thr, cells):
    """a voxel is far by itself when no map voxel above `thr` lies inside hasCloseTo's stencil (statements.close_at)"""
    return ~st.close_at(m, thr, np.float32(TOL_CELLS * VS), VS, cells)


def brick_of(cells, map_offset, sp):
    """brick (4 x 4 x 4 cells of the reference lattice, frame_geometry.ref_lattice) of map cells"""
    lat = fg.ref_lattice(list(sp.oparea_offset), list(sp.oparea_size), float(sp.voxel_size))
    shift = np.round((np.asarray(map_offset, dtype=np.float64) - lat["off"].astype(np.float64)) / float(sp.voxel_size)).astype(np.int64)
    return (np.asarray(cells, dtype=np.int64) + shift) // 4


def pure_far_bricks(cells, far, map_offset, sp):
    """number of bricks that hold voxels of the frame and no close one"""
    b = brick_of(cells, map_offset, sp)
    key = (b[:, 2] * 4096 + b[:, 1]) * 4096 + b[:, 0]
    return len(np.setdiff1d(np.unique(key), np.unique(key[~far])))


# ------------------------------------------------------------------------------------------------------------ single scans
CAND_SHAPES = [("pair x", te.PAIRS["pair x"]), ("pair y", te.PAIRS["pair y"]), ("2x2x2 cube", te.block(2, 2, 2)), ("L triple", te.L_TRIPLE), ("pair z", te.PAIRS["pair z"])]


def _specials():
    """close voxels, the tainted chain and the five candidates of a single-scan scene, in map x >= 320 (the filler stays below 300)"""
    L = te.SHEET_LAYER
    close = [(330, 60 + 20 * j, L + 1 + j) for j in range(5)]
    anchor = (380, 60, L + TOL_CELLS)
    chain = []
    for r in range(5):  # rows at layers 16, 23, 30, 37, 44; 40 voxels 5 cells apart along y; a connector 4 layers above each row's end
        ys = [60 + 5 * i for i in range(40)]
        if r % 2:
            ys.reverse()
        chain += [(380, y, L + 8 + 7 * r) for y in ys]
        if r < 4:
            chain.append((380, ys[-1], L + 8 + 7 * r + 4))
    chain = np.array(chain, dtype=np.int64)
    step = np.diff(chain, axis=0)
    assert ((step * step).sum(1) < TOL_CELLS**2).all() and chain[:, 2].min() == chain[0, 2] == anchor[2] + 2
    shapes = [_shape(f"close {j}", c) for j, c in enumerate(close)] + [_shape("close anchor", anchor), _shape("chain", chain)]
    for j, (n, rel) in enumerate(CAND_SHAPES):
        shapes.append(_shape("cand " + n, np.asarray(rel) + (325 + 16 * j, 320, 40), cand=True, det=True))
    return shapes


def single_scan(K, filler, min_points=None):
    """S(K, filler): K far-by-themselves voxels in one scan"""
    shapes = _specials()
    n_special = sum(len(s.cells) for s in shapes if role(s) in ("chain", "cand"))
    R = K - n_special
    assert R > 3000
    if filler == "block":
        cells = (te.block(R // 256 + 1, 16, 16)[:, ::-1] + (100, 100, 40))[:R]  # x fastest: full layers of 16 x 16 and a partial one on top
        shapes.append(_shape("filler block", cells))
        n_comp = 1
    else:
        gx, gy, gz = np.meshgrid(np.arange(299, 39, -7), np.arange(40, 360, 7), np.arange(16, 94, 7), indexing="ij")  # (from the sensor's side outwards: within classification__max_distance)
        cells = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)[:R]
        assert len(cells) == R
        shapes += [_shape(f"filler single {i}", c) for i, c in enumerate(cells)]
        n_comp = R
    cands = [s for s in shapes if s.cand]
    mp = 2 if min_points is None else min_points
    singles_are_cands = filler == "singles" and mp <= 1
    if singles_are_cands:
        for s in shapes:
            if role(s) == "filler":
                s.cand, s.det = True, None  # (beyond classification__max_distance or not: the oracle decides)
    claims = dict(n_far=K, far_clusters=len(cands) + n_comp, close_clusters=6, cand_clusters=len(cands) + (R if singles_are_cands else 0),
                  cand_members=sum(len(s.cells) for s in cands) + (R if singles_are_cands else 0), detections=None if singles_are_cands else len(cands))
    return EdgeScene([shapes], dyn={} if min_points is None else dict(classification__min_points=min_points), claims=claims, scan_frames=(0,))


# ----------------------------------------------------------------------------------------------------------------- batches
def _batch_specials():
    L = te.SHEET_LAYER
    shapes = [_shape(f"close {j}", (330 + 20 * j, 100, L + 4)) for j in range(4)]
    shapes += [_shape("close anchor", (380, 60, L + TOL_CELLS)), _shape("taint", [(380, 60, L + 8), (380, 60, L + 12), (380, 60, L + 16)])]
    shapes.append(_shape("cand pair in a brick", [(328, 320, 40), (329, 320, 40)], cand=True, det=True))
    shapes.append(_shape("cand L triple across bricks", [(347, 320, 40), (348, 320, 40), (347, 321, 40)], cand=True, det=True))
    shapes.append(_shape("cand pair two bricks apart", [(363, 320, 40), (368, 320, 40)], cand=True, det=True))
    return shapes


def _filler_bricks(n, skip=0):
    """one voxel in each of n bricks two apart; along x the voxels sit at brick cells 3, 1, 3, 1 ...: 6 and 10 cells apart in turn"""
    bz, by, bx = np.meshgrid(np.arange(6, 24, 2), np.arange(10, 90, 2), np.arange(12, 72, 2), indexing="ij")  # x fastest: whole rows of 15 such pairs
    b = np.stack([bx.ravel(), by.ravel(), bz.ravel()], axis=1)[skip : skip + n]
    assert len(b) == n
    lx = np.where((b[:, 0] // 2) % 2 == 0, 3, 1)
    return b * 4 + np.stack([lx, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)], axis=1)


def small_frame(k):
    """thirty singles in bricks of their own, two close voxels and one pair, shifted from frame to frame"""
    L = te.SHEET_LAYER
    shapes = [_shape(f"filler single {i}", c) for i, c in enumerate(_filler_bricks(30, skip=3000 + 40 * k))]
    shapes += [_shape(f"close {j}", (330 + 20 * j + k, 140 + 3 * k, L + 3)) for j in range(2)]
    shapes.append(_shape("cand pair", np.asarray(te.PAIRS[te.FLAT_PAIRS[k % 6]]) + (330 + 5 * k, 280 + 4 * k, 44), cand=True, det=True))
    return shapes


def _n_special_bricks(shapes):
    cells = np.vstack([s.cells for s in shapes if role(s) in ("taint", "cand")])
    return len(np.unique(cells // 4, axis=0))  # (the default area's reference lattice starts at the map's corner: test_close_first_edges_cpu checks it through brick_of)


def batch(P, edge_frame=0):
    """B(P): P pure-far bricks in frame `edge_frame` of four"""
    big = _batch_specials()
    F = P - _n_special_bricks(big)
    big += [_shape(f"filler single {i}", c) for i, c in enumerate(_filler_bricks(F))]
    frames = [small_frame(k) for k in (1, 2, 3)]
    frames.insert(edge_frame, big)
    claims = dict(pure_far_bricks=P, far_clusters=3 + F, close_clusters=5, cand_clusters=3, cand_members=7, detections=[3 if f == edge_frame else 1 for f in range(4)],
                  small_pure_far_bricks=30 + 1)
    return EdgeScene(frames, claims=claims, edge_frame=edge_frame, scan_frames=())


def background_corner(n, map_size):
    """n map cells in the far upper corner of the map (x >= 420, y >= 340, z >= 60): 100 cells and more from every voxel of a scene"""
    sx, sy, sz = map_size
    gz, gy, gx = np.meshgrid(np.arange(60, sz), np.arange(340, sy), np.arange(420, sx), indexing="ij")
    c = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)
    assert n <= len(c)
    return c[:n]
