"""The input pass of the frame kernel (k_frame_lds, kernels_frame.h, phase "in") compacts lane units: a lane's 8 consecutive points
are pushed into a 64-unit queue of the wave in LDS when the unit is live (it starts inside the cloud and - where the exclude box
holds the origin, so that exact zeros are dropped - one of its points is not +-0 in all three coordinates); the heavy part of
the pass runs on full queues and once more on the rest.  Nothing the kernel gives may change by it.

The frames here are scene scans (test_gpu_frame_inputs.scene_frames) with zero patterns punched into them, 16 x 1024 points:
two rounds of 16 pieces of 64 units.  Wave w takes piece w of round 0 and piece (w + 1) & 15 of round 1, so a frame is written
as 16 pairs of live-lane counts and the tests check on the host that the handed-over points really hold them.

Every comparison is HIP against the CPU oracle fed the same points as plain host columns, bit-exact, in the three views of
test_gpu_frame_inputs.three_views (full debug, far-only, production synchronous and as two tickets), which also asserts from the
profile that k_frame_lds_full* / k_frame_lds_far* ran - as packed columns and as 48-byte structs, the two input passes."""
import numpy as np
import pytest

from vofod_amd.detector import ScanData, VoFOD, default_params

from test_gpu_frame_inputs import DEFAULT_AREA, OS1_16, host_scan, lay_aos48, lay_columns, make_area_pair, scene_frames, survivors, three_views, warm_both

pytestmark = pytest.mark.gpu
f32 = np.float32
UNIT = 8  # points of a lane unit (IN_PPT)
PIECE = 64  # units of a piece: one per lane
WAVES = 16
LAYOUTS = {"columns": (lay_columns, "packed"), "aos48": (lay_aos48, "strided")}


class Frame:
    """what lay_* / host_scan read of a synth scan, over points of our own"""

    def __init__(self, x, y, z, tf, shape=OS1_16):
        self.x, self.y, self.z = (np.ascontiguousarray(v, dtype=f32) for v in (x, y, z))
        self.intensity = self.range = None
        self.tf = tf
        self.scan = ScanData(x=self.x, y=self.y, z=self.z, width=shape[1], height=shape[0], stride_bytes=4)


def nonzero_points(x, y, z):
    """the kernel's test: some coordinate is not +-0 (bit pattern without the sign)"""
    return ((x.view(np.uint32) | y.view(np.uint32) | z.view(np.uint32)) & np.uint32(0x7FFFFFFF)) != 0


def live_units(fr):
    nz = nonzero_points(fr.x, fr.y, fr.z)
    pad = (-nz.size) % UNIT
    return np.concatenate([nz, np.zeros(pad, dtype=bool)]).reshape(-1, UNIT).any(axis=1)


def wave_pairs(fr):
    """per wave: its live-lane counts in round 0 and round 1 (16 384 points)"""
    per_piece = live_units(fr).reshape(2, WAVES, PIECE).sum(axis=2)
    return [(int(per_piece[0, w]), int(per_piece[1, (w + 1) % WAVES])) for w in range(WAVES)]


def densified(s, only=None):
    """the scan with every point outside `only` (default: the points that are not zero) replaced by the last point inside it
    before it in scan order (the first ones: by the first inside): no zero is left, the cloud keeps its surfaces"""
    x, y, z = s.x.copy(), s.y.copy(), s.z.copy()
    ok = nonzero_points(x, y, z) if only is None else only
    assert ok.any()
    src = np.maximum.accumulate(np.where(ok, np.arange(ok.size), -1))
    src[src < 0] = np.flatnonzero(ok)[0]
    return x[src], y[src], z[src]


def punched(s, unit_mask, zero=0.0):
    """densified scan, the units outside `unit_mask` set to `zero` in all three coordinates"""
    x, y, z = densified(s)
    dead = ~np.repeat(np.asarray(unit_mask, dtype=bool), UNIT)[: x.size]
    x[dead] = y[dead] = z[dead] = f32(zero)
    return Frame(x, y, z, s.tf)


def mask_of_pairs(pairs, pick, rng):
    """unit mask of a 2 x 16 x 64 frame from the waves' (round 0, round 1) live-lane counts; pick: which lanes of a piece"""
    m = np.zeros((2, WAVES, PIECE), dtype=bool)
    for w, (c0, c1) in enumerate(pairs):
        for r, p, c in ((0, w, c0), (1, (w + 1) % WAVES, c1)):
            lanes = {"first": np.arange(c), "last": np.arange(PIECE - c, PIECE), "random": rng.choice(PIECE, c, replace=False)}[pick]
            m[r, p, lanes] = True
    return m.reshape(-1)


# wave by wave: nothing; one unit in either round; a drain that is just full (63 + 1, 1 + 63, 64 + 0, 0 + 64, 40 + 24); two full
# drains; 64 k + 1 (a one-unit flush behind a full drain); a push that straddles the full queue (40 + 40: 24 go in, the drain,
# 16 follow; 63 + 63; 63 + 2; 33 + 32)
BOUNDARY_PAIRS = [(0, 0), (0, 1), (1, 0), (63, 1), (1, 63), (64, 0), (0, 64), (64, 64), (64, 1), (1, 64), (40, 40), (40, 24), (40, 25), (63, 63), (63, 2), (33, 32)]


@pytest.fixture(scope="module")
def case(oracle, hip):
    """one warmed pair on the default area, eight scene scans with targets"""
    ref, dev = make_area_pair(oracle, hip, max_batch=8)
    warm_scene, _, frames = scene_frames(DEFAULT_AREA, (0.0, 0.0), 8, scene_seed=5, seed0=70)
    warm_both(ref, dev, warm_scene, (0.0, 0.0))
    return ref, dev, frames


def run(ref, dev, frames, layout, name, min_crop=0, min_vox=0):
    lay, want = LAYOUTS[layout]
    scans_dev = [host_scan(fr, lay(fr)) for fr in frames]
    tfs = np.stack([fr.tf for fr in frames])
    return three_views(ref, dev, [fr.scan for fr in frames], scans_dev, tfs, want, f"compaction/{name}/{layout}", min_crop, min_vox)


def queue_frames(frames):
    rng = np.random.default_rng(5)
    out = [Frame(frames[0].x, frames[0].y, frames[0].z, frames[0].tf)]  # the scan as it is: its own runs of returns
    out.append(punched(frames[1], mask_of_pairs(BOUNDARY_PAIRS, "random", rng)))
    out.append(punched(frames[2], mask_of_pairs(BOUNDARY_PAIRS[::-1], "first", rng)))
    out.append(punched(frames[3], mask_of_pairs(BOUNDARY_PAIRS[5:] + BOUNDARY_PAIRS[:5], "last", rng)))
    out.append(punched(frames[4], mask_of_pairs([(40, 40)] * WAVES, "random", rng)))  # every wave straddles
    c = rng.integers(1, 64, WAVES)
    out.append(punched(frames[5], mask_of_pairs([(int(k), 64 - int(k)) for k in c], "random", rng)))  # every wave: 64 exactly, one drain, no flush
    out.append(punched(frames[6], mask_of_pairs([(int(k), 65 - int(k)) for k in c], "random", rng)))  # every wave: 65
    out.append(punched(frames[7], np.ones(2 * WAVES * PIECE, dtype=bool)))  # every lane live: the queue passes the pieces through
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_queue_boundaries(case, layout):
    """pieces with 0, 1, 63 and 64 live lanes; waves whose live units total 64 k and 64 k + 1; pushes that straddle a full queue"""
    ref, dev, frames = case
    fs = queue_frames(frames)
    assert wave_pairs(fs[1]) == BOUNDARY_PAIRS and wave_pairs(fs[2]) == BOUNDARY_PAIRS[::-1] and wave_pairs(fs[3]) == BOUNDARY_PAIRS[5:] + BOUNDARY_PAIRS[:5]
    assert wave_pairs(fs[4]) == [(40, 40)] * WAVES
    assert all(a + b == 64 and 0 < a < 64 for a, b in wave_pairs(fs[5])) and all(a + b == 65 for a, b in wave_pairs(fs[6]))
    assert wave_pairs(fs[7]) == [(64, 64)] * WAVES
    mixed = live_units(fs[0]) & ~nonzero_points(fs[0].x, fs[0].y, fs[0].z).reshape(-1, UNIT).all(axis=1)
    assert 0 < live_units(fs[0]).sum() < 2 * WAVES * PIECE and mixed.any()  # the plain scan: zero runs, and units that are partly zero
    run(ref, dev, fs, layout, "queue")


def granularity_frames(frames, dev):
    rng = np.random.default_rng(6)
    n = frames[0].x.size
    out = [Frame(frames[0].x, frames[0].y, frames[0].z, frames[0].tf)]
    # 1: units whose only point that is not zero is the first (even units) or the last (odd units)
    x, y, z = densified(frames[1])
    keep = np.zeros((n // UNIT, UNIT), dtype=bool)
    keep[0::2, 0] = keep[1::2, UNIT - 1] = True
    for v in (x, y, z):
        v[~keep.reshape(-1)] = 0.0
    out.append(Frame(x, y, z, frames[1].tf))
    # 2: points with x == 0 and y or z != 0 (a third), with x == y == 0 (a tenth) - alone in their unit in every fourth unit
    x, y, z = densified(frames[2])
    pick = rng.random(n)
    x[pick < 0.33] = 0.0
    y[pick < 0.10] = 0.0
    lone = np.zeros((n // UNIT, UNIT), dtype=bool)
    lone[0::4, 3] = True
    lone = lone.reshape(-1)
    in_lone_unit = np.repeat(np.arange(n // UNIT) % 4 == 0, UNIT)
    x[in_lone_unit] = 0.0
    y[in_lone_unit & ~lone] = 0.0
    z[in_lone_unit & ~lone] = 0.0
    assert (nonzero_points(x, y, z) & (x == 0)).sum() > n // 4
    out.append(Frame(x, y, z, frames[2].tf))
    # 3: -0.0: dead units of -0.0 in all coordinates, and single -0.0 coordinates inside live units
    fr = punched(frames[3], rng.random(n // UNIT) < 0.5, zero=-0.0)
    assert np.signbit(fr.x[~nonzero_points(fr.x, fr.y, fr.z)]).all() and (~live_units(fr)).sum() > 500
    for v in (fr.x, fr.y, fr.z):
        v[rng.random(n) < 0.05] = f32(-0.0)
    mix = rng.random(n) < 0.05  # (-0.0, +0.0, -0.0): a zero point inside a live unit
    fr.x[mix], fr.y[mix], fr.z[mix] = f32(-0.0), f32(0.0), f32(-0.0)
    out.append(fr)
    # 4: points inside live units that the crops drop - inside the exclude box, outside the area, NaN, +-Inf - and units of nothing else
    x, y, z = densified(frames[4])
    bad = [(0.1, 0.1, 0.0), (500.0, 0.0, 0.0), (np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf), (np.nan, np.nan, np.nan), (0.0, 0.0, np.inf), (-0.0, np.nan, 0.0)]
    kind = rng.integers(0, len(bad), n)
    hit = rng.random(n) < 0.25
    hit |= np.repeat(rng.random(n // UNIT) < 0.1, UNIT)  # whole units: live by the zero test, nothing survives
    for k, b in enumerate(bad):
        sel = hit & (kind == k)
        x[sel], y[sel], z[sel] = f32(b[0]), f32(b[1]), f32(b[2])
    fr = Frame(x, y, z, frames[4].tf)
    with np.errstate(invalid="ignore"):
        _, kept = survivors(np.stack([x, y, z], axis=1), fr.tf, DEFAULT_AREA, dev=dev)
    assert live_units(fr).all() and (~kept.reshape(-1, UNIT).any(axis=1)).sum() > 100
    out.append(fr)
    # 5: the same bad points next to dead units
    fr = punched(frames[5], rng.random(n // UNIT) < 0.5)
    sel = hit & nonzero_points(fr.x, fr.y, fr.z)
    for k, b in enumerate(bad):
        s2 = sel & (kind == k)
        fr.x[s2], fr.y[s2], fr.z[s2] = f32(b[0]), f32(b[1]), f32(b[2])
    out.append(fr)
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_unit_granularity(case, layout):
    """units with one live point at either end, x == 0 points, -0.0, and points the crops drop inside live units"""
    ref, dev, frames = case
    fs = granularity_frames(frames, dev)
    assert live_units(fs[1]).all() and nonzero_points(fs[1].x, fs[1].y, fs[1].z).sum() == fs[1].x.size // UNIT
    run(ref, dev, fs, layout, "granularity")


def all_surviving(s, dev):
    x, y, z = s.x, s.y, s.z
    _, kept = survivors(np.stack([x, y, z], axis=1), s.tf, DEFAULT_AREA, dev=dev)
    kept &= nonzero_points(x, y, z)
    x, y, z = densified(s, only=kept)
    _, kept = survivors(np.stack([x, y, z], axis=1), s.tf, DEFAULT_AREA, dev=dev)
    assert kept.all()
    return Frame(x, y, z, s.tf)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ends(case, layout):
    """an all-zero frame inside a batch (and as its last frame); a frame all of whose 16 384 points survive both crops - every
    wave's segment of the code list is full; frames whose returns sit in one half of the scan"""
    ref, dev, frames = case
    n = frames[0].x.size
    zero = np.zeros(n, dtype=f32)
    half = np.arange(n // UNIT) < n // UNIT // 2
    fs = [
        Frame(frames[0].x, frames[0].y, frames[0].z, frames[0].tf),
        Frame(zero, zero, zero, frames[1].tf),
        all_surviving(frames[2], dev),
        punched(frames[3], half),
        punched(frames[4], ~half),
        all_surviving(frames[5], dev),
        Frame(-zero, zero, -zero, frames[6].tf),
    ]
    assert not live_units(fs[1]).any() and not live_units(fs[6]).any() and np.signbit(fs[6].x).all()
    gb = run(ref, dev, fs, layout, "ends")
    assert gb[1]["n_input_after_crop"] == 0 and gb[6]["n_input_after_crop"] == 0
    assert gb[2]["n_input_after_crop"] == n and gb[5]["n_input_after_crop"] == n


def make_pair_exclude_moved(oracle, hip, dx, max_batch=8):
    """make_area_pair on the default area with the exclude box moved by dx along x: it no longer holds the origin"""
    dets = []
    for lib in (oracle, hip):
        sp, dp = default_params(lib)
        sp.voxel_size = 0.25
        sp.sensor_hrays, sp.sensor_vrays = OS1_16[1], OS1_16[0]
        sp.sensor_vfov = f32(np.deg2rad(OS1_16[2]))
        sp.max_batch_frames = max_batch
        sp.oparea_offset[:] = DEFAULT_AREA[0]
        sp.oparea_size[:] = DEFAULT_AREA[1]
        sp.exclude_offset[0] = f32(sp.exclude_offset[0]) + f32(dx)
        dets.append(VoFOD(lib, sp, dp))
    return dets


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_zeros_are_ordinary_points_when_the_exclude_box_misses_the_origin(oracle, hip, layout):
    """exclude box at x = 1.84 .. 4.34 m: an exact zero is a point at the sensor, inside the area - kept.  Every unit that
    starts inside the cloud is live, the queue passes whole pieces through; what becomes of the zeros the oracle decides."""
    ref, dev = make_pair_exclude_moved(oracle, hip, 3.0)
    sp = dev.sp
    assert f32(sp.exclude_offset[0]) - f32(sp.exclude_size[0]) / f32(2) > 0
    warm_scene, _, frames = scene_frames(DEFAULT_AREA, (0.0, 0.0), 5, scene_seed=5, seed0=70)
    warm_both(ref, dev, warm_scene, (0.0, 0.0))
    rng = np.random.default_rng(7)
    n = frames[0].x.size
    zero = np.zeros(n, dtype=f32)
    fs = [
        Frame(frames[0].x, frames[0].y, frames[0].z, frames[0].tf),
        punched(frames[1], mask_of_pairs(BOUNDARY_PAIRS, "random", rng)),
        Frame(zero, zero, zero, frames[2].tf),
        punched(frames[3], rng.random(n // UNIT) < 0.5, zero=-0.0),
        punched(frames[4], mask_of_pairs([(40, 40)] * WAVES, "first", rng)),
    ]
    zeros = [int((~nonzero_points(fr.x, fr.y, fr.z)).sum()) for fr in fs]
    assert min(zeros) > 1000, zeros
    gb = run(ref, dev, fs, layout, "zeros_kept")
    assert gb[2]["n_input_after_crop"] == n  # the all-zero frame: every point kept, one voxel


@pytest.mark.parametrize("vrays,hrays", [(15, 1021), (15, 1020)])
def test_last_unit_is_partial(oracle, hip, vrays, hrays):
    """15 315 points (n % 8 = 3, n % 4 = 3: strided only) and 15 300 points (n % 8 = 4: the packed pass's last lane loads its
    second quad clamped): the last unit ends behind the cloud.  Its points inside the cloud are the only ones of the last piece
    that are not zero, or zero with the rest of it."""
    shape = (vrays, hrays, 33.2, 120.0)
    n = vrays * hrays
    assert n % UNIT in (3, 4) and (n % 4 == 0) == (hrays == 1020)
    ref, dev = make_area_pair(oracle, hip, shape=shape, max_batch=4)
    warm_scene, _, frames = scene_frames(DEFAULT_AREA, (0.0, 0.0), 4, shape=shape, scene_seed=5, seed0=70)
    warm_both(ref, dev, warm_scene, (0.0, 0.0), shape=shape)
    units = (n + UNIT - 1) // UNIT
    last_piece = np.arange(units) >= (units - 1) // PIECE * PIECE
    only_last = ~last_piece | (np.arange(units) == units - 1)
    fs = []
    for k, s in enumerate(frames):
        if k == 0:
            fs.append(Frame(s.x, s.y, s.z, s.tf, shape))
            continue
        x, y, z = densified(s)
        dead = ~np.repeat([only_last, ~last_piece, np.ones(units, dtype=bool)][k - 1], UNIT)[:n]
        x[dead] = y[dead] = z[dead] = 0.0
        fs.append(Frame(x, y, z, s.tf, shape))
    assert live_units(fs[1])[-1] and live_units(fs[1])[last_piece].sum() == 1 and not live_units(fs[2])[last_piece].any() and live_units(fs[3]).all()
    for layout in LAYOUTS if n % 4 == 0 else ["aos48"]:
        run(ref, dev, fs, layout, f"partial_{n}")
