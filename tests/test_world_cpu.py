"""The world store without a GPU: the numpy statement (world_cases.World) against cases written out by hand, its invariants, the
a-priori cell expression against the oracle, the C surface, and the patrol the store exists for - out of the box's reach and back -
on the CPU oracle."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import map_shift_cases as mc
import world_cases as wc
from vofod_amd import capi

I = 99  # init value of the hand-written cases
S = (5, 4, 3)


def _window():
    """value 100 * iz + 10 * iy + ix + 1 on the 5 x 4 x 3 window"""
    iz, iy, ix = np.indices((3, 4, 5))
    return (100 * iz + 10 * iy + ix + 1).astype(np.uint32)


def _world(max_tiles=8, lo=(3, 0, 0), hi=(2, 0, 0)):
    """box x in [-3, 7): two tiles along x - tile 0 holds x in [-3, 5), tile 1 x in [5, 7); y and z fit one tile"""
    return wc.World(S, lo, hi, max_tiles, I)


# ------------------------------------------------------------------------------------------------ hand-written cases
def test_out_and_back_by_hand():
    w, a = _world(), _window()
    assert tuple(w.T) == (2, 1, 1) and w.cap == 2  # (the pool is never larger than the box)
    b = w.shift(a, (2, 0, 0))
    # the columns x = 0, 1 left (world x = 0, 1: tile 0, allocated now); x = 3, 4 of the new window are world x = 5, 6: tile 1, absent
    want = np.full_like(a, I)
    want[:, :, :3] = a[:, :, 2:]
    np.testing.assert_array_equal(b, want)
    assert w.info() == dict(enabled=1, tile_edge=8, origin=(2, 0, 0), box_lo=(-3, 0, 0), box_hi=(7, 4, 3), tiles_used=1, tiles_cap=2, shifts_short_of_tiles=0, voxels_forgotten=0)
    assert w.alloc.tolist() == [[[True, False]]]
    # W: the stored columns, then the window
    np.testing.assert_array_equal(w.read(b, (0, 0, 0), (5, 4, 3)), a)
    np.testing.assert_array_equal(w.read(b, (-3, 0, 0), (3, 4, 3)), np.full((3, 4, 3), I, dtype=np.uint32))
    # back: the two init columns leave (nothing wanted, nothing forgotten), the stored ones re-enter
    c = w.shift(b, (-2, 0, 0))
    # (x = 2, 3, 4 never left: new[x] = old[x - 2] brings them back from b's x = 0, 1, 2)
    np.testing.assert_array_equal(c, a)
    assert w.info()["tiles_used"] == 1 and w.info()["origin"] == (0, 0, 0) and w.info()["voxels_forgotten"] == 0


def test_leaving_the_box_by_hand():
    w, a = _world(), _window()
    b = w.shift(a, (-4, 0, 0))  # window at world x in [-4, 1): its x = 0 is outside the box; x = 1..4 left: world x = 1..4
    assert w.info()["tiles_used"] == 1 and w.info()["voxels_forgotten"] == 0
    want = np.full_like(a, I)
    want[:, :, 4] = a[:, :, 0]
    np.testing.assert_array_equal(b, want)
    b[:, :, 0] = 7  # world x = -4: outside the box
    c = w.shift(b, (4, 0, 0))  # everything but x = 4 leaves: world x = -4 is forgotten (12 voxels), x = -3..-1 are init
    assert w.info()["voxels_forgotten"] == 12 and w.info()["origin"] == (0, 0, 0)
    np.testing.assert_array_equal(c, a)
    np.testing.assert_array_equal(w.read(c, (-4, 0, 0), (1, 4, 3)), np.full((3, 4, 1), I, dtype=np.uint32))


def test_an_init_pattern_overwrites_a_stored_one():
    """a voxel stored as non-init re-enters, is set to init, leaves and re-enters: it is init"""
    w, a = _world(), _window()
    b = w.shift(a, (1, 0, 0))
    c = w.shift(b, (-1, 0, 0))
    np.testing.assert_array_equal(c, a)
    c[:, :, 0] = I
    d = w.shift(w.shift(c, (1, 0, 0)), (-1, 0, 0))
    np.testing.assert_array_equal(d, c)
    assert w.info()["tiles_used"] == 1


def test_all_or_nothing_by_hand():
    """two tiles along y, one slot: a tile that exists is still updated when the shift's new tile does not fit, and where two are
    wanted and one would fit, none is taken"""
    w = wc.World(S, (0, 0, 0), (0, 9, 0), 1, I)  # tiles: y in [0, 8) and [8, 13); one slot
    a = _window()
    assert tuple(w.T) == (1, 2, 1) and w.cap == 1
    b = w.shift(a, (0, 6, 0))  # window y in [6, 10): leaving rows are world y = 0..3, tile 0: fits
    assert (w.used, w.short, w.forgotten) == (1, 0, 0)
    b[:] = a  # the window now spans both tiles: y = 6, 7 in tile 0, y = 8, 9 in tile 1
    c = w.shift(b, (0, -6, 0))  # all four rows leave: tile 1 is wanted and does not fit - rows y = 6, 7 are stored, 8, 9 forgotten
    assert (w.used, w.short, w.forgotten) == (1, 1, 2 * 5 * 3)
    np.testing.assert_array_equal(c, a)  # (the rows stored on the first trip)
    np.testing.assert_array_equal(w.read(c, (0, 6, 0), (5, 2, 3)), a[:, :2, :])
    np.testing.assert_array_equal(w.read(c, (0, 8, 0), (5, 2, 3)), np.full((3, 2, 5), I, dtype=np.uint32))
    # nothing at all where even the first wanted tile does not fit: two tiles wanted, one slot
    w = wc.World(S, (0, 0, 0), (0, 9, 0), 1, I)
    w.K[1] = 6
    w.shift(a, (0, 6, 0))
    assert (w.used, w.short, w.forgotten) == (0, 1, 60) and not w.alloc.any()
    assert (w.dense == I).all()


# ------------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_w_is_unchanged_by_random_walks_when_tiles_suffice(seed):
    rng = np.random.default_rng(seed)
    S_, lo, hi = (7, 5, 4), (11, 6, 3), (9, 10, 5)
    init = 0x3F000000
    w = wc.World(S_, lo, hi, wc.tile_count(S_, lo, hi), init)
    win = mc.random_bits(rng, (4, 5, 7))
    before = w.read_box(win)
    for _ in range(40):
        s = rng.integers(-9, 10, size=3)
        K1 = w.K + s
        if (K1 < w.lo).any() or (K1 + w.S > w.hi).any():  # the walk stays inside the box
            continue
        win = w.shift(win, s)
        np.testing.assert_array_equal(w.read_box(win), before)
    assert w.forgotten == 0 and w.short == 0 and w.used > 0


def test_all_or_nothing_on_random_maps():
    rng = np.random.default_rng(5)
    S_, lo, hi = (21, 13, 9), (19, 11, 5), (30, 9, 7)
    win = mc.random_bits(rng, (9, 13, 21))
    full = wc.World(S_, lo, hi, 10**6, 0)
    need = full.wanted_by_shift(win, (5, -3, 2))
    assert need > 1
    short = wc.World(S_, lo, hi, need - 1, 0)
    out = short.shift(win, (5, -3, 2))
    np.testing.assert_array_equal(out, mc.shift_statement(win, (5, -3, 2), 0))
    assert (short.used, short.short) == (0, 1) and not short.alloc.any() and (short.dense == 0).all()
    leaving = np.zeros(win.shape, dtype=bool)  # s = (5, -3, 2): x in [0, 5), y in [10, 13), z in [0, 2) - all inside the box
    leaving[:, :, :5] = leaving[:, 10:, :] = leaving[:2, :, :] = True
    assert short.forgotten == int((win[leaving] != 0).sum())
    exact = wc.World(S_, lo, hi, need, 0)
    exact.shift(win, (5, -3, 2))
    assert (exact.used, exact.short, exact.forgotten) == (need, 0, 0)


# ------------------------------------------------------------------------------------------------ a-priori cells
def test_apriori_cells_are_the_oracles_inside_the_window(oracle):
    det = mc.make_det(oracle, voxel_size=0.25, oparea_offset=(40.0, 20.0, -1.25), oparea_size=(10.0, 6.0, 4.0))
    sx, sy, sz = det.map_size
    rng = np.random.default_rng(11)
    off = np.array(det.map_offset, dtype=np.float32)
    pts = (off + rng.random((4000, 3)) * np.array([sx, sy, sz]) * 0.25).astype(np.float32)
    # points on and next to voxel faces, where one rounding decides
    k = rng.integers(0, [sx, sy, sz], size=(2000, 3))
    face = (off + k.astype(np.float32) * np.float32(0.25)).astype(np.float32)
    pts = np.vstack([pts, face, np.nextafter(face, np.float32(-1e9)), np.nextafter(face, np.float32(1e9))])
    det.load_apriori(pts)
    got = det.read_map().view(np.uint32) == wc.INF_BITS
    w = wc.World((sx, sy, sz), (0, 0, 0), (0, 0, 0), 1, mc.init_bits(det, capi.MAP_VOXELS))
    st, win = w.load_apriori(np.full((sz, sy, sx), w.init, dtype=np.uint32), pts, det.map_offset, 0.25)
    assert st == capi.OK and w.used == 0
    np.testing.assert_array_equal(win == wc.INF_BITS, got)
    assert got.sum() > 3000


def test_apriori_far_points_by_hand():
    w = wc.World(S, (3, 0, 0), (2, 0, 0), 2, I)
    a = _window()
    off, vs = (10.0, 20.0, 30.0), 0.5
    pts = np.array([[10.25, 20.25, 30.25],   # cell (0, 0, 0): the window
                    [9.75, 20.25, 30.25],    # x = -1: tile 0
                    [12.75, 21.75, 31.25],   # x = 5, y = 3, z = 2: tile 1
                    [8.25, 20.25, 30.25],    # x = -4: outside the box
                    [10.25, 22.25, 30.25],   # y = 4: outside the box
                    [np.nan, 20.25, 30.25], [np.inf, 20.25, 30.25], [3e9, 20.25, 30.25]], dtype=np.float32)
    st, b = w.load_apriori(a, pts, off, vs)
    assert st == capi.OK and w.used == 2
    want = a.copy()
    want[0, 0, 0] = wc.INF_BITS
    np.testing.assert_array_equal(b, want)
    box = w.read_box(b)
    assert box[0, 0, 2] == wc.INF_BITS and box[2, 3, 8] == wc.INF_BITS and (box == wc.INF_BITS).sum() == 3
    # a pool one tile short: nothing changes, the window included
    w = wc.World(S, (3, 0, 0), (2, 0, 0), 1, I)
    st, b = w.load_apriori(a, pts, off, vs)
    assert st == capi.ERR_CAPACITY and b is a and w.used == 0 and not w.alloc.any() and (w.dense == I).all()


# ------------------------------------------------------------------------------------------------ the surface
def test_entry_points_are_declared_bound_and_exported():
    names = ("world_enable", "world_disable", "world_status", "world_read")
    for n in names:
        assert n in capi.declared_entry_points() and n in capi._SIGS and n in capi.PRODUCT_ONLY, n
    header = capi.HEADER.read_text()
    assert "#define VOFOD_WORLD_TILE 8" in header and "WORLD STORE" in header and capi.WORLD_TILE == wc.TILE == 8
    # the struct as the header lays it out: eleven int32, padding, four uint64
    body = header[header.index("typedef struct vofod_world_info {"):header.index("} vofod_world_info;")]
    fields = [f for f, _ in capi.WorldInfo._fields_]
    assert [body.index(f) for f in fields] == sorted(body.index(f) for f in fields)
    assert C.sizeof(capi.WorldInfo) == 80 and capi.WorldInfo.tiles_used.offset == 48
    so = Path(capi.__file__).resolve().parent / "csrc" / "libvofod_hip.so"
    if not so.exists():  # hipcc cross-compiles gfx950 without a GPU
        import subprocess

        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    lib = capi.Library(so, "vofod_")
    three = (C.c_int32 * 3)(0, 0, 0)
    info = capi.WorldInfo()
    # null handle: refused before anything is touched
    assert lib.world_enable(None, three, three, 1) == capi.ERR_INVALID_ARG
    assert lib.world_disable(None) == capi.ERR_INVALID_ARG
    assert lib.world_status(None, C.byref(info)) == capi.ERR_INVALID_ARG
    assert lib.world_read(None, three, three, None, 0) == capi.ERR_INVALID_ARG
    from vofod_amd.detector import VoFOD

    for m in ("world_enable", "world_disable", "world_info", "world_read"):
        assert callable(getattr(VoFOD, m))


def test_oracle_does_not_export_the_store(oracle):
    for n in ("world_enable", "world_disable", "world_status", "world_read"):
        assert not hasattr(oracle, n)


# ------------------------------------------------------------------------------------------------ the patrol
def _near_box(dets, tgt):
    return int((np.abs(dets["position"] - np.array(tgt)).max(axis=1) < 1.0).sum()) if len(dets) else 0


def test_patrol_out_and_back_keeps_what_the_vehicle_knew(oracle):
    """Handle A warms up round TARGET_IN_AREA; the area goes 40 voxels towards -x and back.  With the store the voxel map returns bit
    for bit and a fresh handle on it finds the box in every continuation scan; on the maps as vofod_map_shift alone leaves them -
    unknown space round everything mapped before - it finds none.  Flags and raycast map are there-and-back on both sides."""
    tgt = mc.TARGET_IN_AREA
    out, back = (-40, 0, 0), (40, 0, 0)
    a = mc.make_det(oracle)
    mc.warm(a, tgt)
    maps = {w: mc.read_bits(a, w) for w in mc.MAPS}
    forgetful = {w: mc.shift_statement(mc.shift_statement(maps[w], out, mc.init_bits(a, w)), back, mc.init_bits(a, w)) for w in mc.MAPS}
    assert int((forgetful[capi.MAP_VOXELS] != maps[capi.MAP_VOXELS]).sum()) > 10000
    lo, hi = (43, 3, 0), (5, 2, 1)
    world = wc.World(a.map_size, lo, hi, wc.tile_count(a.map_size, lo, hi), mc.init_bits(a, capi.MAP_VOXELS))
    v = world.shift(world.shift(maps[capi.MAP_VOXELS], out), back)
    np.testing.assert_array_equal(v, maps[capi.MAP_VOXELS])
    assert world.forgotten == 0 and world.short == 0 and tuple(world.K) == (0, 0, 0)
    remembered = dict(forgetful)
    remembered[capi.MAP_VOXELS] = v
    found = {}
    for name, m in (("remembered", remembered), ("forgetful", forgetful)):
        b = mc.hand_over(oracle, {w: m[w].view(np.float32) for w in mc.MAPS})
        found[name] = [_near_box(b.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST), tgt) for s in mc.continuation_scans(tgt)]
    print(found)
    assert all(n >= 1 for n in found["remembered"]), found
    assert all(n == 0 for n in found["forgetful"]), found
