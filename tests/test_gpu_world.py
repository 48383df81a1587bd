"""The world store on the device (include/vofod.h WORLD STORE, vofod_amd/csrc/world_store.h) against the numpy statement of
world_cases.World: after every call the three window maps, vofod_world_read over the whole box and every counter are the
statement's.  All-or-nothing allocation makes that comparison exact whatever order the device's atomics arrive in."""
import os

import numpy as np
import pytest

import map_shift_cases as mc
import world_cases as wc
from helpers import sync_maps
from test_gpu_map_shift import BASE, SIZES, _assert_unchanged, _compare_maps, _det, _shifts, _snapshot_state
from test_gpu_stream_route import profiled_calls
from vofod_amd import capi

pytestmark = pytest.mark.gpu
if os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"):
    pytest.skip("oracle against oracle: the oracle has no world store", allow_module_level=True)

LO, HI = (19, 11, 5), (30, 9, 7)  # margins: no multiples of the tile edge
V = capi.MAP_VOXELS


class Rig:
    """a detector with the store enabled beside the statement, and the integer origin k the offsets are made from"""

    def __init__(self, lib, which, max_tiles=None, lo=LO, hi=HI, seed=0, offset=BASE):
        self.det, self.vs = _det(lib, which, offset=offset)
        self.base = offset
        self.S = self.det.map_size
        self.rng = np.random.default_rng(seed)
        self.k = np.zeros(3, dtype=np.int64)
        self.init = {w: mc.init_bits(self.det, w) for w in mc.MAPS}
        self.bits = {w: np.full(self.S[::-1], self.init[w], dtype=np.uint32) for w in mc.MAPS}
        self.world = None
        if max_tiles is not False:
            self.enable(wc.tile_count(self.S, lo, hi) if max_tiles is None else max_tiles, lo, hi)

    def enable(self, max_tiles, lo=LO, hi=HI):
        assert self.det.world_enable(lo, hi, max_tiles) == capi.OK
        self.world = wc.World(self.S, lo, hi, max_tiles, self.init[V])

    def fill(self, maps=mc.MAPS, density=1.0):
        """random 32-bit patterns in the window (a share `density` of the voxels, init elsewhere)"""
        for w in maps:
            b = mc.random_bits(self.rng, self.S[::-1])
            if density < 1.0:
                b[self.rng.random(b.shape) >= density] = self.init[w]
            self.write(w, b)

    def write(self, which, b):
        self.bits[which] = np.ascontiguousarray(b, dtype=np.uint32)
        mc.write_bits(self.det, which, self.bits[which])

    def shift(self, s, allow=()):
        k1 = self.k + np.array(s, dtype=np.int64)
        st = self.det.map_shift(s, mc.shifted_offset(self.base, k1, self.vs), allow=allow)
        if st != capi.OK:
            return st
        self.k = k1
        same_place = not any(s)  # (a shift by zero to the same offset returns before anything runs)
        for w in mc.MAPS:
            if w == V and not same_place:
                self.bits[w] = self.world.shift(self.bits[w], s)
            else:
                self.bits[w] = mc.shift_statement(self.bits[w], s, self.init[w])
        return st

    def check(self, what=""):
        for w in mc.MAPS:
            np.testing.assert_array_equal(mc.read_bits(self.det, w), self.bits[w], err_msg=f"{what}: map {w}")
        assert wc.info_dict(self.det) == self.world.info(), what
        wd = self.world
        got = self.det.world_read(wd.lo, wd.hi - wd.lo).view(np.uint32)
        np.testing.assert_array_equal(got, wd.read_box(self.bits[V]), err_msg=f"{what}: W over the box")


# ------------------------------------------------------------------------------------------------ 1. sequences of shifts
@pytest.mark.parametrize("which,pool", [("21x13x9", "ample"), ("21x13x9", "tight"), ("121x81x33", "ample"), ("121x81x33", "tight")])
def test_sequences_of_shifts_equal_the_statement(hip, which, pool):
    S = SIZES[which][1]
    total = wc.tile_count(S, LO, HI)
    r = Rig(hip, which, max_tiles=total if pool == "ample" else max(total // 3, 1), seed=len(which) + len(pool))
    r.fill()
    r.check("after enable")
    seq = _shifts(S) + [(-(S[0] - 1), 0, 0), (0, -S[1], 0), (-2, 3, -1), (0, 0, S[2] + 3), (0, 0, -(S[2] + 3))]
    for n, s in enumerate(seq):
        assert r.shift(s) == capi.OK
        r.check(f"shift {n} {s}")
        if n % 3 == 2:
            r.fill((V,), density=0.5)  # new content, so that later trips have something to store
    i = r.world.info()
    print(which, pool, i)
    assert i["tiles_used"] > 0 and i["voxels_forgotten"] > 0  # (the walk leaves the box: S - 1 and S are beyond the margins)
    assert (i["shifts_short_of_tiles"] > 0) == (pool == "tight")


# ------------------------------------------------------------------------------------------------ 2. there and back
@pytest.mark.parametrize("s", [(2, -3, 1), (-5, 0, 0), (3, 1, 0)], ids=str)
def test_there_and_back_returns_the_voxel_map_bit_for_bit(hip, s):
    r = Rig(hip, "121x81x33", seed=7)
    r.fill()
    before = {w: r.bits[w].copy() for w in mc.MAPS}
    assert (before[V] == 0x7F800000).any() and (before[V] == 0x80000000).any() and (before[V] == 0x7FC01234).any()
    assert r.shift(s) == capi.OK
    assert r.shift(tuple(-v for v in s)) == capi.OK
    r.check()
    np.testing.assert_array_equal(mc.read_bits(r.det, V), before[V])  # +inf, -0.0f and NaN payloads included
    for w in (capi.MAP_FLAGS, capi.MAP_RAYCAST):  # per-pass state: the rim is init as without the store
        want = mc.shift_statement(mc.shift_statement(before[w], s, 0), tuple(-v for v in s), 0)
        got = mc.read_bits(r.det, w)
        np.testing.assert_array_equal(got, want)
        assert (got != before[w]).any()
    i = r.world.info()
    assert i["voxels_forgotten"] == 0 and i["shifts_short_of_tiles"] == 0 and i["origin"] == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ 3. stale values
def test_an_init_pattern_replaces_the_stored_one(hip):
    """A voxel stored as non-init re-enters, is set to init through write_map, leaves and re-enters: it is init.  (A put that
    skips patterns equal to init brings the first trip's value back.)"""
    r = Rig(hip, "21x13x9", seed=3)
    r.fill((V,))
    first = r.bits[V].copy()
    s, back = (3, 0, 0), (-3, 0, 0)
    assert r.shift(s) == capi.OK and r.shift(back) == capi.OK
    np.testing.assert_array_equal(mc.read_bits(r.det, V), first)
    cleared = first.copy()
    cleared[:, :, :3] = r.init[V]  # the three columns that were stored
    assert (first[:, :, :3] != r.init[V]).any()
    r.write(V, cleared)
    assert r.shift(s) == capi.OK and r.shift(back) == capi.OK
    r.check()
    np.testing.assert_array_equal(mc.read_bits(r.det, V), cleared)


# ------------------------------------------------------------------------------------------------ 4. reset
def test_reset_empties_the_store_and_reused_tiles_start_from_init(hip):
    """After vofod_reset the pool's slots are handed out again; a reused tile still holds the first life's patterns in memory, and
    every voxel of it that the new trip does not write must read init.  (A claim without the fill shows the old patterns.)"""
    r = Rig(hip, "21x13x9", seed=4)
    r.fill((V,))
    assert r.shift((5, 2, 1)) == capi.OK
    r.check("first life")
    used = r.world.used
    assert used > 1
    r.det.reset()
    r.world.reset()
    for w in mc.MAPS:
        r.bits[w] = np.full(r.S[::-1], r.init[w], dtype=np.uint32)
    r.check("after reset")  # W is init everywhere; K, the box and the switch are kept
    assert wc.info_dict(r.det)["origin"] == (5, 2, 1) and wc.info_dict(r.det)["tiles_used"] == 0
    # second life: one voxel per leaving column, so that every reused tile takes a few words only
    sparse = r.bits[V].copy()
    sparse[4, 6, :] = 0x12345678
    r.write(V, sparse)
    assert r.shift((-5, -2, -1)) == capi.OK and r.shift((9, 0, 0)) == capi.OK
    r.check("second life")
    assert 0 < r.world.used <= used
    box = r.det.world_read(r.world.lo, r.world.hi - r.world.lo).view(np.uint32)
    assert set(np.unique(box).tolist()) == {int(r.init[V]), 0x12345678}


# ------------------------------------------------------------------------------------------------ 5. the pool one tile short
def test_pool_one_tile_short_allocates_nothing_and_still_updates(hip):
    s1, s2 = (3, 0, 0), (-6, 2, 0)
    S = SIZES["21x13x9"][1]
    # what the two shifts want, from a dry run of the statement with an ample pool and the same windows
    dry = wc.World(S, LO, HI, 10**6, mc.init_bits(_det(hip, "21x13x9")[0], V))
    rng = np.random.default_rng(5)
    w1, w2 = mc.random_bits(rng, S[::-1]), mc.random_bits(rng, S[::-1])
    n1 = dry.wanted_by_shift(w1, s1)
    dry.shift(w1, s1)
    n2 = dry.wanted_by_shift(w2, s2)
    assert n1 >= 2 and n2 >= 2
    r = Rig(hip, "21x13x9", max_tiles=n1 + n2 - 1)
    r.write(V, w1)
    assert r.shift(s1) == capi.OK
    r.check("first shift fits")
    assert r.world.used == n1 and r.world.short == 0
    r.write(V, w2)
    stored_before = r.world.dense.copy()
    assert r.shift(s2) == capi.OK  # the shift goes through: the vehicle must not lose its box
    r.check("second shift is one tile short")
    i = wc.info_dict(r.det)
    assert i["tiles_used"] == n1 and i["shifts_short_of_tiles"] == 1 and i["voxels_forgotten"] > 0
    assert (r.world.dense != stored_before).any()  # the tiles of the first trip took the rows that left through them
    # the next shift that fits allocates: one voxel leaves into a tile that does not exist yet
    one = np.full(S[::-1], r.init[V], dtype=np.uint32)
    one[8, 12, 20] = 0xCAFE0001
    r.write(V, one)
    assert r.world.wanted_by_shift(one, (-1, -1, -1)) == 1
    assert r.shift((-1, -1, -1)) == capi.OK
    r.check("third shift fits")
    i = wc.info_dict(r.det)
    assert i["tiles_used"] == n1 + 1 and i["shifts_short_of_tiles"] == 1


# ------------------------------------------------------------------------------------------------ 6. leaving the box
def test_a_walk_out_of_the_box_forgets_and_counts(hip):
    r = Rig(hip, "21x13x9", seed=6)
    r.fill((V,))
    first = r.bits[V].copy()
    assert r.shift((-25, 0, 0)) == capi.OK  # the window covers world x in [-25, -4): six columns beyond box_lo = -19
    r.check("out")
    assert r.world.forgotten == 0
    r.fill((V,))
    outside = int((r.bits[V][:, :, :6] != r.init[V]).sum())
    assert r.shift((25, 0, 0)) == capi.OK
    r.check("back")
    np.testing.assert_array_equal(mc.read_bits(r.det, V), first)
    assert wc.info_dict(r.det)["voxels_forgotten"] == outside > 0
    got = r.det.world_read((-25, 0, 0), (6, 13, 9)).view(np.uint32)  # W outside the box is init
    assert (got == r.init[V]).all()


# ------------------------------------------------------------------------------------------------ 7. a-priori map
def _sheet_and_wall(r):
    """a ground sheet that reaches beyond the window on every side and a wall 10 voxels beyond its +x face, with points on voxel
    faces of the window's last voxels (where one rounding decides between window and store)"""
    off = np.array(r.det.map_offset, dtype=np.float64)
    sx, sy, sz = r.S
    vs = r.vs
    gx, gy = np.meshgrid(np.arange(-25, sx + 40) + 0.5, np.arange(-15, sy + 14) + 0.5, indexing="ij")
    sheet = np.stack([off[0] + gx.ravel() * vs, off[1] + gy.ravel() * vs, np.full(gx.size, off[2] + 0.25 * vs)], axis=1)
    wy, wz = np.meshgrid(np.arange(-3, sy + 3) + 0.5, np.arange(0, sz + 4) + 0.5, indexing="ij")
    wall = np.stack([np.full(wy.size, off[0] + (sx + 10.5) * vs), off[1] + wy.ravel() * vs, off[2] + wz.ravel() * vs], axis=1)
    face = np.array([[off[0] + sx * vs, off[1] + 2.5 * vs, off[2] + 3.5 * vs], [off[0], off[1] + sy * vs, off[2] + 3.5 * vs]], dtype=np.float32)
    edge = np.vstack([face, np.nextafter(face, np.float32(-1e9)), np.nextafter(face, np.float32(1e9))])
    odd = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [3e9, 0, 0], [-3e9, 1e30, 0]], dtype=np.float32)
    return np.vstack([sheet, wall, edge, odd]).astype(np.float32), wall.astype(np.float32)


def _load(r, pts, allow=()):
    st = r.det.load_apriori(pts, allow=allow)
    want, win = r.world.load_apriori(r.bits[V], pts, r.det.map_offset, r.vs)
    assert st == want
    r.bits[V] = win
    return st


def test_apriori_points_beyond_the_window_enter_with_the_shift(hip):
    r = Rig(hip, "21x13x9", seed=8)
    pts, _ = _sheet_and_wall(r)
    assert _load(r, pts) == capi.OK
    r.check("after the load")
    assert (r.bits[V] == wc.INF_BITS).sum() >= 21 * 13 and r.world.used > 10
    st = r.det.status()
    assert (st.background_pts_sufficient, st.sure_background_sufficient) == (1, 1)
    for s in [(8, 0, 0), (5, -4, 0), (-20, 9, 0)]:
        before = r.bits[V]
        assert r.shift(s) == capi.OK
        r.check(f"shift {s}")
        rim = mc.shift_statement(np.zeros_like(before), s, 1).astype(bool)
        assert (r.bits[V][rim] == wc.INF_BITS).any()  # the a-priori map is there when the area gets to it
        if tuple(r.world.K) == (13, -4, 0):  # the wall, 10 voxels beyond the first window's +x face (world x = 31), has entered
            assert (r.bits[V][1:, 3:, 18] == wc.INF_BITS).all() and (r.bits[V][1:, 3:, 17] != wc.INF_BITS).all()
    # a second cloud at K != 0: the cells come from the window's geometry now
    assert tuple(r.world.K) != (0, 0, 0)
    assert _load(r, _sheet_and_wall(r)[0]) == capi.OK
    r.check("second load")


def test_apriori_with_a_pool_too_small_changes_nothing(hip):
    r = Rig(hip, "21x13x9", max_tiles=False, seed=9)
    pts, wall = _sheet_and_wall(r)
    need = wc.World(r.S, LO, HI, 10**6, r.init[V])
    need.load_apriori(r.bits[V], pts, r.det.map_offset, r.vs)
    r.enable(need.used - 1)
    r.fill((V,), density=0.3)
    before = _snapshot_state(r.det)
    assert _load(r, pts, allow=(capi.ERR_CAPACITY,)) == capi.ERR_CAPACITY
    _assert_unchanged(r.det, before, "capacity")  # window and latches
    r.check("capacity")  # store and counters
    assert wc.info_dict(r.det)["tiles_used"] == 0 and r.det.status().sure_background_sufficient == 0
    # the store still works: a shift allocates, and a cloud that fits loads
    assert r.shift((2, 0, 0)) == capi.OK
    r.check("shift after the refusal")
    used = r.world.used
    assert _load(r, wall[:50]) == capi.OK
    r.check("a cloud that fits")
    assert r.world.used > used


# ------------------------------------------------------------------------------------------------ 8. the patrol against the oracle
def test_patrol_out_and_back_against_the_oracle(oracle, hip):
    tgt = mc.TARGET_IN_AREA
    out, back = (-40, 0, 0), (40, 0, 0)
    dev = mc.make_det(hip)
    mc.warm(dev, tgt)
    id_shift = int(dev.status().last_detection_id)
    base = tuple(dev.sp.oparea_offset)
    lo, hi = (43, 3, 0), (5, 2, 1)
    assert dev.world_enable(lo, hi, wc.tile_count(dev.map_size, lo, hi)) == capi.OK
    maps = {w: mc.read_bits(dev, w) for w in mc.MAPS}
    world = wc.World(dev.map_size, lo, hi, wc.tile_count(dev.map_size, lo, hi), mc.init_bits(dev, V))
    assert dev.map_shift(out, mc.shifted_offset(base, out, mc.VS)) == capi.OK
    assert dev.map_shift(back, mc.shifted_offset(base, (0, 0, 0), mc.VS)) == capi.OK
    want = {w: mc.shift_statement(mc.shift_statement(maps[w], out, mc.init_bits(dev, w)), back, mc.init_bits(dev, w)) for w in mc.MAPS}
    want[V] = world.shift(world.shift(maps[V], out), back)
    np.testing.assert_array_equal(want[V], maps[V])
    for w in mc.MAPS:
        np.testing.assert_array_equal(mc.read_bits(dev, w), want[w], err_msg=f"map {w}")
    assert wc.info_dict(dev) == world.info()
    b = mc.hand_over(oracle, {w: want[w].view(np.float32) for w in mc.MAPS})
    n_det = 0
    for k, s in enumerate(mc.continuation_scans(tgt)):
        da = b.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        db = dev.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        print(f"continuation scan {k}: oracle {len(da)} detections, HIP {len(db)}")
        mc.assert_detections_equal_mod_id(da, db, id_shift)
        _compare_maps(b, dev, f"continuation scan {k}")
        assert b.status().raycast_pending == dev.status().raycast_pending
        sync_maps(b, dev)
        n_det += int((np.abs(da["position"] - np.array(tgt)).max(axis=1) < 1.0).sum()) if len(da) else 0
    assert n_det >= 1  # the oracle finds the box: the carved air came back with the voxel map


# ------------------------------------------------------------------------------------------------ 9. refusals change nothing
def _world_state(det):
    i = wc.info_dict(det)
    box = det.world_read(i["box_lo"], np.array(i["box_hi"]) - np.array(i["box_lo"])).view(np.uint32).copy() if i["enabled"] else None
    return i, box


def _assert_world_unchanged(det, before, what):
    i, box = _world_state(det)
    assert i == before[0], what
    if box is not None:
        np.testing.assert_array_equal(box, before[1], err_msg=what)


def test_refusals_change_nothing(hip):
    dev = mc.make_det(hip)
    dev.load_apriori(mc.ground_apriori())
    sc = mc.scans(mc.TARGET_IN_AREA, 0, 2)
    dev.process_scan(sc[0].scan, sc[0].tf)
    off = {"enabled": 0, "tile_edge": 0, "origin": (0, 0, 0), "box_lo": (0, 0, 0), "box_hi": (0, 0, 0), "tiles_used": 0, "tiles_cap": 0, "shifts_short_of_tiles": 0, "voxels_forgotten": 0}
    assert wc.info_dict(dev) == off
    # off: disable and read have nothing to work on
    before = _snapshot_state(dev)
    assert dev.world_disable(allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
    three = np.zeros(3, dtype=np.int32)
    one = np.ones(3, dtype=np.int32)
    buf = np.zeros(1, dtype=np.float32)
    assert dev.lib.world_read(dev.h, capi.ptr(three), capi.ptr(one), capi.ptr(buf), 1) == capi.ERR_NOT_PENDING
    # bad margins, no tiles, a directory beyond 2^31 words
    for lo, hi, n in [((-1, 0, 0), (0, 0, 0), 4), ((0, 0, 0), (0, -3, 0), 4), ((0, 0, 0), (0, 0, 0), 0), ((2**31 - 1,) * 3, (0, 0, 0), 4), ((0, 0, 0), (2**31 - 1, 0, 0), 4)]:
        assert dev.world_enable(lo, hi, n, allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG, (lo, hi, n)
        assert wc.info_dict(dev) == off
    # a ticket in flight
    t = dev.batch_submit([sc[1].scan], sc[1].tf[None])
    assert dev.world_enable(LO, HI, 64, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
    assert wc.info_dict(dev) == off
    dev.batch_collect(t)
    _assert_unchanged(dev, (before[0], mc.status_tuple(dev)), "refused enables")  # (the collect may hand out ids: the maps are compared)
    # a raycast pass pending
    dev.raycast_begin(sc[1].scan, sc[1].tf)
    assert dev.world_enable(LO, HI, 64, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
    assert wc.info_dict(dev) == off
    dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION, capi.ERR_RAYCAST_EMPTY))
    # enabled: a second enable, a shift that takes K past 2^30
    assert dev.world_enable(LO, HI, 4096) == capi.OK
    base = tuple(dev.sp.oparea_offset)
    assert dev.map_shift((3, 0, 0), mc.shifted_offset(base, (3, 0, 0), mc.VS)) == capi.OK
    assert wc.info_dict(dev)["tiles_used"] > 0
    before, wbefore = _snapshot_state(dev), _world_state(dev)
    assert dev.world_enable(LO, HI, 64, allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG
    assert dev.world_enable((1, 1, 1), (1, 1, 1), 8, allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG
    _assert_unchanged(dev, before, "second enable")
    _assert_world_unchanged(dev, wbefore, "second enable")
    for s in [(2**30 - 2, 0, 0), (0, -(2**30) - 1, 0), (0, 0, 2**31 - 1), (-(2**31), 0, 0)]:
        k1 = np.array([3, 0, 0]) + np.array(s)
        assert dev.map_shift(s, mc.shifted_offset(base, k1, mc.VS), allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG, s
        assert b"2^30" in dev.lib.last_error_string(dev.h)
        _assert_unchanged(dev, before, f"shift {s}")
        _assert_world_unchanged(dev, wbefore, f"shift {s}")
    # a ticket in flight: the shift's own refusal, with the store on
    t = dev.batch_submit([sc[1].scan], sc[1].tf[None])
    assert dev.map_shift((1, 0, 0), mc.shifted_offset(base, (4, 0, 0), mc.VS), allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
    assert dev.world_disable(allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
    dev.batch_collect(t)
    _assert_world_unchanged(dev, wbefore, "ticket in flight")
    # disable, and the handle is as it was before the store
    assert dev.world_disable() == capi.OK
    assert wc.info_dict(dev) == off
    assert dev.world_disable(allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
    assert dev.map_shift((2**30 + 5, 0, 0), mc.shifted_offset(base, (4, 0, 0), mc.VS), allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG  # (the geometry check's refusal)
    assert b"2^30" not in dev.lib.last_error_string(dev.h)
    assert dev.world_enable(LO, HI, 64) == capi.OK and wc.info_dict(dev)["origin"] == (0, 0, 0)  # K starts again


# ------------------------------------------------------------------------------------------------ 10. routes
def test_routes_with_the_store_on_and_off(hip):
    r = Rig(hip, "121x81x33", max_tiles=False, seed=10)
    r.fill()
    world = {"k_world_mark", "k_world_claim", "k_world_put", "k_world_get"}
    lib, det = r.det.lib, r.det
    lib.profile_enable(det.h, 1)
    profiled_calls(lib, det)
    assert det.map_shift((3, 1, 0), mc.shifted_offset(BASE, (3, 1, 0), r.vs)) == capi.OK
    off = profiled_calls(lib, det)
    assert off == {"k_map_shift": 3}, off  # the parent's launches
    assert det.world_enable(LO, HI, 4096) == capi.OK
    profiled_calls(lib, det)
    assert det.map_shift((-3, -1, 0), mc.shifted_offset(BASE, (0, 0, 0), r.vs)) == capi.OK
    on = profiled_calls(lib, det)
    assert on == {"k_map_shift": 3, **{k: 1 for k in world}}, on
    det.world_read((0, 0, 0), (4, 4, 4))
    assert profiled_calls(lib, det) == {"k_world_gather": 1}
    det.load_apriori(np.array([[BASE[0] - 3.0, BASE[1] + 1.0, BASE[2] + 1.0]], dtype=np.float32))
    ap = profiled_calls(lib, det)
    assert ap == {"k_world_mark_points": 1, "k_world_claim": 1, "k_apriori": 1, "k_world_put_points": 1}, ap
    assert det.world_disable() == capi.OK
    assert det.map_shift((1, 0, 0), mc.shifted_offset(BASE, (1, 0, 0), r.vs)) == capi.OK
    assert profiled_calls(lib, det) == {"k_map_shift": 3}
    lib.profile_enable(det.h, 0)
