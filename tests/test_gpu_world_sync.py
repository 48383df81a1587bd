"""World snapshots on the device (include/vofod.h WORLD SNAPSHOTS, vofod_amd/csrc/world_sync.h) against the numpy statement of
world_sync_cases.SyncWorld: every exported record is the statement's byte for byte (the generation is the device's own: it is random),
every apply answers what the statement answers, and afterwards the three window maps, vofod_world_read over the whole box and every
counter are the statement's."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import map_shift_cases as mc
import world_cases as wc
import world_sync_cases as ws
from test_gpu_range_image import DeviceMem
from test_gpu_map_shift import BASE, SIZES, _assert_unchanged, _snapshot_state
from test_gpu_stream_route import profiled_calls
from test_gpu_world import HI, LO, Rig, V, _assert_world_unchanged, _sheet_and_wall, _world_state
from vofod_amd import capi

pytestmark = pytest.mark.gpu
if os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"):
    pytest.skip("oracle against oracle: the oracle has no world store", allow_module_level=True)

FULL, DELTA = capi.SNAPSHOT_FULL, capi.SNAPSHOT_DELTA
BIG_LO, BIG_HI = (43, 29, 9), (51, 21, 11)  # 121 x 81 x 33: a box of 215 x 131 x 53 voxels, 27 x 17 x 7 = 3213 tiles


class SRig(Rig):
    """test_gpu_world.Rig with the snapshots' statement in the place of the store's"""

    def enable(self, max_tiles, lo=LO, hi=HI):
        assert self.det.world_enable(lo, hi, max_tiles) == capi.OK
        self.world = ws.SyncWorld(self.S, lo, hi, max_tiles, self.init[V], self.det.map_offset, self.vs)
        self.margins = (lo, hi)

    def shift(self, s, allow=()):
        st = super().shift(s, allow)
        if st == capi.OK and not any(s):  # (Rig leaves the statement alone where nothing moves; to the chains it is a shift like any other)
            self.bits[V] = self.world.shift(self.bits[V], s)
        self.world.offset = np.array(self.det.map_offset, dtype=np.float32)
        return st

    def load(self, pts, allow=()):
        st = self.det.load_apriori(pts, allow=allow)
        want, win = self.world.load_apriori(self.bits[V], pts, self.det.map_offset, self.vs)
        assert st == want
        self.bits[V] = win
        return st

    def export(self, kind, device=False, allow=()):
        """the device's record, held to the statement's bytes; a status in `allow` (the statement's too) is returned instead"""
        if device:  # through a device buffer of the caller's, 16-byte aligned (hipMalloc's are)
            mem = DeviceMem()
            cap = ws.nbytes(int(np.prod(self.world.T)))
            addr = mem.empty(cap)
            assert addr % 16 == 0
            rec = self.det.world_export(kind, device=(addr, cap), allow=allow)
            rec = mem.get(addr, rec, dtype=np.uint8) if allow == () or rec not in allow else rec
            mem.free()
        else:
            rec = self.det.world_export(kind, allow=allow)
        if isinstance(rec, int):
            assert self.world.export(kind)[0] == rec
            return rec
        st, want, size = self.world.export(kind, new_gen=ws.gens(rec)[1])
        assert st == capi.OK and size == rec.size
        assert ws.gens(rec)[1] != 0 and (kind == FULL) == (ws.gens(rec)[0] == 0)
        np.testing.assert_array_equal(rec[:128], want[:128], err_msg="header")
        assert rec.tobytes() == want.tobytes()
        return rec

    def apply(self, rec, allow=()):
        want = self.world.apply(rec)
        st = self.det.world_apply(rec, allow=allow)
        assert st == want, self.det.lib.last_error_string(self.det.h)
        return st

    def state(self):
        return _snapshot_state(self.det), _world_state(self.det)

    def assert_unchanged(self, before, what):
        _assert_unchanged(self.det, before[0], what)
        _assert_world_unchanged(self.det, before[1], what)


def _far_points(r, n):
    """n a-priori points beyond the window, each in a tile of its own (the tile grid is anchored at box_lo = -LO)"""
    off = np.array(r.det.map_offset, dtype=np.float64)
    sx, sy, sz = r.S
    g = [(sx + 2, 5, 3), (sx + 10, 5, 3), (sx + 18, 5, 3), (sx + 26, 5, 3), (sx + 2, sy + 4, 3)][:n]
    tiles = {tuple((np.array(c) + np.array(LO)) // 8) for c in g}
    assert len(tiles) == n
    return (off + (np.array(g, dtype=np.float64).reshape(-1, 3) + 0.5) * r.vs).astype(np.float32)


def _same_world(a, b, what=""):
    """two handles hold the same world: world_info but tiles_cap, and vofod_world_read over the whole box"""
    ia, ib = wc.info_dict(a.det), wc.info_dict(b.det)
    assert {**ia, "tiles_cap": 0} == {**ib, "tiles_cap": 0}, what
    lo, ext = a.world.lo, a.world.hi - a.world.lo
    np.testing.assert_array_equal(a.det.world_read(lo, ext).view(np.uint32), b.det.world_read(lo, ext).view(np.uint32), err_msg=what)


# ------------------------------------------------------------------------------------------------ 1. full export bytes
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5])
def test_full_export_with_n_tiles_covers_the_index_padding(hip, n):
    r = SRig(hip, "21x13x9", seed=n)
    if n:
        assert r.load(_far_points(r, n)) == capi.OK
    rec = r.export(FULL)
    assert ws.n_tiles(rec) == n and rec.size == 128 + 4 * (-(-n // 4) * 4) + 2048 * n
    dev = r.export(FULL, device=True)  # host and device memspace: the same bytes but the generation
    np.testing.assert_array_equal(np.delete(dev, np.s_[48:64]), np.delete(rec, np.s_[48:64]))
    assert r.export(DELTA).size == 128
    r.check()


@pytest.mark.parametrize("which,pool", [("21x13x9", "ample"), ("21x13x9", "tight"), ("121x81x33", "tight")])
def test_full_export_after_shifts_and_a_far_sheet_is_the_statements(hip, which, pool):
    S = SIZES[which][1]
    total = wc.tile_count(S, LO, HI)
    r = SRig(hip, which, max_tiles=total if pool == "ample" else max(total // 8, 1), seed=len(which) + len(pool))
    r.fill()
    seen = np.zeros(0, dtype=np.uint32)
    for n, s in enumerate([(3, 0, 0), (-5, 4, -2), (0, -S[1], 0), (2, -3, 1), (-(S[0] - 1), 0, 0)]):
        assert r.shift(s) == capi.OK
        if n == 1 and which == "21x13x9":
            assert r.load(_sheet_and_wall(r)[0], allow=(capi.ERR_CAPACITY,)) == (capi.OK if pool == "ample" else capi.ERR_CAPACITY)  # (the statement's answer: load asserts it)
        if n % 2 == 1:
            r.fill((V,), density=0.5)
        rec = r.export(FULL)
        seen = np.union1d(seen, rec[128 + 4 * (-(-ws.n_tiles(rec) // 4) * 4):].view(np.uint32))
    r.check()
    i = r.world.info()
    assert i["tiles_used"] > 4 and (i["shifts_short_of_tiles"] > 0) == (pool == "tight")
    for pattern in (0x7F800000, 0x80000000, 0x7FC01234, 0xFFC00001):  # +inf, -0.0f and NaN payloads travel bit for bit
        assert pattern in seen
    # a buffer one byte short: VOFOD_ERR_CAPACITY, the size reported, and the next delta is what it would have been
    r.fill((V,))
    for s in [(1, 2, 0), (S[0] - 1, 0, 0), (0, S[1] - 1, 0), (S[0], S[1], 0)]:  # the first that writes into the store where the walk has ended
        probe = copy.deepcopy(r.world)
        probe.shift(r.bits[V], s)
        if probe.export(DELTA)[2] > 128:
            break
    assert r.shift(s) == capi.OK
    n = C.c_size_t(0)
    assert r.det.lib.world_export(r.det.h, DELTA, None, 0, capi.MEM_HOST, C.byref(n)) == capi.OK  # the size query
    size = n.value
    assert size > 128
    buf = np.zeros(size, dtype=np.uint8)
    n = C.c_size_t(0)
    assert r.det.lib.world_export(r.det.h, DELTA, capi.ptr(buf), size - 1, capi.MEM_HOST, C.byref(n)) == capi.ERR_CAPACITY
    assert n.value == size and not buf.any()
    assert r.world.export(DELTA, cap=size - 1) == (capi.ERR_CAPACITY, None, size)
    assert r.export(DELTA).size == size
    assert r.export(DELTA).size == 128


# ------------------------------------------------------------------------------------------------ 2. full apply onto a second handle
@pytest.mark.parametrize("which", ["21x13x9", "121x81x33"])
def test_full_apply_onto_a_second_handle(hip, which):
    S = SIZES[which][1]
    total = wc.tile_count(S, LO, HI)
    a = SRig(hip, which, max_tiles=total, seed=21)
    a.fill()
    for s in [(4, -2, 1), (-7, 0, 2), (0, 5, -3)]:
        assert a.shift(s) == capi.OK
        a.fill((V,), density=0.6)
    rec = a.export(FULL)
    n = ws.n_tiles(rec)
    assert n > 4
    # the second handle is created where the owner's window is now: its own origin starts at 0 and becomes the owner's
    b = SRig(hip, which, max_tiles=n + 3, offset=mc.shifted_offset(BASE, a.k, a.vs), seed=22)
    assert tuple(a.k) != (0, 0, 0) and wc.info_dict(b.det)["origin"] == (0, 0, 0)
    assert b.apply(rec) == capi.OK
    b.check("after the world snapshot")
    assert wc.info_dict(b.det)["origin"] == tuple(int(v) for v in a.k) and wc.info_dict(b.det)["tiles_cap"] == n + 3
    b.det.apply_map(a.det.export_map(capi.MAPS_ALL, True))  # the window snapshot
    for w in mc.MAPS:
        b.bits[w] = a.bits[w].copy()
    b.check("after the window snapshot")
    _same_world(a, b, "restored")
    # the same further shifts on both: windows, store and counters stay equal (the follower's pool has three tiles to spare)
    for s in [(2, 0, 0), (-3, 1, 0), (1, -2, 1)]:
        fill = mc.random_bits(a.rng, S[::-1])
        for r in (a, b):
            r.write(V, fill)
            assert r.shift(s) == capi.OK
            r.check(f"shift {s}")
        if a.world.short == b.world.short:  # (with a tile short on one side only the stores part, as they must)
            _same_world(a, b, f"shift {s}")
    # a device buffer is applied as the host's bytes are
    c = SRig(hip, which, max_tiles=total, offset=mc.shifted_offset(BASE, a.k, a.vs), seed=23)
    assert c.apply(a.export(FULL)) == capi.OK
    mem = DeviceMem()
    addr = mem.empty(ws.nbytes(total))
    size = a.det.world_export(FULL, device=(addr, ws.nbytes(total)))
    d = SRig(hip, which, max_tiles=total, offset=mc.shifted_offset(BASE, a.k, a.vs), seed=24)
    assert d.det.world_apply((addr, size)) == capi.OK
    mem.free()
    assert wc.info_dict(c.det) == wc.info_dict(d.det)
    _same_world(c, d, "device buffer")
    # a handle whose window sits elsewhere: the displacement d of the header's formula is not zero, its origin is the owner's plus d
    disp = np.array([2, -1, 1])
    e = SRig(hip, which, max_tiles=total, offset=mc.shifted_offset(BASE, a.k + disp, a.vs), seed=25)
    assert e.apply(a.export(FULL)) == capi.OK
    e.check("d != 0")
    assert wc.info_dict(e.det)["origin"] == tuple(int(v) for v in a.k + disp)
    assert {**wc.info_dict(e.det), "origin": 0} == {**wc.info_dict(a.det), "origin": 0}
    lo, ext = a.world.lo, a.world.hi - a.world.lo
    wa, we = a.det.world_read(lo, ext).view(np.uint32), e.det.world_read(lo, ext).view(np.uint32)
    g = np.indices(wa.shape)[::-1] + lo.reshape(3, 1, 1, 1)
    outside = ~a.world._in_window(g, a.world.K) & ~e.world._in_window(g, e.world.K)
    np.testing.assert_array_equal(we[outside], wa[outside])


# ------------------------------------------------------------------------------------------------ 3. a chain of deltas
def _chain_shifts(S):
    return [(1, 0, 0), (-1, 0, 0), (3, 0, 0), (0, -3, 0), (2, -3, 1), (-5, 4, -2), (S[0] - 1, 0, 0), (0, S[1], 0), (-(S[0] + 2), 0, 1), (0, -1, -(S[2] + 1))]


@pytest.mark.parametrize("which,pool", [("21x13x9", "ample"), ("21x13x9", "tight"), ("121x81x33", "ample")])
def test_delta_chain_on_a_follower_that_never_shifts(hip, which, pool):
    S = SIZES[which][1]
    total = wc.tile_count(S, LO, HI)
    a = SRig(hip, which, max_tiles=total if pool == "ample" else max(total // 8, 1), seed=31)
    d = (2, -1, 1)  # the follower's window sits elsewhere: its origin is the owner's plus d, whatever the owner does
    b = SRig(hip, which, max_tiles=total + 1, offset=mc.shifted_offset(BASE, d, a.vs), seed=32)
    a.fill()
    records = [a.export(FULL)]
    assert b.apply(records[0]) == capi.OK
    assert wc.info_dict(b.det)["origin"] == d
    lo, ext = a.world.lo, a.world.hi - a.world.lo
    for n, s in enumerate(_chain_shifts(S)):
        assert a.shift(s) == capi.OK
        if n % 2 == 0:
            a.fill((V,), density=0.5)
        rec = a.export(DELTA)
        records.append(rec)
        assert ws.gens(rec)[0] == ws.gens(records[-2])[1]
        assert b.apply(rec) == capi.OK
        assert wc.info_dict(b.det)["origin"] == d
        b.check(f"delta {n} {s}")
        # W outside both windows: the owner's
        wa, wb = a.det.world_read(lo, ext).view(np.uint32), b.det.world_read(lo, ext).view(np.uint32)
        g = np.indices(wa.shape)[::-1] + lo.reshape(3, 1, 1, 1)
        outside = ~a.world._in_window(g, a.world.K) & ~b.world._in_window(g, b.world.K)
        np.testing.assert_array_equal(wb[outside], wa[outside], err_msg=f"delta {n} {s}")
        assert {**wc.info_dict(b.det), "tiles_cap": 0, "origin": 0} == {**wc.info_dict(a.det), "tiles_cap": 0, "origin": 0}
    assert a.world.used > 4 and (a.world.short > 0) == (pool == "tight")
    assert max(ws.n_tiles(r) for r in records[1:]) > 0 and any(0 < ws.n_tiles(r) < a.world.used for r in records[1:])
    # the same chain replayed from its bytes on a fresh handle
    c = SRig(hip, which, max_tiles=total, offset=mc.shifted_offset(BASE, d, a.vs), seed=33)
    for rec in records:
        assert c.apply(rec.tobytes()) == capi.OK
    c.check("replayed")
    _same_world(b, c, "replayed")


# ------------------------------------------------------------------------------------------------ 4. refusals change nothing
def test_refusals_change_nothing(hip):
    S = SIZES["21x13x9"][1]
    total = wc.tile_count(S, LO, HI)
    a = SRig(hip, "21x13x9", max_tiles=total, seed=41)
    a.fill()
    assert a.shift((3, -2, 1)) == capi.OK
    # store off
    off = SRig(hip, "21x13x9", max_tiles=False, offset=mc.shifted_offset(BASE, a.k, a.vs), seed=42)
    off.fill()
    full = a.export(FULL)
    while ws.n_tiles(full) % 4 == 0:  # (the damaged padding entry below needs one)
        a.fill((V,), density=0.7)
        assert a.shift(tuple(int(v) for v in a.rng.integers(-4, 5, size=3))) == capi.OK
        full = a.export(FULL)
    before = _snapshot_state(off.det)
    n = C.c_size_t(7)
    assert off.det.lib.world_export(off.det.h, FULL, None, 0, capi.MEM_HOST, C.byref(n)) == capi.ERR_NOT_PENDING
    assert off.det.world_apply(full, allow=(capi.ERR_NOT_PENDING,)) == capi.ERR_NOT_PENDING
    _assert_unchanged(off.det, before, "store off")
    assert wc.info_dict(off.det)["enabled"] == 0
    # a follower that holds the full snapshot; `delta` carries at least two tiles, `delta2` follows it
    a.fill((V,), density=0.7)
    assert a.shift((-5, 4, 2)) == capi.OK
    delta = a.export(DELTA)
    assert ws.n_tiles(delta) >= 2
    index = np.frombuffer(delta.tobytes(), dtype="<u4", count=ws.n_tiles(delta), offset=128)
    assert a.shift((1, 1, 0)) == capi.OK
    delta2 = a.export(DELTA)
    b = SRig(hip, "21x13x9", max_tiles=total, offset=mc.shifted_offset(BASE, (0, 0, 0), a.vs), seed=43)
    b.fill()
    assert b.apply(full) == capi.OK
    before = b.state()
    nf, nd = ws.n_tiles(full), ws.n_tiles(delta)
    i0, i1 = (int(v) for v in index[:2])
    E = capi
    cases = [
        ("magic", ws.patched(delta, "magic", "I", 0x444D4656), E.ERR_INVALID_ARG),
        ("version", ws.patched(delta, "version", "I", 2), E.ERR_INVALID_ARG),
        ("kind", ws.patched(delta, "kind", "I", 2), E.ERR_INVALID_ARG),
        ("length", delta[:-16], E.ERR_INVALID_ARG),
        ("shorter than a header", delta[:64], E.ERR_INVALID_ARG),
        ("reserved word", ws.patched(delta, "zero", "I", 1), E.ERR_INVALID_ARG),
        ("unsorted", ws.with_index(ws.with_index(delta, 0, i1), 1, i0), E.ERR_INVALID_ARG),
        ("repeated", ws.with_index(delta, 1, i0), E.ERR_INVALID_ARG),
        ("out of range", ws.with_index(delta, nd - 1, total), E.ERR_INVALID_ARG),
        ("padding", ws.with_index(full, nf, 0), E.ERR_INVALID_ARG),
        ("voxel size", ws.patched(delta, "voxel_size", "f", 0.25), E.ERR_SIZE_MISMATCH),
        ("half a voxel off", ws.patched(delta, "map_offset", "3f", *(np.frombuffer(delta.tobytes(), "<f4", 3, 28) + np.float32([a.vs / 2, 0, 0]))), E.ERR_SIZE_MISMATCH),
        ("a skipped delta", delta2, E.ERR_DELTA_BASE),
    ]
    for what, rec, want in cases:
        assert b.apply(rec, allow=(want,)) == want, what
        b.assert_unchanged(before, what)
    # other margins
    m = SRig(hip, "21x13x9", max_tiles=total + 500, lo=(LO[0] + 1, LO[1], LO[2]), hi=HI, seed=44)
    mb = m.state()
    assert m.apply(full, allow=(E.ERR_SIZE_MISMATCH,)) == E.ERR_SIZE_MISMATCH
    m.assert_unchanged(mb, "other margins")
    # a pool one tile short: the full snapshot on a fresh handle, the delta on a follower that holds the full one
    t = SRig(hip, "21x13x9", max_tiles=nf - 1, seed=45)
    t.fill()
    tb = t.state()
    assert t.apply(full, allow=(E.ERR_CAPACITY,)) == E.ERR_CAPACITY
    t.assert_unchanged(tb, "full, one tile short")
    st, _, _, _, _, fresh = b.world.check(delta)
    assert st == E.OK and fresh >= 1
    u = SRig(hip, "21x13x9", max_tiles=nf + fresh - 1, seed=46)
    assert u.apply(full) == E.OK
    ub = u.state()
    assert u.apply(delta, allow=(E.ERR_CAPACITY,)) == E.ERR_CAPACITY
    u.assert_unchanged(ub, "delta, one tile short")
    # a misaligned device buffer
    mem = DeviceMem()
    addr = mem.put(delta, shift=4)
    assert b.det.world_apply((addr, delta.size), allow=(E.ERR_INVALID_ARG,)) == E.ERR_INVALID_ARG
    assert b.det.world_export(FULL, device=(addr, delta.size), allow=(E.ERR_INVALID_ARG,)) == E.ERR_INVALID_ARG
    mem.free()
    b.assert_unchanged(before, "misaligned")
    # after all that the chain still holds
    assert b.apply(delta) == E.OK and b.apply(delta2) == E.OK
    b.check("the chain after the refusals")


def test_a_batch_in_flight_refuses_apply_and_admits_export(hip):
    dev = mc.make_det(hip)
    dev.load_apriori(mc.ground_apriori())
    sc = mc.scans(mc.TARGET_IN_AREA, 0, 2)
    dev.process_scan(sc[0].scan, sc[0].tf)
    assert dev.world_enable(LO, HI, 4096) == capi.OK
    base = tuple(dev.sp.oparea_offset)
    assert dev.map_shift((3, 0, 0), mc.shifted_offset(base, (3, 0, 0), mc.VS)) == capi.OK
    full = dev.world_export(FULL)
    assert ws.n_tiles(full) > 0
    before, wbefore = _snapshot_state(dev), _world_state(dev)
    t = dev.batch_submit([sc[1].scan], sc[1].tf[None])
    assert dev.world_apply(full, allow=(capi.ERR_BUSY,)) == capi.ERR_BUSY
    delta = dev.world_export(DELTA)  # export only reads the store: admitted like vofod_map_export
    assert delta.size == 128
    dev.batch_collect(t)
    _assert_unchanged(dev, (before[0], mc.status_tuple(dev)), "ticket in flight")
    _assert_world_unchanged(dev, wbefore, "ticket in flight")
    assert dev.world_apply(full) == capi.OK
    _assert_world_unchanged(dev, wbefore, "its own snapshot")


# ------------------------------------------------------------------------------------------------ 5. what ends a chain
def test_chain_enders(hip):
    S = SIZES["21x13x9"][1]
    total = wc.tile_count(S, LO, HI)
    a = SRig(hip, "21x13x9", max_tiles=total, seed=51)
    a.fill()
    B = capi.ERR_DELTA_BASE
    assert a.export(DELTA, allow=(B,)) == B  # no chain yet
    assert a.shift((4, 0, -1)) == capi.OK
    full = a.export(FULL)
    # the owner: reset, disable / enable, an apply on itself
    a.det.reset()
    a.world.reset()
    for w in mc.MAPS:
        a.bits[w] = np.full(a.S[::-1], a.init[w], dtype=np.uint32)
    assert a.export(DELTA, allow=(B,)) == B
    a.export(FULL)
    K = a.world.K.copy()
    assert a.det.world_disable() == capi.OK
    a.enable(total)
    a.k[:] = 0  # (K starts again at the offset the window has now)
    a.base = tuple(a.det.sp.oparea_offset)
    assert a.export(DELTA, allow=(B,)) == B
    a.fill()
    assert a.shift((-2, 3, 0)) == capi.OK
    full = a.export(FULL)
    assert a.export(DELTA).size == 128
    assert a.apply(full) == capi.OK
    assert a.export(DELTA, allow=(B,)) == B
    a.check("the owner")
    # the follower: its own shift or a-priori load ends the applied chain, a full snapshot repairs it
    b = SRig(hip, "21x13x9", max_tiles=total, offset=tuple(a.det.sp.oparea_offset), seed=52)
    assert b.apply(a.export(FULL)) == capi.OK
    a.fill((V,))
    assert a.shift((1, 0, 0)) == capi.OK
    delta = a.export(DELTA)
    assert b.shift((0, 1, 0)) == capi.OK
    before = b.state()
    assert b.apply(delta, allow=(B, capi.ERR_SIZE_MISMATCH)) in (B, capi.ERR_SIZE_MISMATCH)  # (its origin has moved too: the statement says which)
    b.assert_unchanged(before, "after the follower's shift")
    assert b.shift((0, -1, 0)) == capi.OK
    before = b.state()
    assert b.apply(delta, allow=(B,)) == B
    b.assert_unchanged(before, "back at the old origin")
    assert b.apply(a.export(FULL)) == capi.OK
    assert a.shift((0, 0, 1)) == capi.OK
    assert b.apply(a.export(DELTA)) == capi.OK
    assert b.load(_far_points(b, 2)) == capi.OK
    assert a.shift((0, 0, -1)) == capi.OK
    delta = a.export(DELTA)
    before = b.state()
    assert b.apply(delta, allow=(B,)) == B
    b.assert_unchanged(before, "after the follower's a-priori load")
    assert b.apply(a.export(FULL)) == capi.OK
    b.check("repaired")
    # the rule has no exception: a shift that moves nothing and a cloud of no points end the applied chain as well
    for what, call in (("a shift by zero", lambda: b.shift((0, 0, 0))), ("a cloud of zero points", lambda: b.load(np.zeros((0, 3), dtype=np.float32)))):
        assert a.shift((1, 0, 0)) == capi.OK
        delta = a.export(DELTA)
        assert call() == capi.OK
        before = b.state()
        assert b.apply(delta, allow=(B,)) == B, what
        b.assert_unchanged(before, what)
        assert b.apply(a.export(FULL)) == capi.OK
    b.check("repaired again")


# ------------------------------------------------------------------------------------------------ 6. larger geometry
def test_larger_geometry_full_delta_and_a_mixed_apply(hip):
    S = SIZES["121x81x33"][1]
    total = wc.tile_count(S, BIG_LO, BIG_HI)
    assert total >= 3000
    a = SRig(hip, "121x81x33", max_tiles=total, lo=BIG_LO, hi=BIG_HI, seed=61)
    b = SRig(hip, "121x81x33", max_tiles=1500, lo=BIG_LO, hi=BIG_HI, seed=62)
    a.fill()
    assert a.shift((S[0] + 3, 0, 0)) == capi.OK  # the whole window goes into the store
    full = a.export(FULL)
    assert ws.n_tiles(full) >= 600 and total // 64 > 4  # more than one workgroup's share of the directory, whatever its size
    assert b.apply(full) == capi.OK
    b.check("full")
    a.fill((V,), density=0.3)
    assert a.shift((-40, 30, -5)) == capi.OK  # tiles of the first trip change, and new ones are allocated
    delta = a.export(DELTA)
    idx = np.frombuffer(delta.tobytes(), dtype="<u4", count=ws.n_tiles(delta), offset=128)
    known = b.world.alloc.reshape(-1)[idx]
    assert known.any() and (~known).any() and 0 < ws.n_tiles(delta)
    assert b.apply(delta) == capi.OK
    b.check("delta: new and existing tiles mixed")
    np.testing.assert_array_equal(b.world.tiles(), a.world.tiles())
    assert a.export(DELTA).size == 128
    a.check("the owner")


# ------------------------------------------------------------------------------------------------ 7. routes
def test_the_new_kernels_appear_under_their_names(hip):
    a = SRig(hip, "21x13x9", seed=71)
    a.fill()
    assert a.shift((3, 1, 0)) == capi.OK
    lib, det = a.det.lib, a.det
    lib.profile_enable(det.h, 1)
    profiled_calls(lib, det)
    full = a.export(FULL)  # a size query, then the export
    assert profiled_calls(lib, det) == {"k_world_select": 2, "k_gscan_a": 2, "k_gscan_b": 2, "k_gscan_c": 2, "k_world_emit": 1}
    assert a.shift((-1, 0, 2)) == capi.OK
    assert profiled_calls(lib, det) == {"k_map_shift": 3, "k_world_mark": 1, "k_world_claim": 1, "k_world_put": 1, "k_world_get": 1}  # the parent's launches
    a.export(DELTA)
    assert profiled_calls(lib, det) == {"k_world_select": 2, "k_gscan_a": 2, "k_gscan_b": 2, "k_gscan_c": 2, "k_world_emit": 1}
    assert a.apply(full) == capi.OK
    assert profiled_calls(lib, det) == {"k_world_check": 1, "k_world_scatter": 1}
    lib.profile_enable(det.h, 0)
