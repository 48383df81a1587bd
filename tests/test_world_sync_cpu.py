"""The world snapshots without a GPU: the numpy statement (world_sync_cases.SyncWorld) against records written out by hand, the
property the feature exists for - a full snapshot and its deltas, applied in order on a fresh store, give the owner's world - the
product's codec (vofod_amd.mapsync) against the statement's bytes, and every refusal of apply in the order include/vofod.h states."""
import struct

import numpy as np
import pytest

import map_shift_cases as mc
import world_cases as wc
import world_sync_cases as ws
from vofod_amd import capi, mapsync

I = 99  # init value of the hand-written cases
S = (5, 4, 3)
VS = 0.25
FULL, DELTA = capi.SNAPSHOT_FULL, capi.SNAPSHOT_DELTA


def _window():
    iz, iy, ix = np.indices((3, 4, 5))
    return (100 * iz + 10 * iy + ix + 1).astype(np.uint32)


def _world(max_tiles=8, offset=(1.0, 2.0, 3.0)):
    """the 5 x 4 x 3 window of test_world_cpu.py: box x in [-3, 7), tile 0 holds x in [-3, 5), tile 1 x in [5, 7)"""
    return ws.SyncWorld(S, (3, 0, 0), (2, 0, 0), max_tiles, I, offset, VS)


def _hand_header(kind, offset, base_gen, new_gen, K, n, short=0, forgotten=0):
    f32 = lambda v: struct.pack("<f", v)
    return (struct.pack("<4I", 0x44574656, 1, kind, 8) + struct.pack("<3i", 5, 4, 3) + b"".join(f32(v) for v in offset) + f32(0.25) + np.array([I], dtype="<u4").tobytes() +
            struct.pack("<2Q", base_gen, new_gen) + struct.pack("<3i", *K) + struct.pack("<3i", -3, 0, 0) + struct.pack("<3i", 7, 4, 3) + struct.pack("<I", 0) + struct.pack("<3Q", n, short, forgotten))


# ------------------------------------------------------------------------------------------------ hand-written records
def test_records_by_hand():
    w, a = _world(), _window()
    st, empty, size = w.export(FULL, new_gen=5)
    assert (st, size) == (capi.OK, 128) and empty.tobytes() == _hand_header(FULL, (1.0, 2.0, 3.0), 0, 5, (0, 0, 0), 0)  # nothing allocated: a header
    b = w.shift(a, (2, 0, 0))  # the columns x = 0, 1 left into tile 0
    w.offset = np.array([1.5, 2.0, 3.0], dtype=np.float32)
    st, rec, size = w.export(DELTA, new_gen=6)
    assert st == capi.OK and size == 128 + 16 + 2048 == rec.size
    tile0 = np.full((8, 8, 8), I, dtype="<u4")  # [z, y, x]: world x = -3 + x
    tile0[:3, :4, 3:5] = a[:, :, :2]
    want = _hand_header(DELTA, (1.5, 2.0, 3.0), 5, 6, (2, 0, 0), 1) + struct.pack("<4I", 0, ws.PAD, ws.PAD, ws.PAD) + tile0.tobytes()
    assert rec.tobytes() == want
    # an unchanged store: a delta of a header
    st, rec, size = w.export(DELTA, new_gen=7)
    assert (st, size) == (capi.OK, 128) and rec.tobytes() == _hand_header(DELTA, (1.5, 2.0, 3.0), 6, 7, (2, 0, 0), 0)
    # world x = 5, 6 take a value and leave into tile 1, whose x >= 2, y >= 4 and z >= 3 lie beyond box_hi: padding, init
    b[:, :, 3:] = 7
    w.shift(b, (-2, 0, 0))
    w.offset = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    st, rec, size = w.export(DELTA, new_gen=8)
    tile1 = np.full((8, 8, 8), I, dtype="<u4")
    tile1[:3, :4, :2] = 7
    assert rec.tobytes() == _hand_header(DELTA, (1.0, 2.0, 3.0), 7, 8, (0, 0, 0), 1) + struct.pack("<4I", 1, ws.PAD, ws.PAD, ws.PAD) + tile1.tobytes()
    # a full record carries both, in directory order; a tile whose words all equal init travels too
    b2 = w.shift(a, (2, 0, 0))
    b2[:] = I
    w.shift(b2, (-2, 0, 0))  # x = 5, 6 are init again: tile 1 is all init and still allocated
    st, rec, size = w.export(FULL, new_gen=9)
    assert size == 128 + 16 + 2 * 2048
    all_init = np.full((8, 8, 8), I, dtype="<u4")
    assert rec.tobytes() == _hand_header(FULL, (1.0, 2.0, 3.0), 0, 9, (0, 0, 0), 2) + struct.pack("<4I", 0, 1, ws.PAD, ws.PAD) + tile0.tobytes() + all_init.tobytes()


def test_delta_without_a_chain_and_the_chain_enders():
    w, a = _world(), _window()
    assert w.export(DELTA)[0] == capi.ERR_DELTA_BASE
    assert w.export(FULL, new_gen=3)[0] == capi.OK
    w.shift(a, (1, 0, 0))  # the owner's chain survives what it records
    assert w.export(DELTA, new_gen=4)[0] == capi.OK
    w.reset()
    assert w.export(DELTA)[0] == capi.ERR_DELTA_BASE
    st, rec, _ = w.export(FULL, new_gen=5)
    assert w.apply(rec) == capi.OK  # an apply on the owner itself
    assert w.export(DELTA)[0] == capi.ERR_DELTA_BASE
    # a buffer one byte short: nothing moves, the next delta is what it would have been
    w.export(FULL, new_gen=6)
    w.shift(a, (2, 0, 0))
    st, none, size = w.export(DELTA, new_gen=7, cap=128 + 16 + 2048 - 1)
    assert (st, none, size) == (capi.ERR_CAPACITY, None, 128 + 16 + 2048) and w.chain_gen == 6
    st, rec, _ = w.export(DELTA, new_gen=7)
    assert st == capi.OK and ws.gens(rec) == (6, 7) and ws.n_tiles(rec) == 1


def _move(owner, win, s, base):
    """the owner's shift with its map offset moved along: offset = base + K * voxel_size (K = 0 at base)"""
    win = owner.shift(win, s)
    owner.offset = (np.asarray(base) + owner.K * VS).astype(np.float32)
    return win


# ------------------------------------------------------------------------------------------------ the property
def _walk(seed, d, tight):
    """an owner that walks, refills its window and loads far points; a follower, `d` voxels away, that applies what the owner exports"""
    rng = np.random.default_rng(seed)
    S_, lo, hi = (7, 5, 4), (11, 6, 3), (9, 10, 5)
    init = 0x3F000000
    total = wc.tile_count(S_, lo, hi)
    base = np.array([-2.0, 1.0, 0.5])
    owner = ws.SyncWorld(S_, lo, hi, 5 if tight else total, init, base, VS)
    follower = ws.SyncWorld(S_, lo, hi, total, init, base + np.array(d) * VS, VS)
    return rng, owner, follower, base


@pytest.mark.parametrize("seed,d,tight", [(1, (0, 0, 0), False), (2, (3, -2, 1), False), (3, (-5, 0, 4), True)])
def test_full_and_deltas_applied_in_order_give_the_owners_world(seed, d, tight):
    rng, owner, follower, base = _walk(seed, d, tight)
    win = mc.random_bits(rng, (4, 5, 7))
    k = np.zeros(3, dtype=np.int64)
    records = []
    fresh = ws.SyncWorld(owner.S, -owner.lo, owner.hi - owner.S, 10**6, int(owner.init), follower.offset, VS)
    gen = 10
    for step in range(30):
        kind = FULL if step == 0 else DELTA
        st, rec, _ = owner.export(kind, new_gen=gen)
        gen += 1
        assert st == capi.OK
        records.append(rec)
        assert follower.apply(rec) == capi.OK
        # the follower holds the owner's world: tiles, allocation, counters; its origin is the owner's plus d and never moves with the owner
        np.testing.assert_array_equal(follower.tiles(), owner.tiles())
        np.testing.assert_array_equal(follower.alloc, owner.alloc)
        assert (follower.used, follower.short, follower.forgotten) == (owner.used, owner.short, owner.forgotten)
        assert tuple(follower.K) == tuple(np.array(d)) if step == 0 else True
        assert tuple(follower.K - np.array(d)) == (0, 0, 0)
        s = rng.integers(-6, 7, size=3)
        win = owner.shift(win, s)
        k += s
        owner.offset = (base + k * VS).astype(np.float32)
        if step % 3 == 1:
            win = mc.random_bits(rng, win.shape)
        if step % 7 == 4:
            pts = (owner.offset + (rng.integers(-12, 20, size=(9, 3)) + 0.5) * VS).astype(np.float32)
            st, win = owner.load_apriori(win, pts, owner.offset, VS)
    assert owner.used > 3 and (owner.short > 0) == tight
    # the same chain replayed from its bytes on a fresh store
    for rec in records:
        assert fresh.apply(rec.tobytes()) == capi.OK
    st, last, _ = owner.export(DELTA, new_gen=gen)
    assert fresh.apply(last) == capi.OK and follower.apply(last) == capi.OK
    np.testing.assert_array_equal(fresh.tiles(), owner.tiles())
    np.testing.assert_array_equal(fresh.dense, follower.dense)
    assert fresh.info() == {**follower.info(), "tiles_cap": fresh.cap}


def test_an_unchanged_store_exports_a_delta_of_128_bytes():
    rng, owner, _, base = _walk(4, (0, 0, 0), False)
    win = owner.shift(mc.random_bits(rng, (4, 5, 7)), (3, 1, -2))
    assert owner.export(FULL, new_gen=1)[2] > 128
    st, rec, size = owner.export(DELTA, new_gen=2)
    assert (st, size, rec.size) == (capi.OK, 128, 128)
    owner.shift(win, (0, 0, 0))  # nothing leaves
    assert owner.export(DELTA, new_gen=3)[2] == 128


# ------------------------------------------------------------------------------------------------ the product's codec
def test_codec_reads_and_writes_the_statements_bytes():
    rng, owner, _, base = _walk(5, (0, 0, 0), False)
    win = owner.shift(mc.random_bits(rng, (4, 5, 7)), (4, -3, 2))
    for n, (kind, move) in enumerate([(FULL, (-2, 1, 0)), (DELTA, (1, 1, 1)), (DELTA, (0, 0, 0))]):
        st, rec, size = owner.export(kind, new_gen=20 + n)
        s = mapsync.decode_world(rec)
        assert (s.kind, s.map_size, s.origin, s.box_lo, s.box_hi) == (kind, (7, 5, 4), tuple(owner.K), tuple(owner.lo), tuple(owner.hi))
        assert (s.base_gen, s.new_gen) == ((0 if kind == FULL else 19 + n), 20 + n) and s.voxel_size == VS and np.float32(s.score_init).view(np.uint32) == owner.init
        assert (s.shifts_short_of_tiles, s.voxels_forgotten) == (owner.short, owner.forgotten)
        assert s.map_offset == tuple(float(v) for v in owner.offset) and mapsync.world_nbytes(len(s.index)) == size
        np.testing.assert_array_equal(s.tiles, owner.tiles()[s.index])
        if len(s.index):
            d = int(s.index[0])
            T = s.tiles_per_axis
            assert s.tile_origin(0) == tuple(int(owner.lo[a]) + 8 * t for a, t in enumerate((d % T[0], d // T[0] % T[1], d // (T[0] * T[1]))))
        assert mapsync.encode_world(s).tobytes() == rec.tobytes()
        assert mapsync.decode_world(rec.tobytes()).new_gen == 20 + n  # bytes as well as arrays
        win = owner.shift(win, move)
    st, rec, _ = owner.export(FULL, new_gen=30)
    while ws.n_tiles(rec) % 4 == 0:  # (the damaged padding entry below needs one)
        win = owner.shift(mc.random_bits(rng, win.shape), rng.integers(-6, 7, size=3))
        st, rec, _ = owner.export(FULL, new_gen=30)
    assert ws.n_tiles(rec) >= 2
    for bad in [ws.patched(rec, "magic", "I", 0x444D4656), ws.patched(rec, "version", "I", 2), ws.patched(rec, "kind", "I", 2), ws.patched(rec, "tile_edge", "I", 4), ws.patched(rec, "zero", "I", 1),
                rec[:-1], rec[:100], np.concatenate([rec, rec[:4]]), ws.with_index(rec, 1, 0), ws.with_index(rec, 0, 10**6), ws.with_index(rec, -(-ws.n_tiles(rec) // 4) * 4 - 1, 7)]:
        with pytest.raises(ValueError):
            mapsync.decode_world(bad)
    assert mapsync.decode_world(ws.with_index(rec, 1, 0), check=False).kind == FULL


# ------------------------------------------------------------------------------------------------ refusals, in order
def test_every_refusal_of_apply_in_the_stated_order():
    rng, owner, follower, base = _walk(6, (0, 0, 0), False)
    win = _move(owner, mc.random_bits(rng, (4, 5, 7)), (4, -3, 2), base)
    st, full, _ = owner.export(FULL, new_gen=40)
    while ws.n_tiles(full) % 4 == 0:  # (the damaged padding entry below needs one)
        win = _move(owner, mc.random_bits(rng, win.shape), rng.integers(-3, 4, size=3), base)
        st, full, _ = owner.export(FULL, new_gen=40)
    at_full = owner.alloc.copy()
    while not (owner.alloc & ~at_full).any():  # (the capacity refusals below need a delta that allocates)
        win = _move(owner, mc.random_bits(rng, win.shape), rng.integers(-6, 7, size=3), base)
    st, delta, _ = owner.export(DELTA, new_gen=41)
    win = _move(owner, win, (3, 3, 1), base)
    st, delta2, _ = owner.export(DELTA, new_gen=42)
    n, nd = ws.n_tiles(full), ws.n_tiles(delta)
    assert n >= 3 and n % 4 != 0 and nd >= 2
    assert follower.apply(full) == capi.OK
    before = ws.state(follower)

    def refused(buf, want, what):
        assert follower.apply(buf) == want, what
        ws.assert_state_equal(ws.state(follower), before, what)

    E = capi
    # 1. format
    refused(full[:100], E.ERR_INVALID_ARG, "shorter than a header")
    refused(ws.patched(delta, "magic", "I", 0x444D4656), E.ERR_INVALID_ARG, "magic")
    refused(ws.patched(delta, "version", "I", 2), E.ERR_INVALID_ARG, "version")
    refused(ws.patched(delta, "kind", "I", 2), E.ERR_INVALID_ARG, "kind")
    refused(ws.patched(delta, "tile_edge", "I", 16), E.ERR_INVALID_ARG, "tile edge")
    refused(ws.patched(delta, "zero", "I", 1), E.ERR_INVALID_ARG, "reserved word")
    refused(delta[:-4], E.ERR_INVALID_ARG, "length")
    refused(ws.patched(delta, "n", "Q", nd + 1), E.ERR_INVALID_ARG, "n against the length")
    i0, i1 = (int(v) for v in mapsync.decode_world(delta).index[:2])
    refused(ws.with_index(ws.with_index(delta, 0, i1), 1, i0), E.ERR_INVALID_ARG, "unsorted")
    refused(ws.with_index(delta, 1, i0), E.ERR_INVALID_ARG, "repeated")
    refused(ws.with_index(delta, nd - 1, int(np.prod(follower.T))), E.ERR_INVALID_ARG, "out of range")
    refused(ws.with_index(full, n, 0), E.ERR_INVALID_ARG, "padding")
    # 2. geometry - in front of the chain: these deltas do not follow either
    skipped = delta2
    refused(ws.patched(skipped, "map_size", "3i", 7, 5, 5), E.ERR_SIZE_MISMATCH, "map size")
    refused(ws.patched(skipped, "voxel_size", "f", 0.5), E.ERR_SIZE_MISMATCH, "voxel size")
    refused(ws.patched(skipped, "score_init", "f", 0.25), E.ERR_SIZE_MISMATCH, "score_init")
    refused(ws.patched(skipped, "box_lo", "3i", -11, -6, -4), E.ERR_SIZE_MISMATCH, "box_lo")
    refused(ws.patched(skipped, "box_hi", "3i", 16, 15, 10), E.ERR_SIZE_MISMATCH, "box_hi")
    off = mapsync.decode_world(skipped).map_offset
    refused(ws.patched(skipped, "map_offset", "3f", off[0] + VS / 2, off[1], off[2]), E.ERR_SIZE_MISMATCH, "half a voxel off")
    refused(ws.patched(skipped, "map_offset", "3f", off[0] + VS, off[1], off[2]), E.ERR_SIZE_MISMATCH, "a delta whose origin is not the handle's")
    refused(ws.patched(full, "K", "3i", 2**30 + 100, 0, 0), E.ERR_SIZE_MISMATCH, "origin beyond 2^30")
    # ... and in front of format's refusals it is not: a bad magic with another voxel size is a bad magic
    refused(ws.patched(ws.patched(skipped, "voxel_size", "f", 0.5), "magic", "I", 1), E.ERR_INVALID_ARG, "format before geometry")
    # 3. chain - in front of capacity
    follower.cap = follower.used  # (a pool without a free tile, for the order alone)
    before = ws.state(follower)
    refused(skipped, E.ERR_DELTA_BASE, "a skipped delta")
    refused(ws.patched(delta, "base_gen", "Q", 0), E.ERR_DELTA_BASE, "base 0")
    # 4. capacity, all or nothing
    fresh = int((~follower.alloc.reshape(-1)[mapsync.decode_world(delta).index]).sum())
    assert fresh >= 1
    refused(delta, E.ERR_CAPACITY, "no free tile")
    follower.cap = follower.used + fresh - 1
    refused(delta, E.ERR_CAPACITY, "one tile short")
    small = ws.SyncWorld(owner.S, -owner.lo, owner.hi - owner.S, n - 1, int(owner.init), follower.offset, VS)
    assert small.apply(full) == E.ERR_CAPACITY and small.used == 0 and not small.alloc.any()
    follower.cap = follower.used + fresh
    assert follower.apply(delta) == E.OK and follower.apply(delta2) == E.OK
    np.testing.assert_array_equal(follower.tiles(), owner.tiles())
    # the follower's own writes end the applied chain; a full snapshot repairs it
    st, delta3, _ = owner.export(DELTA, new_gen=43)
    follower.shift(mc.random_bits(rng, (4, 5, 7)), (0, 0, 0))
    assert follower.apply(delta3) == E.ERR_DELTA_BASE
    follower.cap = 10**6
    st, full2, _ = owner.export(FULL, new_gen=44)
    assert follower.apply(full2) == E.OK
    st, delta4, _ = owner.export(DELTA, new_gen=45)
    follower.load_apriori(mc.random_bits(rng, (4, 5, 7)), np.array([[100.0, 100.0, 100.0]], dtype=np.float32), follower.offset, VS)
    assert follower.apply(delta4) == E.ERR_DELTA_BASE
    follower.reset()
    assert follower.apply(delta4) == E.ERR_DELTA_BASE
