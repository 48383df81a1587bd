"""The numpy statement of the world snapshots (include/vofod.h, WORLD SNAPSHOTS) for test_world_sync_cpu.py and
test_gpu_world_sync.py, built on world_cases.World.

`SyncWorld` adds to the store's statement what vofod_world_export and vofod_world_apply add to the handle: a shadow of the tiles and of
`alloc` as the last export left them, the two chains, and the bytes of the wire format, packed here with `struct` and independent of the
product's codec (vofod_amd.mapsync).  Generations are random on the device, so `export` takes the generation to stamp; everything else
in a record is stated.  The padding voxels of the tiles on the box's upper faces (the box is no multiple of the tile edge) are init
until an applied snapshot says otherwise: they travel verbatim."""
from __future__ import annotations

import struct

import numpy as np

import world_cases as wc
from vofod_amd import capi

MAGIC = 0x44574656  # "VFWD"
VERSION = 1
HEADER_BYTES = 128
TILE_WORDS = wc.TILE ** 3
PAD = 0xFFFFFFFF
_HDR = struct.Struct("<4I3i3f2f2Q9iI3Q")
assert _HDR.size == HEADER_BYTES
# byte offsets of the header's fields, for the tests that damage one
OFF = dict(magic=0, version=4, kind=8, tile_edge=12, map_size=16, map_offset=28, voxel_size=40, score_init=44, base_gen=48, new_gen=56, K=64, box_lo=76, box_hi=88, zero=100, n=104,
           short=112, forgotten=120)


def nbytes(n: int) -> int:
    return HEADER_BYTES + 4 * (-(-n // 4) * 4) + 4 * TILE_WORDS * n


def gens(buf) -> tuple[int, int]:
    """(base_gen, new_gen) of a record"""
    return struct.unpack_from("<2Q", bytes(memoryview(np.ascontiguousarray(buf))[:64]), 48)


def n_tiles(buf) -> int:
    return struct.unpack_from("<Q", bytes(memoryview(np.ascontiguousarray(buf))[:128]), 104)[0]


def _f32_bits(v) -> bytes:
    return struct.pack("<f", float(np.float32(v)))


class SyncWorld(wc.World):
    def __init__(self, S, margin_lo, margin_hi, max_tiles: int, init_bits: int, map_offset, voxel_size):
        self.offset = np.array(list(map_offset), dtype=np.float32)  # the window's map offset (vofod_status_info); the caller moves it with the window
        self.vs = np.float32(voxel_size)
        super().__init__(S, margin_lo, margin_hi, max_tiles, init_bits)
        self.score_init = np.array([init_bits], dtype=np.uint32).view(np.float32)[0]

    # ------------------------------------------------------------------ state
    def reset(self):
        super().reset()
        self.pad = np.full(tuple(int(t) * wc.TILE for t in self.T[::-1]), self.init, dtype=np.uint32)  # read beyond the box only
        self.shadow = self.shadow_alloc = None  # (the device keeps its buffer; without a chain nobody reads it)
        self.chain_gen = self.applied_gen = 0

    def shift(self, window, s):
        out = super().shift(window, s)
        self.applied_gen = 0  # a writer other than apply
        return out

    def load_apriori(self, window, pts, map_offset, voxel_size):
        st, out = super().load_apriori(window, pts, map_offset, voxel_size)
        if st == capi.OK:
            self.applied_gen = 0
        return st, out

    # ------------------------------------------------------------------ tiles
    def _padded(self) -> np.ndarray:
        p = self.pad.copy()
        e = self.hi - self.lo
        p[: e[2], : e[1], : e[0]] = self.dense
        return p

    def _tile_view(self, padded: np.ndarray) -> np.ndarray:
        """[T2, 8, T1, 8, T0, 8] view of a padded box"""
        T = [int(t) for t in self.T]
        return padded.reshape(T[2], wc.TILE, T[1], wc.TILE, T[0], wc.TILE)

    def tiles(self) -> np.ndarray:
        """every tile of the box as the pool would hold it: [n_dir, 512], directory order, z / y / x inside the tile"""
        return np.ascontiguousarray(self._tile_view(self._padded()).transpose(0, 2, 4, 1, 3, 5)).reshape(-1, TILE_WORDS)

    # ------------------------------------------------------------------ export
    def export(self, kind: int, new_gen: int = 1, cap: int | None = None):
        """(status, bytes | None, size): vofod_world_export into a buffer of `cap` bytes (None: large enough)"""
        full = kind == capi.SNAPSHOT_FULL
        if not full and self.chain_gen == 0:
            return capi.ERR_DELTA_BASE, None, 0
        tiles = self.tiles()
        alloc = self.alloc.reshape(-1)
        if full:
            sel = alloc.copy()
        else:
            sel = alloc & (~self.shadow_alloc | (tiles != self.shadow).any(axis=1))
        idx = np.flatnonzero(sel).astype(np.uint32)
        n = int(idx.size)
        size = nbytes(n)
        if cap is not None and cap < size:
            return capi.ERR_CAPACITY, None, size
        hdr = _HDR.pack(MAGIC, VERSION, int(kind), wc.TILE, *(int(v) for v in self.S), *(float(v) for v in self.offset), float(self.vs), float(self.score_init),
                        0 if full else self.chain_gen, int(new_gen), *(int(v) for v in self.K), *(int(v) for v in self.lo), *(int(v) for v in self.hi), 0, n, self.short, self.forgotten)
        lst = np.full(-(-n // 4) * 4, PAD, dtype="<u4")
        lst[:n] = idx
        out = np.concatenate([np.frombuffer(hdr, dtype=np.uint8), lst.view(np.uint8), np.ascontiguousarray(tiles[idx], dtype="<u4").reshape(-1).view(np.uint8)])
        assert out.size == size
        if full or self.shadow is None:
            self.shadow = np.full_like(tiles, self.init)
            self.shadow_alloc = np.zeros_like(alloc)
        self.shadow[idx] = tiles[idx]
        self.shadow_alloc |= sel
        self.chain_gen = int(new_gen)
        return capi.OK, out, size

    # ------------------------------------------------------------------ apply
    def check(self, buf):
        """(status, header tuple, idx, tiles, K1, new tiles) of an incoming record, the checks in the header's order"""
        b = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else buf).view(np.uint8).reshape(-1)
        bad = (capi.ERR_INVALID_ARG, None, None, None, None, 0)
        if b.size < HEADER_BYTES:
            return bad
        h = _HDR.unpack(b[:HEADER_BYTES].tobytes())
        magic, version, kind, edge = h[0:4]
        size, off, vs, si, base_gen = h[4:7], h[7:10], h[10], h[11], h[12]
        K, lo, hi, zero, n = h[14:17], h[17:20], h[20:23], h[23], h[24]
        # 1. format
        if magic != MAGIC or version != VERSION or kind > 1 or edge != wc.TILE or zero != 0:
            return bad
        if n > 0xFFFFFFF0 or b.size != nbytes(n):
            return bad
        n4 = -(-n // 4) * 4
        lst = b[HEADER_BYTES : HEADER_BYTES + 4 * n4].view("<u4")
        idx = lst[:n].astype(np.int64)
        n_dir = int(np.prod(self.T))
        if (lst[n:] != PAD).any() or (idx >= n_dir).any() or (np.diff(idx) <= 0).any():
            return bad
        tiles = b[HEADER_BYTES + 4 * n4 :].view("<u4").reshape(n, TILE_WORDS)
        # 2. geometry
        mismatch = (capi.ERR_SIZE_MISMATCH, None, None, None, None, 0)
        if tuple(size) != tuple(int(v) for v in self.S) or _f32_bits(vs) != _f32_bits(self.vs) or _f32_bits(si) != _f32_bits(self.score_init):
            return mismatch
        if tuple(lo) != tuple(int(v) for v in self.lo) or tuple(hi) != tuple(int(v) for v in self.hi):
            return mismatch
        vsd = float(self.vs)
        gap = self.offset.astype(np.float64) - np.array(off, dtype=np.float32).astype(np.float64)
        d = np.rint(gap / vsd)
        K1 = np.array(K, dtype=np.float64) + d
        if not (np.abs(gap - d * vsd) < vsd / 4.0).all() or not (np.abs(K1) <= wc.K_LIMIT).all():
            return mismatch
        K1 = K1.astype(np.int64)
        if kind == capi.SNAPSHOT_DELTA and (K1 != self.K).any():
            return mismatch
        # 3. chain
        if kind == capi.SNAPSHOT_DELTA and (base_gen == 0 or base_gen != self.applied_gen):
            return (capi.ERR_DELTA_BASE, None, None, None, None, 0)
        # 4. capacity
        alloc = self.alloc.reshape(-1)
        fresh = n if kind == capi.SNAPSHOT_FULL else int((~alloc[idx]).sum())
        used = 0 if kind == capi.SNAPSHOT_FULL else self.used
        if used + fresh > self.cap:
            return (capi.ERR_CAPACITY, None, None, None, None, fresh)
        return capi.OK, h, idx, tiles, K1, fresh

    def apply(self, buf) -> int:
        """vofod_world_apply: the status; on anything but OK nothing has changed"""
        st, h, idx, tiles, K1, fresh = self.check(buf)
        if st != capi.OK:
            return st
        if h[2] == capi.SNAPSHOT_FULL:
            wc.World.reset(self)  # (the chains are set below)
            self.pad[...] = self.init
            self.K = K1
        p = self._padded()
        T0, T1 = int(self.T[0]), int(self.T[1])
        tx, ty, tz = idx % T0, (idx // T0) % T1, idx // (T0 * T1)
        self._tile_view(p)[tz, :, ty, :, tx, :] = tiles.reshape(-1, wc.TILE, wc.TILE, wc.TILE)
        e = self.hi - self.lo
        self.dense = np.ascontiguousarray(p[: e[2], : e[1], : e[0]])
        self.pad = p
        self.alloc.reshape(-1)[idx] = True
        self.used += fresh
        self.short, self.forgotten = int(h[25]), int(h[26])
        self.applied_gen = int(h[13])
        self.chain_gen = 0
        return capi.OK


def patched(buf, field: str, fmt: str, *vals) -> np.ndarray:
    """a copy of record `buf` with header field `field` (OFF) overwritten by struct format `fmt`"""
    out = np.array(np.frombuffer(bytes(memoryview(np.ascontiguousarray(buf))), dtype=np.uint8))
    raw = struct.pack("<" + fmt, *vals)
    out[OFF[field] : OFF[field] + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return out


def with_index(buf, k: int, value: int) -> np.ndarray:
    """a copy of record `buf` with entry k of its index list (padding included) set to `value`"""
    out = np.array(np.frombuffer(bytes(memoryview(np.ascontiguousarray(buf))), dtype=np.uint8))
    out[HEADER_BYTES + 4 * k : HEADER_BYTES + 4 * k + 4] = np.frombuffer(struct.pack("<I", value), dtype=np.uint8)
    return out


def state(w: SyncWorld):
    """everything an apply may change, for `refusals change nothing`"""
    return (w.dense.copy(), w.alloc.copy(), w.pad.copy(), tuple(int(k) for k in w.K), w.used, w.short, w.forgotten, w.applied_gen, w.chain_gen)


def assert_state_equal(a, b, what=""):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            np.testing.assert_array_equal(x, y, err_msg=what)
        else:
            assert x == y, what
