"""The numpy statement of the world store (include/vofod.h, WORLD STORE) for test_world_cpu.py and test_gpu_world.py.

`World` is the contract written out: a dense uint32 array over the box plus a mask of allocated tiles.  The window itself stays with
the caller (what read_map returns, as uint32 [S2, S1, S0]); `shift` and `load_apriori` take it and return the new one.  Invariant:
a voxel of a tile that is not allocated holds init in the dense array, so W outside the window is the dense array as it stands.
All-or-nothing allocation makes every outcome independent of the order in which the device's atomics arrive."""
from __future__ import annotations

import numpy as np

import map_shift_cases as mc
from vofod_amd import capi

TILE = 8
K_LIMIT = 1 << 30
INF_BITS = 0x7F800000


def tile_count(S, margin_lo, margin_hi) -> int:
    return int(np.prod([-(-(int(s) + int(a) + int(b)) // TILE) for s, a, b in zip(S, margin_lo, margin_hi)]))


class World:
    def __init__(self, S, margin_lo, margin_hi, max_tiles: int, init_bits: int):
        self.S = np.array(S, dtype=np.int64)  # (sx, sy, sz)
        self.lo = -np.array(margin_lo, dtype=np.int64)
        self.hi = self.S + np.array(margin_hi, dtype=np.int64)
        self.T = -(-(self.hi - self.lo) // TILE)
        self.init = np.uint32(init_bits)
        self.cap = min(int(max_tiles), int(np.prod(self.T)))
        self.K = np.zeros(3, dtype=np.int64)
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        """vofod_reset: W is init everywhere; K, the box and the pool's size stay"""
        ext = self.hi - self.lo
        self.dense = np.full((ext[2], ext[1], ext[0]), self.init, dtype=np.uint32)
        self.alloc = np.zeros((self.T[2], self.T[1], self.T[0]), dtype=bool)
        self.used = self.short = self.forgotten = 0

    def info(self):
        """what vofod_world_status answers"""
        return dict(enabled=1, tile_edge=TILE, origin=tuple(int(k) for k in self.K), box_lo=tuple(int(v) for v in self.lo), box_hi=tuple(int(v) for v in self.hi),
                    tiles_used=self.used, tiles_cap=self.cap, shifts_short_of_tiles=self.short, voxels_forgotten=self.forgotten)

    # ------------------------------------------------------------------ helpers
    def _window_world(self, K):
        """world indices of the window's voxels: three arrays [S2, S1, S0] (x, y, z)"""
        sx, sy, sz = (int(v) for v in self.S)
        iz, iy, ix = np.indices((sz, sy, sx), dtype=np.int64)
        return ix + K[0], iy + K[1], iz + K[2]

    def _in_box(self, g):
        return (g[0] >= self.lo[0]) & (g[0] < self.hi[0]) & (g[1] >= self.lo[1]) & (g[1] < self.hi[1]) & (g[2] >= self.lo[2]) & (g[2] < self.hi[2])

    def _in_window(self, g, K):
        return (g[0] >= K[0]) & (g[0] < K[0] + self.S[0]) & (g[1] >= K[1]) & (g[1] < K[1] + self.S[1]) & (g[2] >= K[2]) & (g[2] < K[2] + self.S[2])

    def _cells(self, g, mask):
        """(dense index, tile index) of the world indices g[...][mask], all inside the box"""
        r = [(g[a][mask] - self.lo[a]) for a in range(3)]
        return (r[2], r[1], r[0]), (r[2] // TILE, r[1] // TILE, r[0] // TILE)

    def _want(self, tiles) -> int:
        """the tiles of `tiles` (index arrays) that are not allocated, as a set; allocates all of them or none.  Returns their number,
        negative when they did not fit."""
        lin = np.unique((tiles[0] * self.T[1] + tiles[1]) * self.T[0] + tiles[2])
        new = lin[~self.alloc.reshape(-1)[lin]]
        if self.used + len(new) > self.cap:
            return -len(new)
        self.alloc.reshape(-1)[new] = True
        self.used += len(new)
        return len(new)

    def wanted_by_shift(self, window: np.ndarray, s) -> int:
        """how many new tiles the write-back of shift(window, s) wants"""
        g = self._window_world(self.K)
        K1 = self.K + np.array(s, dtype=np.int64)
        want = ~self._in_window(g, K1) & self._in_box(g) & (window != self.init)
        _, tiles = self._cells(g, want)
        lin = np.unique((tiles[0] * self.T[1] + tiles[1]) * self.T[0] + tiles[2])
        return int((~self.alloc.reshape(-1)[lin]).sum())

    # ------------------------------------------------------------------ the calls
    def shift(self, window: np.ndarray, s) -> np.ndarray:
        """vofod_map_shift on the voxel map with the store enabled: steps 1 to 4 of the header"""
        window = np.asarray(window)
        assert window.dtype == np.uint32 and window.shape == (self.S[2], self.S[1], self.S[0])
        s = np.array(s, dtype=np.int64)
        K1 = self.K + s
        assert (np.abs(K1) <= K_LIMIT).all()
        # 1. write back
        g = self._window_world(self.K)
        leaving = ~self._in_window(g, K1)
        inbox = self._in_box(g)
        differs = window != self.init
        _, tiles = self._cells(g, leaving & inbox & differs)
        if self._want(tiles) < 0:
            self.short += 1
        cells, tiles = self._cells(g, leaving & inbox)
        has = self.alloc[tiles]
        vals = window[leaving & inbox]
        self.dense[tuple(c[has] for c in cells)] = vals[has]
        self.forgotten += int((leaving & ~inbox & differs).sum()) + int((~has & (vals != self.init)).sum())
        # 2. the map moves
        new = mc.shift_statement(window, tuple(int(v) for v in s), int(self.init))
        # 3. read in
        g1 = self._window_world(K1)
        entering = ~self._in_window(g1, self.K) & self._in_box(g1)
        cells, tiles = self._cells(g1, entering)
        has = self.alloc[tiles]
        sub = new[entering]
        sub[has] = self.dense[tuple(c[has] for c in cells)]
        new[entering] = sub
        # 4.
        self.K = K1
        return new

    @staticmethod
    def point_cells(pts, map_offset, voxel_size):
        """floor((p - off) * vs_inv) in float32, as k_apriori: [n, 3] float32 (not yet integers: a floor may be non-finite or huge)"""
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        off = np.array(list(map_offset), dtype=np.float32)
        vs_inv = np.float32(1.0) / np.float32(voxel_size)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.floor(((p - off).astype(np.float32) * vs_inv).astype(np.float32))

    def load_apriori(self, window: np.ndarray, pts, map_offset, voxel_size):
        """vofod_load_apriori with the store enabled: (status, window afterwards)"""
        f = self.point_cells(pts, map_offset, voxel_size)
        ok = np.isfinite(f).all(axis=1) & (np.abs(f) <= K_LIMIT).all(axis=1)
        c = f[ok].astype(np.int64)
        inwin = ((c >= 0) & (c < self.S)).all(axis=1)
        g = tuple(c[~inwin, a] + self.K[a] for a in range(3))
        far = self._in_box(g)
        cells, tiles = self._cells(g, far)
        if self._want(tiles) < 0:
            return capi.ERR_CAPACITY, window
        self.dense[cells] = INF_BITS
        out = window.copy()
        w = c[inwin]
        out[w[:, 2], w[:, 1], w[:, 0]] = INF_BITS
        return capi.OK, out

    def read(self, window: np.ndarray, lo, size) -> np.ndarray:
        """W over [lo, lo + size): uint32 [size2, size1, size0]"""
        lo = np.array(lo, dtype=np.int64)
        size = np.array(size, dtype=np.int64)
        out = np.full((size[2], size[1], size[0]), self.init, dtype=np.uint32)
        for src, base, ext in ((self.dense, self.lo, self.hi - self.lo), (window, self.K, self.S)):  # the window last: it wins
            a = np.maximum(lo, base)
            b = np.minimum(lo + size, base + ext)
            if (b > a).all():
                o, i = a - lo, a - base
                n = b - a
                out[o[2]:o[2] + n[2], o[1]:o[1] + n[1], o[0]:o[0] + n[0]] = src[i[2]:i[2] + n[2], i[1]:i[1] + n[1], i[0]:i[0] + n[0]]
        return out

    def read_box(self, window: np.ndarray) -> np.ndarray:
        return self.read(window, self.lo, self.hi - self.lo)


def info_dict(det) -> dict:
    """vofod_world_status of a detector in the shape of World.info()"""
    i = det.world_info()
    return dict(enabled=i.enabled, tile_edge=i.tile_edge, origin=tuple(i.origin), box_lo=tuple(i.box_lo), box_hi=tuple(i.box_hi), tiles_used=i.tiles_used, tiles_cap=i.tiles_cap,
                shifts_short_of_tiles=i.shifts_short_of_tiles, voxels_forgotten=i.voxels_forgotten)
