"""The wire format of the map snapshots and deltas (include/vofod.h, vofod_map_export / vofod_map_apply) in plain numpy.

Independent of the library: `encode` builds the bytes the library writes, `decode` reads and checks them.  Little endian: a
128-byte header, then for each selected map (voxels, flags, raycast in that order) u32 idx[n] followed by u32 bits[n].
Byte 112, the first of the header's 16 reserved bytes, holds S + 1 when the snapshot carries a pending EXACT raycast pass with the
raycast map in its mask (include/vofod.h, EXACT RAYCAST ACCUMULATION: the raycast records are then uint32 units, 2^S per metre) and
0 otherwise; the other 15 are zero.  `Snapshot.raycast_log2_units` carries it (None: no such pass).

The world store travels in a format of its own (vofod_world_export / vofod_world_apply): `WorldSnapshot`, `encode_world`,
`decode_world` at the end of this module.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

MAGIC = 0x444D4656  # "VFMD"
VERSION = 1
HEADER_BYTES = 128
KIND_DELTA, KIND_FULL = 0, 1
MAP_VOXELS, MAP_FLAGS, MAP_RAYCAST = 0, 1, 2
MAPS_ALL = (1 << MAP_VOXELS) | (1 << MAP_FLAGS) | (1 << MAP_RAYCAST)

HEADER = np.dtype(
    {
        "names": ["magic", "version", "maps", "kind", "map_size", "map_offset", "voxel_size", "score_init", "base_gen", "new_gen", "detection_its",
                  "last_detection_id", "background_pts_sufficient", "sure_background_sufficient", "raycast_pending", "raycast_start_its", "n_records", "zero"],
        "formats": ["<u4", "<u4", "<u4", "<u4", ("<i4", 3), ("<f4", 3), "<f4", "<f4", "<u8", "<u8", "<i4", "<u4", "<i4", "<i4", "<i4", "<i4", ("<u8", 3), ("u1", 16)],
        "offsets": [0, 4, 8, 12, 16, 28, 40, 44, 48, 56, 64, 68, 72, 76, 80, 84, 88, 112],
        "itemsize": HEADER_BYTES,
    }
)

STATE_FIELDS = ("detection_its", "last_detection_id", "background_pts_sufficient", "sure_background_sufficient", "raycast_pending", "raycast_start_its")


@dataclass
class Snapshot:
    maps: int
    kind: int
    map_size: tuple
    map_offset: tuple
    voxel_size: float
    score_init: float
    base_gen: int = 0
    new_gen: int = 0
    detection_its: int = 0
    last_detection_id: int = 0
    background_pts_sufficient: int = 0
    sure_background_sufficient: int = 0
    raycast_pending: int = 0
    raycast_start_its: int = 0
    raycast_log2_units: int | None = None  # S of a pending exact raycast pass whose units travel in the raycast records; None: floats
    records: dict = field(default_factory=dict)  # map -> (idx uint32[n], bits uint32[n]) for every selected map

    @property
    def n_voxels(self) -> int:
        return int(np.prod(np.asarray(self.map_size, dtype=np.int64)))


def nbytes(counts) -> int:
    """size of a snapshot with these record counts"""
    return HEADER_BYTES + 8 * int(sum(int(c) for c in counts))


def init_bits(which: int, score_init: float) -> np.uint32:
    """bit pattern of a map's init state: score_init for the voxel map, 0.0f for flags and raycast"""
    v = np.float32(score_init if which == MAP_VOXELS else 0.0)
    return v.view(np.uint32)


def diff_records(cur: np.ndarray, base) -> tuple[np.ndarray, np.ndarray]:
    """(idx, bits) of the voxels of float32 map `cur` whose bits differ from `base`: a float32 map of the same size, or the
    uint32 bit pattern of an init state (init_bits)"""
    c = np.ascontiguousarray(cur, dtype=np.float32).reshape(-1).view(np.uint32)
    b = np.ascontiguousarray(base, dtype=np.float32).reshape(-1).view(np.uint32) if np.ndim(base) else np.uint32(base)
    idx = np.flatnonzero(c != b).astype(np.uint32)
    return idx, c[idx]


def encode(s: Snapshot) -> np.ndarray:
    """the bytes of snapshot `s` (uint8)"""
    h = np.zeros(1, dtype=HEADER)
    h["magic"], h["version"], h["maps"], h["kind"] = MAGIC, VERSION, s.maps, s.kind
    h["map_size"], h["map_offset"] = np.asarray(s.map_size, dtype=np.int32), np.asarray(s.map_offset, dtype=np.float32)
    h["voxel_size"], h["score_init"], h["base_gen"], h["new_gen"] = s.voxel_size, s.score_init, s.base_gen, s.new_gen
    for k in STATE_FIELDS:
        h[k] = getattr(s, k)
    parts = []
    counts = [0, 0, 0]
    for m in range(3):
        if not (s.maps >> m) & 1:
            continue
        idx, bits = s.records.get(m, (np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
        idx = np.ascontiguousarray(idx, dtype="<u4")
        bits = np.ascontiguousarray(bits, dtype="<u4") if np.asarray(bits).dtype != np.float32 else np.ascontiguousarray(bits, dtype="<f4").view("<u4")
        assert idx.shape == bits.shape
        counts[m] = idx.size
        parts += [idx.view(np.uint8), bits.view(np.uint8)]
    h["n_records"] = counts
    if s.raycast_log2_units is not None:
        if not (s.raycast_pending and (s.maps >> MAP_RAYCAST) & 1 and 0 <= int(s.raycast_log2_units) <= 24):
            raise ValueError("map snapshot: raycast_log2_units needs a pending pass, the raycast map in the mask and S in [0, 24]")
        h["zero"][0, 0] = int(s.raycast_log2_units) + 1
    return np.concatenate([h.view(np.uint8).reshape(-1)] + parts)


def decode(buf, check: bool = True) -> Snapshot:
    """parse a snapshot; ValueError on a bad magic / version / length / mask, or (check) indices not strictly ascending or >= M"""
    b = np.frombuffer(memoryview(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if b.size < HEADER_BYTES:
        raise ValueError(f"map snapshot: {b.size} bytes, shorter than the {HEADER_BYTES}-byte header")
    h = b[:HEADER_BYTES].view(HEADER)[0]
    if int(h["magic"]) != MAGIC:
        raise ValueError(f"map snapshot: bad magic {int(h['magic']):#x}")
    if int(h["version"]) != VERSION:
        raise ValueError(f"map snapshot: unknown version {int(h['version'])}")
    maps, kind = int(h["maps"]), int(h["kind"])
    if maps == 0 or maps & ~MAPS_ALL or kind not in (KIND_DELTA, KIND_FULL):
        raise ValueError(f"map snapshot: bad maps mask {maps} or kind {kind}")
    counts = [int(c) for c in h["n_records"]]
    if any(counts[m] and not (maps >> m) & 1 for m in range(3)):
        raise ValueError("map snapshot: records for a map outside the mask")
    if b.size != nbytes(counts):
        raise ValueError(f"map snapshot: {b.size} bytes, the header asks for {nbytes(counts)}")
    s = Snapshot(maps=maps, kind=kind, map_size=tuple(int(v) for v in h["map_size"]), map_offset=tuple(float(v) for v in h["map_offset"]),
                 voxel_size=float(h["voxel_size"]), score_init=float(h["score_init"]), base_gen=int(h["base_gen"]), new_gen=int(h["new_gen"]))
    for k in STATE_FIELDS:
        setattr(s, k, int(h[k]))
    tag = int(h["zero"][0])
    if np.any(h["zero"][1:]) or (tag and not (s.raycast_pending and (maps >> MAP_RAYCAST) & 1 and tag <= 25)):
        raise ValueError("map snapshot: reserved header bytes are not zero (byte 112 may hold S + 1 of a pending exact raycast pass)")
    s.raycast_log2_units = tag - 1 if tag else None
    off = HEADER_BYTES
    n_vox = s.n_voxels
    for m in range(3):
        if not (maps >> m) & 1:
            continue
        n = counts[m]
        idx = b[off : off + 4 * n].view("<u4").copy()
        bits = b[off + 4 * n : off + 8 * n].view("<u4").copy()
        off += 8 * n
        if check and n and (np.any(idx[1:] <= idx[:-1]) or int(idx[-1]) >= n_vox):
            raise ValueError(f"map snapshot: indices of map {m} not strictly ascending or outside the map")
        s.records[m] = (idx, bits)
    return s


def apply_to(s: Snapshot, maps: dict) -> dict:
    """what applying `s` does to plain arrays: `maps` {which: float32 array of M} -> the new arrays (numpy statement of the
    library's apply; a full snapshot starts from the init state)"""
    out = dict(maps)
    for m, (idx, bits) in s.records.items():
        if s.kind == KIND_FULL:
            cur = np.full(s.n_voxels, init_bits(m, s.score_init), dtype=np.uint32)
        else:
            cur = np.ascontiguousarray(maps[m], dtype=np.float32).reshape(-1).view(np.uint32).copy()
        cur[idx] = bits
        out[m] = cur.view(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# World snapshots (include/vofod.h, WORLD SNAPSHOTS: vofod_world_export / vofod_world_apply): the tiles of the world store.
# A 128-byte header, u32 tile[n4] (n4 = n rounded up to a multiple of 4; directory indices, strictly ascending, padding 0xFFFFFFFF),
# then n tiles of 512 u32 words as the pool holds them.
WORLD_MAGIC = 0x44574656  # "VFWD"
WORLD_VERSION = 1
WORLD_TILE = 8
WORLD_TILE_WORDS = WORLD_TILE ** 3
WORLD_PAD = 0xFFFFFFFF

WORLD_HEADER = np.dtype(
    {
        "names": ["magic", "version", "kind", "tile_edge", "map_size", "map_offset", "voxel_size", "score_init", "base_gen", "new_gen", "origin", "box_lo", "box_hi", "zero", "n_tiles",
                  "shifts_short_of_tiles", "voxels_forgotten"],
        "formats": ["<u4", "<u4", "<u4", "<u4", ("<i4", 3), ("<f4", 3), "<f4", "<f4", "<u8", "<u8", ("<i4", 3), ("<i4", 3), ("<i4", 3), "<u4", "<u8", "<u8", "<u8"],
        "offsets": [0, 4, 8, 12, 16, 28, 40, 44, 48, 56, 64, 76, 88, 100, 104, 112, 120],
        "itemsize": HEADER_BYTES,
    }
)


@dataclass
class WorldSnapshot:
    kind: int
    map_size: tuple
    map_offset: tuple
    voxel_size: float
    score_init: float
    origin: tuple  # K: the world index of the owner's window voxel (0, 0, 0)
    box_lo: tuple
    box_hi: tuple
    base_gen: int = 0
    new_gen: int = 0
    shifts_short_of_tiles: int = 0
    voxels_forgotten: int = 0
    index: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))  # directory indices (tz * T1 + ty) * T0 + tx, ascending
    tiles: np.ndarray = field(default_factory=lambda: np.zeros((0, WORLD_TILE_WORDS), np.uint32))  # [n, 512], z / y / x inside a tile

    @property
    def tiles_per_axis(self) -> tuple:
        return tuple(-(-(int(h) - int(l)) // WORLD_TILE) for l, h in zip(self.box_lo, self.box_hi))

    def tile_origin(self, k: int) -> tuple:
        """world index of voxel (0, 0, 0) of carried tile k"""
        T = self.tiles_per_axis
        d = int(self.index[k])
        t = (d % T[0], (d // T[0]) % T[1], d // (T[0] * T[1]))
        return tuple(int(self.box_lo[a]) + WORLD_TILE * t[a] for a in range(3))


def world_nbytes(n: int) -> int:
    """size of a world snapshot of n tiles"""
    return HEADER_BYTES + 4 * (-(-int(n) // 4) * 4) + 4 * WORLD_TILE_WORDS * int(n)


def encode_world(s: WorldSnapshot) -> np.ndarray:
    """the bytes of world snapshot `s` (uint8)"""
    idx = np.ascontiguousarray(s.index, dtype="<u4").reshape(-1)
    tiles = np.ascontiguousarray(s.tiles, dtype="<u4").reshape(-1, WORLD_TILE_WORDS)
    if tiles.shape[0] != idx.size:
        raise ValueError("world snapshot: one tile of 512 words per index")
    h = np.zeros(1, dtype=WORLD_HEADER)
    h["magic"], h["version"], h["kind"], h["tile_edge"] = WORLD_MAGIC, WORLD_VERSION, s.kind, WORLD_TILE
    h["map_size"], h["map_offset"] = np.asarray(s.map_size, dtype=np.int32), np.asarray(s.map_offset, dtype=np.float32)
    h["voxel_size"], h["score_init"], h["base_gen"], h["new_gen"] = s.voxel_size, s.score_init, s.base_gen, s.new_gen
    h["origin"], h["box_lo"], h["box_hi"] = np.asarray(s.origin, dtype=np.int32), np.asarray(s.box_lo, dtype=np.int32), np.asarray(s.box_hi, dtype=np.int32)
    h["n_tiles"], h["shifts_short_of_tiles"], h["voxels_forgotten"] = idx.size, s.shifts_short_of_tiles, s.voxels_forgotten
    lst = np.full(-(-idx.size // 4) * 4, WORLD_PAD, dtype="<u4")
    lst[: idx.size] = idx
    return np.concatenate([h.view(np.uint8).reshape(-1), lst.view(np.uint8), tiles.reshape(-1).view(np.uint8)])


def decode_world(buf, check: bool = True) -> WorldSnapshot:
    """parse a world snapshot; ValueError on a bad magic / version / kind / tile edge / reserved word / length, or (check) indices not
    strictly ascending, beyond the box's directory, or a padding entry other than 0xFFFFFFFF"""
    b = np.frombuffer(memoryview(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if b.size < HEADER_BYTES:
        raise ValueError(f"world snapshot: {b.size} bytes, shorter than the {HEADER_BYTES}-byte header")
    h = b[:HEADER_BYTES].view(WORLD_HEADER)[0]
    if int(h["magic"]) != WORLD_MAGIC:
        raise ValueError(f"world snapshot: bad magic {int(h['magic']):#x}")
    if int(h["version"]) != WORLD_VERSION:
        raise ValueError(f"world snapshot: unknown version {int(h['version'])}")
    if int(h["kind"]) not in (KIND_DELTA, KIND_FULL) or int(h["tile_edge"]) != WORLD_TILE or int(h["zero"]) != 0:
        raise ValueError("world snapshot: bad kind, tile edge or reserved word")
    n = int(h["n_tiles"])
    if b.size != world_nbytes(n):
        raise ValueError(f"world snapshot: {b.size} bytes, the header asks for {world_nbytes(n)}")
    n4 = -(-n // 4) * 4
    lst = b[HEADER_BYTES : HEADER_BYTES + 4 * n4].view("<u4")
    s = WorldSnapshot(kind=int(h["kind"]), map_size=tuple(int(v) for v in h["map_size"]), map_offset=tuple(float(v) for v in h["map_offset"]), voxel_size=float(h["voxel_size"]),
                      score_init=float(h["score_init"]), origin=tuple(int(v) for v in h["origin"]), box_lo=tuple(int(v) for v in h["box_lo"]), box_hi=tuple(int(v) for v in h["box_hi"]),
                      base_gen=int(h["base_gen"]), new_gen=int(h["new_gen"]), shifts_short_of_tiles=int(h["shifts_short_of_tiles"]), voxels_forgotten=int(h["voxels_forgotten"]))
    s.index = lst[:n].copy()
    s.tiles = b[HEADER_BYTES + 4 * n4 :].view("<u4").reshape(n, WORLD_TILE_WORDS).copy()
    if check:
        n_dir = int(np.prod(np.asarray(s.tiles_per_axis, dtype=np.int64)))
        if np.any(lst[n:] != WORLD_PAD) or (n and (np.any(s.index[1:] <= s.index[:-1]) or int(s.index[-1]) >= n_dir)):
            raise ValueError("world snapshot: tile indices not strictly ascending, beyond the box, or bad padding")
    return s
