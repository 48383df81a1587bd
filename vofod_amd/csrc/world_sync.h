// Snapshots and deltas of the world store (include/vofod.h, WORLD SNAPSHOTS: vofod_world_export / vofod_world_apply): the tile pool
// of world_store.h gathered into a wire format on the device, and a checked scatter with tile allocation on the applying side.  The
// reference has no counterpart.
//
// The directory is walked in CHUNKS of 64 words, one wave per chunk (a workgroup holds four independent waves, no LDS, no barrier):
//   k_world_select  lane l of the wave reads directory word 64 * chunk + l; a ballot gives the allocated tiles of the chunk.  FULL:
//                   they are the selection.  DELTA: for every allocated tile in turn (a wave-uniform loop over the ballot's bits) the
//                   wave selects it when its slot is at or beyond what the last export knew (`known`: slots are handed out in order
//                   and never freed inside a chain), or compares its 2 KiB with the shadow - two uint4 per lane and operand, all four
//                   loads issued before the compare, one ballot.  Out: a 64-bit selection mask and a count per chunk.
//   (gscan)         exclusive scan of the chunk counts: the rank of each chunk's first selected tile, and the total.
//   k_world_emit    chunks with a non-zero mask only: tile k of the chunk has rank prefix + popcount(mask below k) - ASCENDING
//                   DIRECTORY ORDER COMES FROM THE SCAN, not from atomics arriving.  Its directory index goes to the index list, its
//                   2 KiB go with 16-byte loads and stores into the record and into the shadow.
//   k_world_check   an incoming index list: strictly ascending, below the directory length, padding 0xFFFFFFFF (any violation sets a
//                   flag); and the number of carried tiles this directory has not allocated.  The host looks at both before anything
//                   is written - the one round trip the a-priori path pays too (api_maps.h); apply is not per-frame work.
//   k_world_scatter behind a passed check: one wave per carried tile.  A tile the directory does not hold takes the next slot (one
//                   atomicAdd on the used counter by lane 0 - which slot a tile gets shows in no answer of the library: exports are
//                   in directory order and vofod_world_read goes through the directory); the 2 KiB are copied with 16-byte stores.
//                   Thread 0 of the grid sets the two cumulative counters to the header's values.
// Order comes from the kernel boundaries on the handle's stream; no workgroup waits for another.  No kernel of world_store.h knows
// about any of this: the select pass finds the changes by comparison, as k_ms_count does for the window (mapsync.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_mem.h"
#include "world_store.h"

namespace vwy
{

constexpr uint32_t WY_MAGIC = 0x44574656u;  // "VFWD"
constexpr uint32_t WY_VERSION = 1;
constexpr int WY_THREADS = 256;
constexpr uint32_t WY_WAVES = WY_THREADS / 64;  // chunks (select, emit) or tiles (scatter) per workgroup and step
constexpr uint32_t WY_CHUNK = 64;               // directory words per wave: one ballot
constexpr uint32_t WY_GRID = 4096;              // cap of the grid-stride walks
constexpr uint32_t WY_PAD = 0xFFFFFFFFu;        // padding entry of the index list

// the 128-byte header of the wire format (little endian: the same bytes in memory and in a file)
struct WireHeader
{
  uint32_t magic, version, kind, tile_edge;
  int32_t map_size[3];
  float map_offset[3];
  float voxel_size, score_init;
  uint64_t base_gen, new_gen;
  int32_t K[3], box_lo[3], box_hi[3];
  uint32_t zero;
  uint64_t n_tiles, shifts_short_of_tiles, voxels_forgotten;
};
static_assert(sizeof(WireHeader) == 128, "world snapshot header: 128 bytes");
static_assert(offsetof(WireHeader, base_gen) == 48 && offsetof(WireHeader, K) == 64 && offsetof(WireHeader, zero) == 100 && offsetof(WireHeader, n_tiles) == 104,
              "world snapshot header layout");

inline uint64_t pad4(uint64_t n) { return (n + 3) & ~3ull; }
inline uint64_t wire_bytes(uint64_t n) { return sizeof(WireHeader) + 4 * pad4(n) + 4ull * vws::WS_TILE_WORDS * n; }

__device__ __forceinline__ bool differs(const uint4 a, const uint4 b) { return (a.x != b.x) | (a.y != b.y) | (a.z != b.z) | (a.w != b.w); }

__device__ __forceinline__ uint32_t below(unsigned long long m, uint32_t k) { return static_cast<uint32_t>(__popcll(m & ((1ull << k) - 1ull))); }

// chunk c covers directory words [64 c, 64 c + 64) of n_dir; sel[c] and cnt[c] are written for every chunk
template <bool FULL>
__global__ __launch_bounds__(WY_THREADS) void k_world_select(const uint32_t* __restrict__ dir, uint32_t n_dir, uint32_t n_chunks, const uint32_t* __restrict__ pool, const uint32_t* __restrict__ shadow,
                                                            uint32_t known, uint64_t cap, unsigned long long* __restrict__ sel, uint32_t* __restrict__ cnt)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t c = blockIdx.x * WY_WAVES + wave; c < n_chunks; c += gridDim.x * WY_WAVES)
  {
    const uint32_t d = c * WY_CHUNK + lane;
    const uint32_t slot = d < n_dir ? dir[d] : vws::WS_EMPTY;
    unsigned long long m = __ballot(slot < vws::WS_WANTED && slot < cap);  // (a slot at or beyond the pool cannot exist: it is not followed)
    if (!FULL)
    {
      unsigned long long todo = m;
      while (todo)  // (wave-uniform)
      {
        const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(todo));
        todo &= todo - 1;
        const uint32_t s = static_cast<uint32_t>(__shfl(static_cast<int>(slot), static_cast<int>(k)));
        if (s >= known)
          continue;  // allocated since the last export: selected as it stands
        const uint4* __restrict__ a = reinterpret_cast<const uint4*>(pool + static_cast<uint64_t>(s) * vws::WS_TILE_WORDS);
        const uint4* __restrict__ b = reinterpret_cast<const uint4*>(shadow + static_cast<uint64_t>(s) * vws::WS_TILE_WORDS);
        const uint4 a0 = a[lane], a1 = a[lane + 64], b0 = b[lane], b1 = b[lane + 64];
        if (!__ballot(differs(a0, b0) || differs(a1, b1)))
          m &= ~(1ull << k);
      }
    }
    if (lane == 0)
    {
      sel[c] = m;
      cnt[c] = static_cast<uint32_t>(__popcll(m));
    }
  }
}

// prefix: the exclusive scan of cnt; idx_out: the index list of the record (n entries behind a passed capacity check), tiles_out: its
// tiles.  Every selected tile is copied into the shadow as well: afterwards shadow == pool on what was carried.
__global__ __launch_bounds__(WY_THREADS) void k_world_emit(const uint32_t* __restrict__ dir, uint32_t n_dir, uint32_t n_chunks, const uint32_t* __restrict__ pool, uint32_t* __restrict__ shadow,
                                                          uint64_t cap, const unsigned long long* __restrict__ sel, const uint32_t* __restrict__ prefix, uint32_t n, uint32_t* __restrict__ idx_out,
                                                          uint32_t* __restrict__ tiles_out)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t c = blockIdx.x * WY_WAVES + wave; c < n_chunks; c += gridDim.x * WY_WAVES)
  {
    unsigned long long todo = sel[c];
    if (!todo)
      continue;  // (wave-uniform)
    const unsigned long long m = todo;
    const uint32_t first = prefix[c];
    const uint32_t d = c * WY_CHUNK + lane;
    const uint32_t slot = d < n_dir ? dir[d] : vws::WS_EMPTY;
    while (todo)
    {
      const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(todo));
      todo &= todo - 1;
      const uint32_t s = static_cast<uint32_t>(__shfl(static_cast<int>(slot), static_cast<int>(k)));
      const uint32_t rank = first + below(m, k);
      if (rank >= n || s >= cap)  // (the record holds n tiles; the directory was read by k_world_select on this stream: it holds by construction)
        continue;
      const uint4* __restrict__ a = reinterpret_cast<const uint4*>(pool + static_cast<uint64_t>(s) * vws::WS_TILE_WORDS);
      const uint4 a0 = a[lane], a1 = a[lane + 64];
      uint4* __restrict__ o = reinterpret_cast<uint4*>(tiles_out + static_cast<uint64_t>(rank) * vws::WS_TILE_WORDS);
      uint4* __restrict__ sh = reinterpret_cast<uint4*>(shadow + static_cast<uint64_t>(s) * vws::WS_TILE_WORDS);
      o[lane] = a0;
      o[lane + 64] = a1;
      sh[lane] = a0;
      sh[lane + 64] = a1;
      if (lane == 0)
        idx_out[rank] = c * WY_CHUNK + k;
    }
  }
}

// out[0]: set to 1 by any violation (a plain store: every writer writes the same 1); out[1]: carried tiles without a slot here
__global__ __launch_bounds__(WY_THREADS) void k_world_check(const uint32_t* __restrict__ idx, uint32_t n, uint32_t n4, const uint32_t* __restrict__ dir, uint32_t n_dir, uint32_t* __restrict__ out)
{
  bool ok = true;
  uint32_t fresh = 0;
  for (uint32_t i = blockIdx.x * WY_THREADS + threadIdx.x; i < n4; i += gridDim.x * WY_THREADS)
  {
    const uint32_t v = idx[i];
    if (i >= n)
    {
      ok &= v == WY_PAD;
      continue;
    }
    const bool inside = v < n_dir;
    ok &= inside && (i == 0 || idx[i - 1] < v);
    if (inside)
      fresh += dir[v] >= vws::WS_WANTED ? 1u : 0u;
  }
  if (!ok)
    out[0] = 1u;
  if (fresh)
    atomicAdd(out + 1, fresh);
}

// one wave per carried tile.  Behind a passed k_world_check: used + fresh <= cap, every index below n_dir - both are tested again,
// since a caller's device buffer is the caller's to change.
__global__ __launch_bounds__(WY_THREADS) void k_world_scatter(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ tiles, uint32_t n, uint32_t* __restrict__ dir, uint32_t n_dir,
                                                             uint32_t* __restrict__ pool, uint64_t cap, unsigned long long* __restrict__ ctr, unsigned long long n_short, unsigned long long n_forgotten)
{
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    ctr[vws::WC_SHORT] = n_short;
    ctr[vws::WC_FORGOTTEN] = n_forgotten;
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t i = blockIdx.x * WY_WAVES + wave; i < n; i += gridDim.x * WY_WAVES)
  {
    const uint32_t d = idx[i];
    if (d >= n_dir)
      continue;  // (wave-uniform)
    uint32_t slot = vws::WS_EMPTY;
    if (lane == 0)
    {
      slot = dir[d];
      if (slot >= vws::WS_WANTED)
      {
        const unsigned long long got = atomicAdd(ctr + vws::WC_USED, 1ull);
        slot = got < cap ? static_cast<uint32_t>(got) : vws::WS_EMPTY;
        if (got < cap)
          dir[d] = slot;
      }
    }
    slot = static_cast<uint32_t>(__shfl(static_cast<int>(slot), 0));
    if (slot >= cap)
      continue;
    const uint4* __restrict__ a = reinterpret_cast<const uint4*>(tiles + static_cast<uint64_t>(i) * vws::WS_TILE_WORDS);
    uint4* __restrict__ o = reinterpret_cast<uint4*>(pool + static_cast<uint64_t>(slot) * vws::WS_TILE_WORDS);
    const uint4 a0 = a[lane], a1 = a[lane + 64];
    o[lane] = a0;
    o[lane + 64] = a1;
  }
}

// Per-handle state of the world snapshots (owned by vofod_handle beside vws::Store).  The shadow pool is as large as the pool (2 KiB
// per tile of max_tiles), allocated by the first export that emits and freed by vofod_world_disable / vofod_destroy.
struct State
{
  DevBuf<uint32_t> d_shadow;
  DevBuf<unsigned long long> d_sel;  // [n_chunks] selection masks
  DevBuf<uint32_t> d_cnt, d_prefix;  // [n_chunks] counts, [n_chunks + 1] their exclusive scan
  DevBuf<uint32_t> d_bsum;           // gscan's block sums
  DevBuf<uint32_t> d_small;          // [0] the total, [1] the check flag, [2] the tiles an apply would allocate
  PinBuf<uint32_t> h_small;
  DevBuf<uint8_t> d_wire;            // staging of host-side snapshots
  uint32_t n_chunks = 0;
  uint64_t chain_gen = 0;    // export side: the generation exported last (0: no chain) ...
  uint64_t known_used = 0;   // ... and the slots it knew: tiles_used at that export
  uint64_t applied_gen = 0;  // apply side: the generation applied last (0: none, or another writer has touched the store since)
  void end_chains() { chain_gen = applied_gen = 0; }
  void drop()
  {
    d_shadow.reset(), d_sel.reset(), d_cnt.reset(), d_prefix.reset(), d_bsum.reset(), d_small.reset(), h_small.reset(), d_wire.reset();
    n_chunks = 0;
    known_used = 0;
    end_chains();
  }
};

}  // namespace vwy
