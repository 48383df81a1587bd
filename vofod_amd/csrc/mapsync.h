// Sparse voxel-map snapshots and deltas (include/vofod.h, vofod_map_export / vofod_map_apply / vofod_broadcast_map): the set
// of voxels whose 32-bit pattern differs from a base, found on the device, sorted by linear index and written in the wire
// format below.  The reference has no counterpart (it can only reload its a-priori cloud, vofod_nodelet.cpp:306-355).
//
//   k_ms_count   streams a map and its base (the owner's shadow = what it last exported, or the init constant of a full
//                snapshot) in tiles of MS_TILE voxels: one difference count per tile.  16-byte loads, MS_QPL of them per lane
//                and operand issued before the first compare, grid-stride over the tiles.
//   (gscan)      exclusive scan of the tile counts: each tile's first record.
//   k_ms_emit    touches only tiles with a non-zero count (a full snapshot: every tile, it also copies the map into the shadow),
//                compacts the differing voxels with ballot + mbcnt prefixes into idx[] / bits[] in ascending order and brings
//                the shadow up to date.
//   k_ms_check   one pass over the records of an incoming snapshot: indices strictly ascending and below M.
//   k_ms_scatter map[idx[i]] = bits[i].
//
// No map-writing kernel of the per-scan path knows about any of this: the count pass finds the changes by comparison.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace vms
{

constexpr uint32_t MS_MAGIC = 0x444D4656u;  // "VFMD"
constexpr uint32_t MS_VERSION = 1;
constexpr int MS_THREADS = 256;
constexpr int MS_QPL = 8;                                 // 16-byte loads per lane, tile and operand
constexpr uint32_t MS_TILE_Q = MS_QPL * MS_THREADS;       // quads (4 voxels) per tile
constexpr uint64_t MS_TILE = 4ull * MS_TILE_Q;            // voxels per tile (8192: 32 KiB of map)
constexpr uint32_t MS_GRID = 2048;                        // workgroups of the streaming passes (8 per CU)

// the 128-byte header of the wire format (little endian: the same bytes in memory, over RCCL and in a file)
struct WireHeader
{
  uint32_t magic, version, maps, kind;
  int32_t map_size[3];
  float map_offset[3];
  float voxel_size, score_init;
  uint64_t base_gen, new_gen;
  int32_t detection_its;
  uint32_t last_detection_id;
  int32_t background_pts_sufficient, sure_background_sufficient;
  int32_t raycast_pending, raycast_start_its;
  uint64_t n_records[3];
  uint8_t zero[16];
};
static_assert(sizeof(WireHeader) == 128, "map snapshot header: 128 bytes");
static_assert(offsetof(WireHeader, base_gen) == 48 && offsetof(WireHeader, detection_its) == 64 && offsetof(WireHeader, n_records) == 88,
              "map snapshot header layout");

__device__ __forceinline__ uint32_t ms_ndiff(const uint4 a, const uint4 b)
{
  return static_cast<uint32_t>(a.x != b.x) + static_cast<uint32_t>(a.y != b.y) + static_cast<uint32_t>(a.z != b.z) + static_cast<uint32_t>(a.w != b.w);
}

// quad q (voxels 4q..4q+3) of a map of n voxels; voxels past the end read as `fill`
__device__ __forceinline__ uint4 ms_load_tail(const uint32_t* __restrict__ p, uint64_t q, uint64_t n, uint32_t fill)
{
  const uint64_t i = 4 * q;
  uint4 v = make_uint4(fill, fill, fill, fill);
  if (i + 4 <= n)
    return reinterpret_cast<const uint4*>(p)[q];
  if (i < n)
    v.x = p[i];
  if (i + 1 < n)
    v.y = p[i + 1];
  if (i + 2 < n)
    v.z = p[i + 2];
  return v;
}

__device__ __forceinline__ void ms_put_tail(uint32_t* __restrict__ p, uint64_t q, uint64_t n, const uint4 v)
{
  const uint64_t i = 4 * q;
  if (i + 4 <= n)
  {
    reinterpret_cast<uint4*>(p)[q] = v;
    return;
  }
  if (i < n)
    p[i] = v.x;
  if (i + 1 < n)
    p[i + 1] = v.y;
  if (i + 2 < n)
    p[i + 2] = v.z;
}

// MS_QPL quads of one lane in tile t: quad t*MS_TILE_Q + k*MS_THREADS + threadIdx.x (a workgroup reads 4 KiB contiguous per k)
__device__ __forceinline__ void ms_load_tile(const uint32_t* __restrict__ p, uint32_t t, uint64_t n, uint32_t fill, uint4 (&v)[MS_QPL])
{
  const uint64_t q0 = static_cast<uint64_t>(t) * MS_TILE_Q + threadIdx.x;
  if ((static_cast<uint64_t>(t) + 1) * MS_TILE <= n)
  {
    const uint4* __restrict__ p4 = reinterpret_cast<const uint4*>(p) + q0;
#pragma unroll
    for (int k = 0; k < MS_QPL; k++)
      v[k] = p4[k * MS_THREADS];
  }
  else
  {
#pragma unroll
    for (int k = 0; k < MS_QPL; k++)
      v[k] = ms_load_tail(p, q0 + k * MS_THREADS, n, fill);
  }
}

__device__ __forceinline__ uint32_t ms_block_sum(uint32_t c, uint32_t* wsum)
{
#pragma unroll
  for (int s = 32; s > 0; s >>= 1)
    c += __shfl_xor(c, s);
  if ((threadIdx.x & 63) == 0)
    wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  const uint32_t tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return tot;
}

// count pass: tile_count[t] = voxels of tile t whose bits differ from the base (FULL: the constant `init`, else `shadow`)
template <bool FULL>
__global__ __launch_bounds__(MS_THREADS) void k_ms_count(const uint32_t* __restrict__ map, const uint32_t* __restrict__ shadow, uint64_t n, uint32_t init, uint32_t ntiles,
                                                         uint32_t* __restrict__ tile_count)
{
  __shared__ uint32_t wsum[MS_THREADS / 64];
  const uint4 ref = make_uint4(init, init, init, init);
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x)
  {
    uint4 a[MS_QPL], b[MS_QPL];
    ms_load_tile(map, t, n, FULL ? init : 0u, a);
    if (!FULL)
      ms_load_tile(shadow, t, n, 0u, b);
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < MS_QPL; k++)
      c += ms_ndiff(a[k], FULL ? ref : b[k]);
    const uint32_t tot = ms_block_sum(c, wsum);
    if (threadIdx.x == 0)
      tile_count[t] = tot;
  }
}

// emit pass: the differing voxels of tile t go to idx / bits from position tile_prefix[t] on, in ascending index order; the
// shadow takes the map's value where they differ (FULL: everywhere - a full snapshot leaves shadow == map)
template <bool FULL>
__global__ __launch_bounds__(MS_THREADS) void k_ms_emit(const uint32_t* __restrict__ map, uint32_t* __restrict__ shadow, uint64_t n, uint32_t init, uint32_t ntiles,
                                                        const uint32_t* __restrict__ tile_count, const uint32_t* __restrict__ tile_prefix, uint32_t* __restrict__ idx_out,
                                                        uint32_t* __restrict__ bits_out)
{
  __shared__ uint32_t wsum[MS_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x)
  {
    const uint32_t cnt = tile_count[t];
    if (!FULL && cnt == 0)
      continue;  // (uniform over the workgroup)
    uint4 a[MS_QPL], b[MS_QPL];
    ms_load_tile(map, t, n, FULL ? init : 0u, a);
    if (!FULL)
      ms_load_tile(shadow, t, n, 0u, b);
    const uint64_t q0 = static_cast<uint64_t>(t) * MS_TILE_Q + threadIdx.x;
    if (FULL)
    {
#pragma unroll
      for (int k = 0; k < MS_QPL; k++)
        ms_put_tail(shadow, q0 + k * MS_THREADS, n, a[k]);
    }
    if (cnt == 0)
      continue;
    uint32_t pos = tile_prefix[t];
#pragma unroll
    for (int k = 0; k < MS_QPL; k++)
    {
      const uint4 r = FULL ? make_uint4(init, init, init, init) : b[k];
      const bool d0 = a[k].x != r.x, d1 = a[k].y != r.y, d2 = a[k].z != r.z, d3 = a[k].w != r.w;
      const unsigned long long m0 = __ballot(d0), m1 = __ballot(d1), m2 = __ballot(d2), m3 = __ballot(d3);
      auto below = [](unsigned long long m) { return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u)); };
      const uint32_t lane_pre = below(m0) + below(m1) + below(m2) + below(m3);
      const uint32_t wave_tot = __popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3);
      if (lane == 0)
        wsum[wave] = wave_tot;
      __syncthreads();
      uint32_t wpre = 0, btot = 0;
#pragma unroll
      for (int w = 0; w < MS_THREADS / 64; w++)
      {
        wpre += w < wave ? wsum[w] : 0u;
        btot += wsum[w];
      }
      __syncthreads();
      if (d0 | d1 | d2 | d3)
      {
        const uint64_t q = q0 + k * MS_THREADS;
        const uint32_t i0 = static_cast<uint32_t>(4 * q);
        uint32_t o = pos + wpre + lane_pre;
        if (d0)
        {
          idx_out[o] = i0;
          bits_out[o++] = a[k].x;
        }
        if (d1)
        {
          idx_out[o] = i0 + 1;
          bits_out[o++] = a[k].y;
        }
        if (d2)
        {
          idx_out[o] = i0 + 2;
          bits_out[o++] = a[k].z;
        }
        if (d3)
        {
          idx_out[o] = i0 + 3;
          bits_out[o] = a[k].w;
        }
        if (!FULL)
          ms_put_tail(shadow, q, n, a[k]);
      }
      pos += btot;
    }
  }
}

// records of one map of an incoming snapshot: strictly ascending, below n.  Any violation sets *bad (a plain store: every
// writer writes the same 1).
__global__ __launch_bounds__(256) void k_ms_check(const uint32_t* __restrict__ idx, uint32_t count, uint64_t n, uint32_t* __restrict__ bad)
{
  bool ok = true;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x)
  {
    const uint32_t v = idx[i];
    ok &= static_cast<uint64_t>(v) < n && (i == 0 || idx[i - 1] < v);
  }
  if (!ok)
    *bad = 1u;
}

__global__ __launch_bounds__(256) void k_ms_scatter(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ bits, uint32_t count, uint32_t* __restrict__ map)
{
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x)
    map[idx[i]] = bits[i];
}

}  // namespace vms

// Per-handle state of the snapshots (owned by vofod_handle).  The shadow of a map costs 4 * M bytes
// (78 MB at 0.25 m, 1.2 GB at 0.1 m for configs[4]); it is allocated on the first export of that map.
struct MapSyncState
{
  DevBuf<uint32_t> d_shadow[3];
  DevBuf<uint32_t> d_tiles;   // [3][ntiles] difference counts
  DevBuf<uint32_t> d_prefix;  // [3][ntiles + 1] their exclusive scan
  DevBuf<uint32_t> d_bsum;    // gscan's block sums
  DevBuf<uint32_t> d_small;   // [0..2] totals per map, [3] the check flag
  PinBuf<uint32_t> h_small;   // its host copy
  DevBuf<uint8_t> d_wire;     // staging of host-side snapshots and of vofod_broadcast_map (its control words live in vofod_comm)
  uint32_t ntiles = 0;
  uint64_t chain_gen = 0;        // export side: generation last exported (0 = no chain) ...
  int32_t chain_mask = 0;        // ... and its maps mask
  uint64_t applied_gen = 0;      // apply side: generation last applied (0 = none) ...
  int32_t applied_mask = 0;      // ... and its maps mask
};
