// Map match (include/vofod.h, MAP MATCH; vofod_map_match): where do this scan's returns land under pose k?  One map look-up per
// return and candidate pose - not a ray walk - for up to 65535 candidates of ONE scan: per candidate the number of returns that fall
// outside the map, into a voxel at or below the threshold and into a voxel above it.  Three launches per call:
//
//   k_match_bits    the occupancy image of THIS call's threshold: bit v = map[v] > threshold over the linear voxel index.  One lane
//                   per voxel, one coalesced float load, one __ballot per wave, one lane stores the 64-bit word; the lanes beyond n
//                   of the last wave contribute 0 and still reach the ballot.  2.4 MB at OS1-128 / 0.25 m (an XCD's L2 holds it), 38 MB at
//                   0.1 m (the Infinity Cache does).  Built per call: d_mapbits has the pipeline's threshold and the pipeline's validity.
//   k_match_points  the live list.  One lane per pixel decodes the point - rd_point of range_decode.h for a range image, included,
//                   not restated; three strided loads for a point scan - and applies the SKIPPED rule; the live points of a wave are
//                   compacted (a ballot, ONE atomicAdd of the popcount by one lane on a device counter, each live lane at its
//                   prefix) into a list of 16-byte points.  THE ORDER OF THE LIST IS ARBITRARY - it depends on which wave's atomic
//                   arrives first - and that is fine: everything computed from it is an integer count, exact in any order.
//                   n_live stays on the device: the next launch is sized for width * height and its blocks beyond n_live leave at once.
//   k_match<U, Look>  the scoring walk (profiler label k_match_score).  The lanes are the CANDIDATES.  blockIdx.x is a group of 256
//                   candidates, blockIdx.y a chunk of the live list.  A lane loads its own pose once (12 VGPRs; a lane beyond
//                   n_poses takes pose n_poses - 1 and adds nothing at the end), the block stages its chunk into LDS tile by tile,
//                   and every lane walks the tile: the point is the same LDS address for all 64 lanes - a broadcast read, no bank
//                   conflict.  Three rows in __fmul_rn / __fadd_rn (PCL's
//                   association, rd_row), the float bounds test, the voxel's element address, one load.  The address never depends
//                   on a loaded value, so - as in k_map_render - the walk goes in BURSTS of U points: U addresses, U loads issued
//                   together, then U tests; per-step arrays are indexed by unrolled constants, the state is in scalar locals.  An
//                   OUTSIDE lane loads element 0 and ignores it: no index outside the image is ever formed, and no float outside
//                   [0, size) is ever converted.  The counters live in registers for the whole chunk - the point loop has no
//                   reduction - and at the end each live lane issues up to three atomicAdds into its candidate's slots, cleared on
//                   the stream before the launch.  Neighbouring candidates sit in neighbouring lanes: a wave's 64 look-ups of one
//                   point fall into a handful of cache lines.
//                   WHAT is looked up is the policy Look, as Acc is k_raycast_t's and Views k_map_render's: LookBits reads the
//                   bit image as 32-bit words (word v >> 5, bit v & 31) and counts OUTSIDE / FREE / OCCUPIED; LookField
//                   (vofod_map_match_field, label k_match_field) reads a distance field, one uint16_t per voxel, and keeps OUTSIDE,
//                   NEAR and a cost sum.  The walk, its bounds rule and its tile rule are one text for both.
//
// The chunk (points per block) and U are host-side choices.  Measured (profiles/r31_map_match.txt; OS1-128 at 0.25 m,
// 38 947 live returns): k_match_score at 1024 poses 51.8 / 57.6 / 78.1 / 132.3 / 488.2 us for chunks of 64 / 128 / 256 / 512 / 2048
// points, at 4096 poses 155.7 / 156.4 / 171.8 / 194.0 / 491.7 us - a block walks its chunk one burst behind the other, so what
// counts is how many blocks there are to hide one another's latency; U = 1 / 2 / 4 / 8 at 1024 poses and chunk 64: 53.8 / 52.6 /
// 50.0 / 49.0 us.  MM_CHUNK = 64 and MM_BURST = 8 are kept (48 VGPRs with LookBits, 51 with LookField, no scratch, 8 waves per
// SIMD); OS2-128 x 2048 at 0.1 m orders them the same way.  VOFOD_MATCH_CHUNK and VOFOD_MATCH_BURST select others per call
// (diagnostics, and the tests' way to make a small scan straddle chunks).
// Out of scope: reuse of the image between calls or of d_mapbits, a NEAR class, several scans per call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.h"
#include "device_mem.h"
#include "range_decode.h"
#include "scan_stage.h"

namespace vmm
{
using namespace vk;

constexpr int MM_THREADS = 256;            // k_match: candidates per group
constexpr uint32_t MM_MAX_POSES = 65535;
constexpr uint32_t MM_TILE = 1024;         // points staged into LDS at a time (16 KiB)
constexpr uint32_t MM_CHUNK = 64;          // points per block of the production launch (VOFOD_MATCH_CHUNK=n selects another)
constexpr int MM_BURST = 8;                // look-ups per burst of the production launch (VOFOD_MATCH_BURST=1|2|4|8 selects another)
constexpr uint32_t MM_MAX_CHUNKS = 65535;  // gridDim.y
constexpr uint32_t MM_HEAD = 4;            // words in front of the device counts: [0] n_live, the rest padding (the counts stay 16-byte aligned)

// the workspace of the match calls and of vofod_map_distance's image, owned by the handle and grown to the largest seen; h_out: where
// the one copy out lands (a host scan is staged by the query calls' one ScanStage, scan_stage.h)
struct Workspace
{
  DevBuf<unsigned long long> d_bits;  // ceil(n_voxels / 64) words
  DevBuf<float4> d_points;            // the live list, width * height entries
  DevBuf<float> d_poses;              // n_poses * 12
  DevBuf<uint32_t> d_out;             // MM_HEAD + n_poses * 4
  std::vector<uint32_t> h_out;
};

using ScanSource = vss::Staged;  // the scan as k_match_points reads it: where stage_scans (api_query.h) put it, or where the caller has it

__global__ __launch_bounds__(256) void k_match_bits(const float* __restrict__ map, uint64_t n, float threshold, unsigned long long* __restrict__ bits)
{
  const uint64_t v = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  const bool set = v < n && map[v] > threshold;  // (a NaN is never above the threshold, +inf is, an equal value is not)
  const unsigned long long word = __ballot(set);
  if ((threadIdx.x & 63) == 0 && v < n)
    bits[v >> 6] = word;
}

enum : int
{
  SRC_RANGE = 0,    // range image without poses
  SRC_MOTION = 1,   // range image with col_tfs
  SRC_POINTS = 2    // point scan
};

template <int SRC, bool POSE16>
__global__ __launch_bounds__(256) void k_match_points(const ScanSource src, uint32_t n_px, const float* __restrict__ lut_dirs, const float* __restrict__ lut_offs, const vrd::MotionArgs ma,
                                                      float4* __restrict__ points, uint32_t* __restrict__ n_live)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
  bool live = false;
  if (i < n_px)
  {
    if constexpr (SRC == SRC_POINTS)
    {
      p0 = ldg_f32(src.x + static_cast<uint64_t>(i) * src.stride);
      p1 = ldg_f32(src.y + static_cast<uint64_t>(i) * src.stride);
      p2 = ldg_f32(src.z + static_cast<uint64_t>(i) * src.stride);
      live = !(p0 == 0.0f && p1 == 0.0f && p2 == 0.0f);  // (either sign of zero)
    }
    else
    {
      const uint32_t rng = *reinterpret_cast<const uint32_t*>(src.range + static_cast<uint64_t>(i) * src.stride);
      uint32_t m = 0;
      if constexpr (SRC == SRC_MOTION)
      {
        const uint32_t row = i / ma.width;
        m = measurement_column(row, i - row * ma.width, ma.width, ma.shift);
      }
      const size_t l = 3u * static_cast<size_t>(i);
      vrd::rd_point<SRC == SRC_MOTION, POSE16>(rng, lut_dirs[l], lut_dirs[l + 1], lut_dirs[l + 2], lut_offs[l], lut_offs[l + 1], lut_offs[l + 2], src.poses, m, ma, p0, p1, p2);
      live = rng != 0u;
    }
    // |p| < inf is false for a NaN too
    const bool finite = fabsf(p0) < INFINITY && fabsf(p1) < INFINITY && fabsf(p2) < INFINITY;
    const bool excluded = p0 >= ma.lo[0] && p0 <= ma.hi[0] && p1 >= ma.lo[1] && p1 <= ma.hi[1] && p2 >= ma.lo[2] && p2 <= ma.hi[2];
    live = live && finite && !excluded;
  }
  // every lane of the wave is here: the wave's live points go behind one another at the place one atomic reserves
  const unsigned long long mask = __ballot(live);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0 && mask)
    base = atomicAdd(n_live, static_cast<uint32_t>(__popcll(mask)));
  base = __shfl(base, 0);
  if (live)
    points[base + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)))] = make_float4(p0, p1, p2, 0.0f);
}

struct ScoreParams
{
  uint32_t n_poses, chunk;
  float fsx, fsy, fsz;  // the map's size as floats: the bounds of the float test
};

// ---- the two policies of k_match.  A policy goes to the kernel by value and is the lane's private state from then on.

// vofod_map_match: the bit image of k_match_bits, read as 32-bit words
struct LookBits
{
  using Elem = uint32_t;
  const Elem* image;
  uint32_t n_out = 0, n_occ = 0;
  __device__ __forceinline__ uint32_t index(uint32_t v) const { return v >> 5; }
  __device__ __forceinline__ void tile_begin() {}
  __device__ __forceinline__ void take(bool counted, bool in, uint32_t word, uint32_t v)
  {
    n_out += counted && !in ? 1u : 0u;
    n_occ += counted && in ? (word >> (v & 31u)) & 1u : 0u;
  }
  __device__ __forceinline__ void tile_end() {}
  __device__ __forceinline__ void finish(uint32_t* slot, uint32_t, uint32_t n_points) const
  {
    const uint32_t n_free = n_points - n_out - n_occ;
    if (n_out)
      atomicAdd(slot + 1, n_out);  // VOFOD_MATCH_OUTSIDE
    if (n_free)
      atomicAdd(slot + 2, n_free);  // VOFOD_MATCH_FREE
    if (n_occ)
      atomicAdd(slot + 3, n_occ);  // VOFOD_MATCH_OCCUPIED
  }
};

// vofod_map_match_field: a distance field (map_distance.h), one 2-byte value per voxel.  Two counters (inside, NEAR) and a sum; THE
// SUM MUST NOT WRAP: a tile of MM_TILE = 1024 points x 65535 = 67 107 840 < 2^32, so the tile's sum is 32 bits wide and is flushed
// into a 64-bit one behind every tile.  At the end one 64-bit atomicAdd and at most two 32-bit ones (OUTSIDE and NEAR; FAR is what
// the host has left of the live list).
struct LookField
{
  using Elem = uint16_t;
  const Elem* image;
  uint32_t near2;
  unsigned long long* cost;  // one sum per candidate, cleared on the stream before the launch
  uint32_t n_in = 0, n_near = 0, tile_sum = 0;  // (the chunk's points inside the map, and those of them that are NEAR)
  unsigned long long sum = 0;
  __device__ __forceinline__ uint32_t index(uint32_t v) const { return v; }
  __device__ __forceinline__ void tile_begin() { tile_sum = 0; }
  __device__ __forceinline__ void take(bool counted, bool in, uint32_t d2, uint32_t)
  {
    const bool inside = counted && in;  // (one lane mask decides all three)
    n_in += inside ? 1u : 0u;
    n_near += inside && d2 <= near2 ? 1u : 0u;
    tile_sum += inside ? d2 : 0u;
  }
  __device__ __forceinline__ void tile_end() { sum += tile_sum; }
  __device__ __forceinline__ void finish(uint32_t* slot, uint32_t cand, uint32_t n_points) const
  {
    const uint32_t n_out = n_points - n_in;
    if (n_out)
      atomicAdd(slot + 1, n_out);  // VOFOD_FIELD_OUTSIDE
    if (n_near)
      atomicAdd(slot + 3, n_near);  // VOFOD_FIELD_NEAR (FAR: the host's n_live - OUTSIDE - NEAR)
    if (sum)
      atomicAdd(cost + cand, sum);
  }
};

template <int U, class Look>
__global__ __launch_bounds__(MM_THREADS) void k_match(const ScoreParams sp, const MapGeom mg, Look look, const float4* __restrict__ points, const float* __restrict__ poses,
                                                     uint32_t* __restrict__ out)
{
  __shared__ float4 s_pts[MM_TILE];
  const uint32_t n_live = out[0];
  const uint32_t begin = blockIdx.y * sp.chunk;
  if (begin >= n_live)
    return;
  const uint32_t end = min(begin + sp.chunk, n_live);
  const uint32_t cand = blockIdx.x * MM_THREADS + threadIdx.x;
  const bool alive = cand < sp.n_poses;
  const float* T = poses + 12u * static_cast<size_t>(alive ? cand : sp.n_poses - 1u);
  const float r00 = T[0], r01 = T[1], r02 = T[2], t0 = T[3];
  const float r10 = T[4], r11 = T[5], r12 = T[6], t1 = T[7];
  const float r20 = T[8], r21 = T[9], r22 = T[10], t2 = T[11];
  const uint32_t sx = static_cast<uint32_t>(mg.sx), sy = static_cast<uint32_t>(mg.sy);
  const typename Look::Elem* __restrict__ image = look.image;
  for (uint32_t tile = begin; tile < end; tile += MM_TILE)
  {
    const uint32_t cnt = min(MM_TILE, end - tile);
    __syncthreads();  // (the tile before this one has been walked by every lane)
    for (uint32_t j = threadIdx.x; j < cnt; j += MM_THREADS)
      s_pts[j] = points[tile + j];
    __syncthreads();
    look.tile_begin();
    // (2-byte values tempt the loop vectoriser to walk two bursts side by side in packed halves: twice the registers, nothing gained)
#pragma clang loop vectorize(disable) interleave(disable)
    for (uint32_t j = 0; j < cnt; j += U)
    {
      // ---- the burst: U addresses, nothing read.  A step behind the tile's end looks at the tile's last point again and counts nothing.
      uint32_t v[U];
      bool in[U];  // (a lane mask each: scalar registers, where a bit per step in a vector register costs a shift and a test per step)
#pragma unroll
      for (int u = 0; u < U; u++)
      {
        const float4 p = s_pts[min(j + u, cnt - 1u)];  // (the same address in all 64 lanes: a broadcast)
        const float w0 = __fadd_rn(__fmul_rn(r00, p.x), __fadd_rn(__fmul_rn(r01, p.y), __fadd_rn(__fmul_rn(r02, p.z), t0)));
        const float w1 = __fadd_rn(__fmul_rn(r10, p.x), __fadd_rn(__fmul_rn(r11, p.y), __fadd_rn(__fmul_rn(r12, p.z), t1)));
        const float w2 = __fadd_rn(__fmul_rn(r20, p.x), __fadd_rn(__fmul_rn(r21, p.y), __fadd_rn(__fmul_rn(r22, p.z), t2)));
        const float f0 = floorf(__fmul_rn(__fsub_rn(w0, mg.off[0]), mg.vs_inv));
        const float f1 = floorf(__fmul_rn(__fsub_rn(w1, mg.off[1]), mg.vs_inv));
        const float f2 = floorf(__fmul_rn(__fsub_rn(w2, mg.off[2]), mg.vs_inv));
        // compared as floats BEFORE the conversion: a NaN or infinite w is OUTSIDE, and only floats of [0, size) are converted
        in[u] = f0 >= 0.0f && f0 < sp.fsx && f1 >= 0.0f && f1 < sp.fsy && f2 >= 0.0f && f2 < sp.fsz;
        const uint32_t x = static_cast<uint32_t>(in[u] ? f0 : 0.0f), y = static_cast<uint32_t>(in[u] ? f1 : 0.0f), z = static_cast<uint32_t>(in[u] ? f2 : 0.0f);
        v[u] = (z * sy + y) * sx + x;  // (an OUTSIDE lane: voxel 0, element 0 - no index outside the image is ever formed)
      }
      // ---- the U loads, together (every index is an element of the image)
      uint32_t m[U];
#pragma unroll
      for (int u = 0; u < U; u++)
        m[u] = image[look.index(v[u])];
      // ---- the tests: an OUTSIDE lane ignores what it loaded, a step behind the tile's end counts as nothing (wave-uniform)
#pragma unroll
      for (int u = 0; u < U; u++)
        look.take(j + u < cnt, in[u], m[u], v[u]);
    }
    look.tile_end();
  }
  if (alive)
    look.finish(out + MM_HEAD + 4u * static_cast<size_t>(cand), cand, end - begin);
}

}  // namespace vmm
