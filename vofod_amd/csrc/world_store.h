// World store (include/vofod.h, WORLD STORE): the voxel map as a window onto a sparse, tiled map of a fixed box of world indices.
// vofod_map_shift writes what leaves the window into it and reads what enters from it; vofod_load_apriori stamps the points that
// fall beyond the window.  The reference has no counterpart (its maps are sized once, voxel_map.cpp:11-48).
//
//   directory   one word per tile of the box (tiles of WS_EDGE^3 voxels, the grid anchored at box_lo, x fastest): WS_EMPTY, WS_WANTED
//               between k_world_mark and k_world_claim of one call, or the tile's slot in the pool.
//   pool        cap tiles of WS_TILE_WORDS words; slots are handed out in order and never freed (vofod_reset empties the directory).
//   ctr         WC_* counters on the device; the driver copies them out behind the last kernel of a call, in front of the call's one
//               hipStreamSynchronize.
//
// A call is a chain of kernels on the handle's stream, and ORDER COMES FROM THE KERNEL BOUNDARIES ONLY - no workgroup waits for another:
//   k_world_mark   every leaving voxel that differs from init and lies in the box: where the directory word is WS_EMPTY, one atomicCAS
//                  to WS_WANTED; the winner appends the tile to the wanted list (a handful of CAS per tile, the others see WS_WANTED
//                  with a plain load).  Leaving voxels outside the box that differ from init are counted as forgotten here.
//   k_world_claim  every workgroup reads used and wanted and takes the same decision, used + wanted <= cap.  Yes: list entry k gets
//                  slot used + k, the tile is filled with init (16-byte stores) - all-or-nothing, so which voxel won a CAS does not
//                  show in the outcome.  No: the words go back to WS_EMPTY.  It does not touch the counters it decides on: the books
//                  are closed by thread 0 of the NEXT kernel (world_commit in k_world_put), behind the kernel boundary.
//   k_world_put    every leaving voxel in the box: stored where its tile exists (a pattern equal to init too: the tile may hold an
//                  older value of the voxel), counted as forgotten where it does not and the voxel differs from init.
//   k_world_get    behind the k_map_shift of the voxel map: every voxel of the new window without a source in the old one takes the
//                  stored pattern where its tile exists.
//   k_world_mark_points / k_world_put_points   the same two steps for the a-priori points beyond the window (+inf); the cell of a point
//                  is k_apriori's float32 expression (apriori_cell) without the in-limits cut, offset by the window's origin K.
//   k_world_gather vofod_world_read: W over a box of world indices.
//
// The leaving and the entering voxels are walked as a RIM of at most three disjoint slabs of the window (Rim), x fastest inside each,
// grid stride, WS_UNROLL voxels per lane and step with their loads issued first: the cost follows |s| / S, not the map (measured:
// profiles/r23_world_store.txt).  No LDS; the only atomics are the directory CAS, the list append and the counters (which the compiler
// folds into one add per wave).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "device_mem.h"

namespace vws
{

// The cell of an a-priori point along one axis before the conversion to int: k_apriori's expression (kernels_cluster.h), token for
// token - that kernel's source is tied to the committed traffic profile and stays as it is, so the two are held together by the tests
// (a point that k_apriori puts into the window's last voxel and its neighbour that the store takes: test_gpu_world.py).
__device__ __forceinline__ float apriori_cell(float p, float off, float vs_inv) { return floorf(__fmul_rn(__fsub_rn(p, off), vs_inv)); }

constexpr int32_t WS_EDGE = 8;  // == VOFOD_WORLD_TILE
constexpr uint32_t WS_TILE_WORDS = WS_EDGE * WS_EDGE * WS_EDGE;
constexpr uint32_t WS_EMPTY = 0xFFFFFFFFu, WS_WANTED = 0xFFFFFFFEu;  // every other word is a slot
constexpr uint64_t WS_MAX_TILES = 0xFFFFFFF0ull;
constexpr int32_t WS_K_LIMIT = 1 << 30;
constexpr int WS_THREADS = 256;
constexpr uint32_t WS_GRID = 8192;  // cap of the grid-stride walks
constexpr int WS_UNROLL = 4;        // rim voxels per lane and step, a grid apart: their loads are issued before the first is used
enum { WC_USED = 0, WC_WANTED = 1, WC_SHORT = 2, WC_FORGOTTEN = 3, WC_N = 4 };

// The store as the handle owns it.  Directory, pool and wanted list are allocated by vofod_world_enable and by nothing else.
struct Store
{
  bool enabled = false;
  int32_t K[3] = {0, 0, 0};  // world index of the window's voxel (0, 0, 0)
  int32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, T[3] = {0, 0, 0};
  uint64_t cap = 0, n_dir = 0;
  DevBuf<uint32_t> d_dir, d_pool, d_list;  // d_list: the wanted tiles of one shift (list_cap: the tiles a window can touch)
  uint32_t list_cap = 0;
  DevBuf<unsigned long long> d_ctr;
  PinBuf<unsigned long long> h_ctr;  // the counters as the last call left them
  void drop()
  {
    d_dir.reset(), d_pool.reset(), d_list.reset(), d_ctr.reset(), h_ctr.reset();
    enabled = false;
    cap = n_dir = 0;
    list_cap = 0;
  }
};

// what the kernels need of the store (by value)
struct View
{
  uint32_t* dir;
  uint32_t* pool;
  unsigned long long* ctr;
  int32_t lo[3], hi[3];  // the box, world indices
  int32_t T[3];          // tiles per axis
  uint32_t init;         // bits of score_init
  uint64_t cap;
};

// Up to three disjoint boxes of window voxels: with per-axis intervals A[a] = [a0, a1) and their complements C[a] (an interval too:
// A[a] is empty, a prefix, a suffix or everything), the voxels with SOME coordinate inside its A are
//   slab 0: A[0] x all x all,   slab 1: C[0] x A[1] x all,   slab 2: C[0] x C[1] x A[2].
struct Rim
{
  int32_t b[3][3], w[3][3];  // per slab: first voxel and widths (x, y, z)
  uint64_t first[4];         // running voxel counts: slab k holds [first[k], first[k + 1])
};

// a0 == a1: empty.  (Plain host code.)
inline Rim make_rim(const int32_t S[3], const int32_t a0[3], const int32_t a1[3])
{
  Rim r{};
  int32_t c0[3], c1[3];
  for (int a = 0; a < 3; a++)
  {
    if (a1[a] <= a0[a])
      c0[a] = 0, c1[a] = S[a];
    else if (a0[a] == 0)
      c0[a] = a1[a], c1[a] = S[a];
    else
      c0[a] = 0, c1[a] = a0[a];
  }
  r.first[0] = 0;
  for (int k = 0; k < 3; k++)
  {
    uint64_t n = 1;
    for (int a = 0; a < 3; a++)
    {
      const int32_t lo = a < k ? c0[a] : (a == k ? a0[a] : 0), hi = a < k ? c1[a] : (a == k ? a1[a] : S[a]);
      r.b[k][a] = lo;
      r.w[k][a] = std::max(hi - lo, 0);
      n *= static_cast<uint64_t>(r.w[k][a]);
    }
    r.first[k + 1] = r.first[k] + n;
  }
  return r;
}

// The interval of window coordinates i whose i - s lies outside [0, S): what the shift s pushes out.  With -s in the place of s: the
// coordinates j of the new window whose source j + s lies outside the old one.
inline void rim_interval(int64_t s, int32_t S, int32_t& a0, int32_t& a1)
{
  if (s > 0)
    a0 = 0, a1 = static_cast<int32_t>(std::min<int64_t>(s, S));
  else if (s < 0)
    a0 = static_cast<int32_t>(std::max<int64_t>(S + s, 0)), a1 = S;
  else
    a0 = a1 = 0;
}

__device__ __forceinline__ void rim_voxel(const Rim& r, uint64_t t, int32_t& x, int32_t& y, int32_t& z)
{
  const int k = t >= r.first[2] ? 2 : (t >= r.first[1] ? 1 : 0);
  const uint64_t q = t - r.first[k];
  const uint32_t w0 = static_cast<uint32_t>(r.w[k][0]), w1 = static_cast<uint32_t>(r.w[k][1]);
  if (q <= 0xFFFFFFFFull)
  {
    // (every map the driver creates: two 32-bit divisions per voxel instead of two 64-bit ones - k_world_mark on 42.9 M rim voxels
    // at 0.1 m took 0.164 ms with the latter, profiles/r23_world_store.txt)
    const uint32_t q32 = static_cast<uint32_t>(q), row = q32 / w0, pl = row / w1;
    x = r.b[k][0] + static_cast<int32_t>(q32 - row * w0);
    y = r.b[k][1] + static_cast<int32_t>(row - pl * w1);
    z = r.b[k][2] + static_cast<int32_t>(pl);
    return;
  }
  const uint64_t row = q / w0;
  x = r.b[k][0] + static_cast<int32_t>(q - row * w0);
  const uint64_t pl = row / w1;
  y = r.b[k][1] + static_cast<int32_t>(row - pl * w1);
  z = r.b[k][2] + static_cast<int32_t>(pl);
}

// world index -> directory index and word offset inside the tile; false outside the box
__device__ __forceinline__ bool world_cell(const View& v, int64_t gx, int64_t gy, int64_t gz, uint32_t& d, uint32_t& in_tile)
{
  if (gx < v.lo[0] || gx >= v.hi[0] || gy < v.lo[1] || gy >= v.hi[1] || gz < v.lo[2] || gz >= v.hi[2])
    return false;
  const uint32_t rx = static_cast<uint32_t>(gx - v.lo[0]), ry = static_cast<uint32_t>(gy - v.lo[1]), rz = static_cast<uint32_t>(gz - v.lo[2]);
  d = ((rz >> 3) * static_cast<uint32_t>(v.T[1]) + (ry >> 3)) * static_cast<uint32_t>(v.T[0]) + (rx >> 3);
  in_tile = ((rz & 7u) * WS_EDGE + (ry & 7u)) * WS_EDGE + (rx & 7u);
  return true;
}

__device__ __forceinline__ uint32_t dir_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// EMPTY -> WANTED; the winner appends the tile.  list_cap is the number of tiles the walked voxels can touch (the driver sizes it),
// so the bound holds by construction; it is tested all the same.
__device__ __forceinline__ void want_tile(const View& v, uint32_t d, uint32_t* list, uint32_t list_cap)
{
  if (dir_load(v.dir + d) != WS_EMPTY)
    return;
  if (atomicCAS(v.dir + d, WS_EMPTY, WS_WANTED) != WS_EMPTY)
    return;
  const unsigned long long pos = atomicAdd(v.ctr + WC_WANTED, 1ull);
  if (pos < list_cap)
    list[pos] = d;
}

// Closes the books of the k_world_claim in front of this kernel (one thread of the grid calls it: nobody else reads the two counters
// in this kernel).
__device__ __forceinline__ void world_commit(const View& v, bool count_short)
{
  const unsigned long long used = v.ctr[WC_USED], wanted = v.ctr[WC_WANTED];
  if (used + wanted <= v.cap)
    v.ctr[WC_USED] = used + wanted;
  else if (count_short)
    atomicAdd(v.ctr + WC_SHORT, 1ull);
  v.ctr[WC_WANTED] = 0;
}

// K: world index of the voxel (0, 0, 0) of `map`
__global__ __launch_bounds__(WS_THREADS) void k_world_mark(const View v, const Rim rim, const uint32_t* __restrict__ map, int32_t sx, int32_t sy, int64_t k0, int64_t k1, int64_t k2,
                                                          uint32_t* __restrict__ list, uint32_t list_cap)
{
  const uint64_t n = rim.first[3], stride = static_cast<uint64_t>(gridDim.x) * WS_THREADS;
  for (uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * WS_THREADS + threadIdx.x; t0 < n; t0 += WS_UNROLL * stride)
  {
    int32_t x[WS_UNROLL], y[WS_UNROLL], z[WS_UNROLL];
    uint32_t bits[WS_UNROLL];
#pragma unroll
    for (int u = 0; u < WS_UNROLL; u++)
    {
      const uint64_t t = t0 + u * stride;
      rim_voxel(rim, t < n ? t : t0, x[u], y[u], z[u]);  // (past the end: the lane's first voxel once more, dropped below)
      bits[u] = map[(static_cast<uint64_t>(z[u]) * sy + y[u]) * sx + x[u]];
      if (t >= n)
        bits[u] = v.init;
    }
#pragma unroll
    for (int u = 0; u < WS_UNROLL; u++)
    {
      if (bits[u] == v.init)
        continue;
      uint32_t d, e;
      if (world_cell(v, k0 + x[u], k1 + y[u], k2 + z[u], d, e))
        want_tile(v, d, list, list_cap);
      else
        atomicAdd(v.ctr + WC_FORGOTTEN, 1ull);
    }
  }
}

// Two tiles per workgroup and step: 128 lanes x 16 bytes fill one.
__global__ __launch_bounds__(WS_THREADS) void k_world_claim(const View v, const uint32_t* __restrict__ list, uint32_t list_cap)
{
  const unsigned long long used = v.ctr[WC_USED];
  const unsigned long long wanted = min(v.ctr[WC_WANTED], static_cast<unsigned long long>(list_cap));
  const bool fits = used + wanted <= v.cap;
  const uint32_t half = threadIdx.x >> 7, lane = threadIdx.x & 127u;
  for (unsigned long long k = 2ull * blockIdx.x + half; k < wanted; k += 2ull * gridDim.x)
  {
    const uint32_t d = list[k];
    const unsigned long long slot = used + k;  // (< cap where fits)
    if (lane == 0)
      v.dir[d] = fits ? static_cast<uint32_t>(slot) : WS_EMPTY;
    if (fits)
      reinterpret_cast<uint4*>(v.pool + slot * WS_TILE_WORDS)[lane] = make_uint4(v.init, v.init, v.init, v.init);
  }
}

__global__ __launch_bounds__(WS_THREADS) void k_world_put(const View v, const Rim rim, const uint32_t* __restrict__ map, int32_t sx, int32_t sy, int64_t k0, int64_t k1, int64_t k2)
{
  if (blockIdx.x == 0 && threadIdx.x == 0)
    world_commit(v, true);
  const uint64_t n = rim.first[3], stride = static_cast<uint64_t>(gridDim.x) * WS_THREADS;
  for (uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * WS_THREADS + threadIdx.x; t0 < n; t0 += WS_UNROLL * stride)
  {
    uint32_t bits[WS_UNROLL], slot[WS_UNROLL], e[WS_UNROLL];
    bool ok[WS_UNROLL];
#pragma unroll
    for (int u = 0; u < WS_UNROLL; u++)
    {
      const uint64_t t = t0 + u * stride;
      int32_t x, y, z;
      rim_voxel(rim, t < n ? t : t0, x, y, z);
      uint32_t d = 0;
      ok[u] = world_cell(v, k0 + x, k1 + y, k2 + z, d, e[u]) && t < n;  // (outside the box: k_world_mark has counted it)
      bits[u] = map[(static_cast<uint64_t>(z) * sy + y) * sx + x];
      slot[u] = v.dir[ok[u] ? d : 0u];
    }
#pragma unroll
    for (int u = 0; u < WS_UNROLL; u++)
    {
      if (!ok[u])
        continue;
      if (slot[u] < WS_WANTED)
        v.pool[static_cast<uint64_t>(slot[u]) * WS_TILE_WORDS + e[u]] = bits[u];
      else if (bits[u] != v.init)
        atomicAdd(v.ctr + WC_FORGOTTEN, 1ull);
    }
  }
}

// K: world index of the voxel (0, 0, 0) of the NEW window
__global__ __launch_bounds__(WS_THREADS) void k_world_get(const View v, const Rim rim, uint32_t* __restrict__ map, int32_t sx, int32_t sy, int64_t k0, int64_t k1, int64_t k2)
{
  const uint64_t n = rim.first[3], stride = static_cast<uint64_t>(gridDim.x) * WS_THREADS;
  for (uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * WS_THREADS + threadIdx.x; t0 < n; t0 += WS_UNROLL * stride)
  {
    uint64_t i[WS_UNROLL];
    uint32_t slot[WS_UNROLL], e[WS_UNROLL];
#pragma unroll
    for (int u = 0; u < WS_UNROLL; u++)
    {
      const uint64_t t = t0 + u * stride;
      int32_t x, y, z;
      rim_voxel(rim, t < n ? t : t0, x, y, z);
      uint32_t d = 0;
      const bool ok = world_cell(v, k0 + x, k1 + y, k2 + z, d, e[u]) && t < n;
      i[u] = (static_cast<uint64_t>(z) * sy + y) * sx + x;
      slot[u] = ok ? v.dir[d] : WS_EMPTY;
    }
#pragma unroll
    for (int u = 0; u < WS_UNROLL; u++)
      if (slot[u] < WS_WANTED)
        map[i[u]] = v.pool[static_cast<uint64_t>(slot[u]) * WS_TILE_WORDS + e[u]];
  }
}

// the world cell of an a-priori point beyond the window; false for a point inside the window (k_apriori's), outside the box, or whose
// floor is not finite or beyond +-2^30
__device__ __forceinline__ bool far_point_cell(const View& v, const vk::MapGeom& mg, const float* __restrict__ xyz, uint32_t t, int64_t k0, int64_t k1, int64_t k2, uint32_t& d, uint32_t& e)
{
  const float f[3] = {apriori_cell(xyz[3 * t + 0], mg.off[0], mg.vs_inv), apriori_cell(xyz[3 * t + 1], mg.off[1], mg.vs_inv), apriori_cell(xyz[3 * t + 2], mg.off[2], mg.vs_inv)};
  const float lim = static_cast<float>(WS_K_LIMIT);
  for (int a = 0; a < 3; a++)
    if (!(fabsf(f[a]) <= lim))  // (NaN fails the comparison)
      return false;
  const int32_t ox = static_cast<int32_t>(f[0]), oy = static_cast<int32_t>(f[1]), oz = static_cast<int32_t>(f[2]);
  if (ox >= 0 && ox < mg.sx && oy >= 0 && oy < mg.sy && oz >= 0 && oz < mg.sz)
    return false;
  return world_cell(v, k0 + ox, k1 + oy, k2 + oz, d, e);
}

__global__ __launch_bounds__(WS_THREADS) void k_world_mark_points(const View v, const vk::MapGeom mg, const float* __restrict__ xyz, uint32_t n, int64_t k0, int64_t k1, int64_t k2,
                                                                 uint32_t* __restrict__ list, uint32_t list_cap)
{
  const uint32_t t = blockIdx.x * WS_THREADS + threadIdx.x;
  uint32_t d, e;
  if (t < n && far_point_cell(v, mg, xyz, t, k0, k1, k2, d, e))
    want_tile(v, d, list, list_cap);
}

// (behind a k_world_claim that the driver has seen to fit: every tile of a far point exists)
__global__ __launch_bounds__(WS_THREADS) void k_world_put_points(const View v, const vk::MapGeom mg, const float* __restrict__ xyz, uint32_t n, int64_t k0, int64_t k1, int64_t k2)
{
  if (blockIdx.x == 0 && threadIdx.x == 0)
    world_commit(v, false);
  const uint32_t t = blockIdx.x * WS_THREADS + threadIdx.x;
  uint32_t d, e;
  if (t < n && far_point_cell(v, mg, xyz, t, k0, k1, k2, d, e))
  {
    const uint32_t slot = v.dir[d];
    if (slot < WS_WANTED)
      v.pool[static_cast<uint64_t>(slot) * WS_TILE_WORDS + e] = 0x7F800000u;  // +inf
  }
}

// dst[(z * n1 + y) * n0 + x] = W(lo + (x, y, z)); map: the window, its voxel (0, 0, 0) at world index K
__global__ __launch_bounds__(WS_THREADS) void k_world_gather(const View v, const uint32_t* __restrict__ map, int32_t sx, int32_t sy, int32_t sz, int64_t k0, int64_t k1, int64_t k2, int64_t l0, int64_t l1,
                                                            int64_t l2, uint32_t n0, uint32_t n1, uint64_t n, uint32_t* __restrict__ dst)
{
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * WS_THREADS;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * WS_THREADS + threadIdx.x; t < n; t += stride)
  {
    const uint64_t row = t / n0, pl = row / n1;
    const int64_t gx = l0 + static_cast<int64_t>(t - row * n0), gy = l1 + static_cast<int64_t>(row - pl * n1), gz = l2 + static_cast<int64_t>(pl);
    const int64_t ix = gx - k0, iy = gy - k1, iz = gz - k2;
    uint32_t bits = v.init, d, e;
    if (ix >= 0 && ix < sx && iy >= 0 && iy < sy && iz >= 0 && iz < sz)
      bits = map[(static_cast<uint64_t>(iz) * sy + iy) * sx + ix];
    else if (world_cell(v, gx, gy, gz, d, e))
    {
      const uint32_t slot = v.dir[d];
      if (slot < WS_WANTED)
        bits = v.pool[static_cast<uint64_t>(slot) * WS_TILE_WORDS + e];
    }
    dst[t] = bits;
  }
}

}  // namespace vws
