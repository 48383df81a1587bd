// Ray-cast map update (K14, K15) and separated-background-cluster removal (K16, K17, K6') kernels.
//
// raycast_cloud (vofod_nodelet.cpp:1397-1605): one lane per LiDAR ray walks the voxel map with the
// Amanatides-Woo DDA of VoxelMap::forEachRay (voxel_map.cpp:229-263) and adds the in-voxel path length
// to the raycast map with hardware atomics; a single fused streaming pass then applies the
// exponential pull of un-flagged traversed voxels towards scores/ray and clears flags + raycast map.
//
// The role is ONE kernel template, k_raycast_t<MOTION, ALIGNED16, Acc>: one front, one walk, one run merge, and two things that
// vary - where the beam comes from (MOTION) and what is added (Acc).  The driver launches five instantiations under three profiler
// names: k_raycast (rigid, float), k_raycast_motion (float, two table alignments), k_raycast_exact (units; rigid and two alignments).
//
// Motion-compensated rays (include/vofod.h, MOTION COMPENSATION, vofod_set_raycast_motion; MOTION): a scan that carries a pose per
// measurement column.  Pixel i = row * width + col was measured in column m = (col + shift_by_row[row]) mod width (the handle keeps
// the shifts reduced to [0, width)), and with T = col_tfs[m], d = lut_dirs[3i..], o = lut_offs[3i..], every operation IEEE float32,
// rounded once, nothing fused:
//   d'[k] = ((T[k][0]*d[0]) + (T[k][1]*d[1])) + (T[k][2]*d[2])
//   o'[k] = (((T[k][0]*o[0]) + (T[k][1]*o[1])) + (T[k][2]*o[2])) + T[k][3]
// From there on the ray is the rigid one with d', o' in place of the LUT entries: dir = R d', start = (R o') + t in the association
// of the kernel's front, the gates, the length, the in-limits test of the ray's own start, the DDA.  An identity table gives d' == d
// and o' == o as values (a zero may change sign; the walk reads only the magnitude of a zero component and compares it).  The two
// matrices are never multiplied together; no exclude-box rule (the reference casts the airframe's short rays too, length <= 0 stops
// them).  New against the rigid front: row = idx / width (one 32-bit division), m with one compare for the wrap, the pose, the two
// transforms.  Lanes of a wave are 64 consecutive columns of one ring: their 64 poses are 3 KB of consecutive memory except where m
// wraps or the wave spans a row end.  ALIGNED16: the table is 16-byte aligned and a pose is three 16-byte loads, otherwise twelve
// 4-byte loads (column_pose.h: load_pose).
//
// Exact raycast accumulation (include/vofod.h, EXACT RAYCAST ACCUMULATION, vofod_set_raycast_exact; Acc = AccUnits): path lengths
// summed as fixed-point units in uint32 instead of float atomics.  With S = log2(units per metre) and QMAX of the handle
// (ray_exact_scale below), a piece dd - the float min(dist, length) - prev of the walk, unchanged - counts
//   q = min(rint(dd * 2^S), QMAX)          (the product is exact, rint is to nearest even; q == 0 leaves no trace)
// and U[v] = sum of q over the pieces laid into voxel v, in the raycast map's own buffer.  Integer addition is associative and
// n_pixels * QMAX fits in 32 bits, so U does not depend on the order of the atomics nor on how the wave groups its lanes into runs:
// two passes of one scan, and the passes of two handles, end with the same bits.  The float view of a voxel is r = float(U) * 2^-S
// (the conversion rounds to nearest even, the scaling is exact); the sweep, the old rule's max_val and vofod_read_map read that r.
// An all-zero map is the same map in both representations, so the driver's ray_dirty / fill_map bookkeeping is shared.
//
// updateSeparatedBGClusters (vofod_nodelet.cpp:1126-1277): thresholded voxels are enumerated in the
// reference's x-outer/z-inner order through a transposed occupancy bitmap, voxelised with the counted
// grid (positional count quirk), clustered, and unsure clusters are erased with an
// order-independent atomic compare-and-swap application of m <- w1*m + w2*ray per (voxel, offset) pair.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "column_pose.h"
#include "kernels_voxelize.h"

namespace vr
{
using namespace vk;

struct RayParams
{
  float R[9];
  float origin[3];
  float max_dist, min_intensity, voxel_size;
  uint32_t n;
};

__device__ __forceinline__ int c2i(float x, float off, float inv) { return static_cast<int>(floorf(__fmul_rn(__fsub_rn(x, off), inv))); }

constexpr int RX_MAX_LOG2 = 24;  // the cap of S: 2^-24 m is below anything a float piece of a metre resolves

// S and QMAX of a handle (host, double): S is the largest integer in [0, 24] with n_pixels * (floor(2 * vs * 2^S) + 1) <= 2^32 - 1,
// QMAX = floor(2 * vs * 2^S).  False when not even S = 0 fits (a voxel size beyond any sensor): the switch is refused then.
inline bool ray_exact_scale(float voxel_size, int hrays, int vrays, int32_t& S, uint32_t& qmax)
{
  const double vs = static_cast<double>(voxel_size);
  const double n_pixels = static_cast<double>(hrays) * static_cast<double>(vrays);
  for (int s = RX_MAX_LOG2; s >= 0; s--)
  {
    const double q = std::floor(2.0 * vs * std::ldexp(1.0, s));
    if (n_pixels * (q + 1.0) <= 4294967295.0)
    {
      S = s;
      qmax = static_cast<uint32_t>(q);
      return true;
    }
  }
  return false;
}

struct ExactScale
{
  float scale;    // 2^S
  uint32_t qmax;  // QMAX
};

// the units of one piece: min(rint(dd * 2^S), QMAX); a NaN piece counts nothing
__device__ __forceinline__ uint32_t rx_units(float dd, const ExactScale& xs)
{
  const float x = rintf(__fmul_rn(dd, xs.scale));
  // (clamped into [0, 2^32 - 256] before the conversion: fmaxf returns the other operand for a NaN)
  const float c = fminf(fmaxf(x, 0.0f), 4294967040.0f);
  return min(static_cast<uint32_t>(c), xs.qmax);
}

// What a pass adds, and how the sweep reads it back.  T is the word of the raycast map; piece() is what a lane lays for a step
// of length dd (zero: no trace), add() joins two pieces of one run, commit() is the atomic of a run's last lane; touched() and
// metres() are the sweep's view of a word.
struct AccFloat  // in-voxel path lengths as floats: the sum depends on the order of the atomics
{
  using T = float;
  __device__ __forceinline__ T piece(float dd) const { return dd; }
  __device__ static __forceinline__ T add(T a, T b) { return __fadd_rn(a, b); }
  __device__ static __forceinline__ void commit(T* cell, T run) { unsafeAtomicAdd(cell, run); }
  __device__ static __forceinline__ bool touched(T r) { return r > 0.0f; }
  __device__ static __forceinline__ float metres(T r, float) { return r; }
};
struct AccUnits  // fixed-point units, quantised per lane BEFORE the run merge: 64 lanes * QMAX fits, nobody reads the atomic's result
{
  using T = uint32_t;
  ExactScale xs;
  __device__ __forceinline__ T piece(float dd) const { return rx_units(dd, xs); }
  __device__ static __forceinline__ T add(T a, T b) { return a + b; }
  __device__ static __forceinline__ void commit(T* cell, T run) { (void)__hip_atomic_fetch_add(cell, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ static __forceinline__ bool touched(T u) { return u != 0u; }
  __device__ static __forceinline__ float metres(T u, float inv_scale) { return __fmul_rn(__uint2float_rn(u), inv_scale); }  // the float view
};

// d' and o' of the definition above
__device__ __forceinline__ void ray_pose_apply(const Pose& T, const float d[3], const float o[3], float dm[3], float om[3])
{
  const float4 rows[3] = {T.r0, T.r1, T.r2};
#pragma unroll
  for (int k = 0; k < 3; k++)
  {
    const float4 t = rows[k];
    dm[k] = __fadd_rn(__fadd_rn(__fmul_rn(t.x, d[0]), __fmul_rn(t.y, d[1])), __fmul_rn(t.z, d[2]));
    om[k] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(t.x, o[0]), __fmul_rn(t.y, o[1])), __fmul_rn(t.z, o[2])), t.w);
  }
}

// one axis of forEachRay's set-up (voxel_map.cpp:229-263):
//   tmax / tdelta as in the reference (the per-ray sequence tmax += tdelta is kept: same floats, same voxel sequence);
//   rem   = steps left on the axis before the walk would leave the map (cur == last of the reference <=> rem == 0);
//   lstep = step * stride: what a step on the axis adds to the linear index of the current voxel.
__device__ __forceinline__ void ray_axis(float dir, float start, int cur, int lim, int lstride, float vs, float off, float half, float& tmax, float& tdelta, int& rem, int& lstep)
{
  const float absdir = fabsf(dir);
  const int step = (dir > 0.0f) - (dir < 0.0f);
  tdelta = __fmul_rn(__fdiv_rn(1.0f, absdir), vs);
  const float ctr = __fadd_rn(__fmul_rn(__fadd_rn(static_cast<float>(cur), 0.5f), vs), off);
  const float ctr_offset = __fsub_rn(ctr, start);
  tmax = __fdiv_rn(__fadd_rn(half, __fmul_rn(static_cast<float>(step), ctr_offset)), absdir);
  rem = step > 0 ? lim - 1 - cur : cur;  // (last = step > 0 ? lim - 1 : 0, :246)
  lstep = step * lstride;
}

// one step of the segmented inclusive sum: lanes whose flag is clear add the value CTRL brings, flags are or-ed
template <class Acc, int CTRL, int MASK>
__device__ __forceinline__ void ray_segstep(typename Acc::T& run, uint32_t& f)
{
  const auto t = __builtin_bit_cast(typename Acc::T, dpp_mov0<CTRL, MASK>(__builtin_bit_cast(uint32_t, run)));
  const uint32_t ft = dpp_mov0<CTRL, MASK>(f);
  run = f ? run : Acc::add(run, t);
  f |= ft;
}

// Neighbouring lanes are neighbouring azimuth columns of one ring: their walks visit almost the same voxels in almost the same
// order, so per DDA step the wave merges runs of lanes that sit in the same voxel and issues one atomic per run instead of one per
// lane: a segmented inclusive sum with DPP moves (row_shr 1 / 2 / 4 / 8, row_bcast 15 / 31: vector ALU only, no LDS crossbar).  The
// last lane of a run holds its total and issues the atomic.  key: the lane's voxel, 0xffffffff where it lays nothing.  Called by
// every lane of the wave; returns whether this lane added.
template <class Acc>
__device__ __forceinline__ bool ray_merge_runs(uint32_t key, typename Acc::T piece, int lane, typename Acc::T* __restrict__ cells)
{
  const uint32_t kprev = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(~key), static_cast<int>(key), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
  const bool head = lane == 0 || kprev != key;
  uint32_t f = head ? 1u : 0u;
  typename Acc::T run = piece;
  ray_segstep<Acc, 0x111, 0xf>(run, f);
  ray_segstep<Acc, 0x112, 0xf>(run, f);
  ray_segstep<Acc, 0x114, 0xf>(run, f);
  ray_segstep<Acc, 0x118, 0xf>(run, f);
  ray_segstep<Acc, 0x142, 0xa>(run, f);
  ray_segstep<Acc, 0x143, 0xc>(run, f);
  const unsigned long long H = __ballot(head);
  const bool tail = lane == 63 || ((H >> (lane + 1)) & 1ull);
  if (tail && key != 0xffffffffu)  // (every lane of such a run laid a non-zero piece)
  {
    Acc::commit(&cells[key], run);
    return true;
  }
  return false;
}

// What bounds the float pass (round 5, profiles/r05_raycast_variants.txt, one OS1-128 scan at 0.25 m): the float atomics.  The same
// kernel without the accumulation: 78.5 us; with plain stores to the same addresses: 83.7 us; with the atomics: 218-222 us.  Tried
// and not kept: two / four rays per lane for ILP (218.0 / 241.1 us against 219.8), and dealing the rays to the XCDs by azimuth sector
// so that all rays through one wedge of the map are walked on one XCD and its L2 keeps the wedge's lines (221.7 us, 1 164 us at
// OS2-128 x 2048 / 0.1 m against 1 168) - neither where the rays sit nor which L2 they go through changes what ~4 M single-float
// read-modify-writes per scan cost.  The run merging stays: without it there would be several times as many.
//
// MOTION: poses, shift and width are read; otherwise they are not (nullptr, 0) and the driver instantiates <false, true, .> only.
// One ray per lane; every lane of every wave stays in the loop (the DPP merge and its ballots need the full wave: a lane beyond n or
// behind a gate is carried as an inactive ray, never returned early).  No LDS and no scratch: the walk state lives in scalar locals
// of the kernel and the step is written out in its body, not in a function on a struct of the state - behind a reference the
// compiler folds `s2 ? rem2 : (s1 ? rem1 : rem0)` into one load through a selected ADDRESS, cannot split the struct into registers
// any more and parks it in LDS (64 B per lane, read and written every step).
template <bool MOTION, bool ALIGNED16, class Acc>
__global__ __launch_bounds__(256) void k_raycast_t(const RayParams rp, const MapGeom mg, const Acc acc, const char* __restrict__ intensity, const char* __restrict__ range,
                                                   uint64_t stride, const float* __restrict__ lut_dirs, const float* __restrict__ lut_offs, const uint8_t* __restrict__ mask,
                                                   const float* __restrict__ poses, const uint32_t* __restrict__ shift, uint32_t width, typename Acc::T* __restrict__ cells,
                                                   uint32_t* __restrict__ any_hit)
{
  const int lane = threadIdx.x & 63;
  const uint32_t idx_raw = blockIdx.x * blockDim.x + threadIdx.x;
  bool alive = idx_raw < rp.n;
  const uint32_t idx = alive ? idx_raw : 0u;  // (a lane beyond n reads pixel 0: row 0, a column and a pose inside the tables)
  const float inten = *reinterpret_cast<const float*>(intensity + static_cast<uint64_t>(idx) * stride);
  const uint32_t rng = *reinterpret_cast<const uint32_t*>(range + static_cast<uint64_t>(idx) * stride);
  if (inten < rp.min_intensity || (!mask[idx] && rng == 0))  // vofod_nodelet.cpp:1449
    alive = false;
  float dm[3] = {lut_dirs[3 * idx], lut_dirs[3 * idx + 1], lut_dirs[3 * idx + 2]};
  float om[3] = {lut_offs[3 * idx], lut_offs[3 * idx + 1], lut_offs[3 * idx + 2]};
  if constexpr (MOTION)
  {
    // the pose of the pixel's measurement column, applied to the beam's direction and offset
    const uint32_t row = idx / width;
    const uint32_t m = measurement_column(row, idx - row * width, width, shift);
    const Pose T = load_pose<ALIGNED16>(poses, m);
    const float d[3] = {dm[0], dm[1], dm[2]}, o[3] = {om[0], om[1], om[2]};
    ray_pose_apply(T, d, o, dm, om);
  }
  // the call's tf
  float dir[3], start[3];
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
    const float* R = &rp.R[3 * r];
    dir[r] = __fadd_rn(__fadd_rn(__fmul_rn(R[0], dm[0]), __fmul_rn(R[1], dm[1])), __fmul_rn(R[2], dm[2]));
    start[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[0], om[0]), __fmul_rn(R[1], om[1])), __fmul_rn(R[2], om[2])), rp.origin[r]);
  }
  // the walk's set-up: length, first voxel, in-limits test, then forEachRay's state one axis at a time
  const float ray_dist = __fmul_rn(0.001f, static_cast<float>(rng));                                             // :1455-1456
  const float length = ray_dist == 0.0f ? rp.max_dist : fminf(__fsub_rn(ray_dist, rp.voxel_size), rp.max_dist);  // :1457
  const int c0 = c2i(start[0], mg.off[0], mg.vs_inv), c1 = c2i(start[1], mg.off[1], mg.vs_inv), c2 = c2i(start[2], mg.off[2], mg.vs_inv);
  if (c0 < 0 || c0 >= mg.sx || c1 < 0 || c1 >= mg.sy || c2 < 0 || c2 >= mg.sz)  // :1482
    alive = false;
  const float half = mg.vs / 2.0f;
  float tmax0, tmax1, tmax2, tdelta0, tdelta1, tdelta2;
  int rem0, rem1, rem2, lstep0, lstep1, lstep2;
  ray_axis(dir[0], start[0], c0, mg.sx, 1, mg.vs, mg.off[0], half, tmax0, tdelta0, rem0, lstep0);
  ray_axis(dir[1], start[1], c1, mg.sy, mg.sx, mg.vs, mg.off[1], half, tmax1, tdelta1, rem1, lstep1);
  ray_axis(dir[2], start[2], c2, mg.sz, mg.sx * mg.sy, mg.vs, mg.off[2], half, tmax2, tdelta2, rem2, lstep2);
  uint32_t lin = alive ? static_cast<uint32_t>((static_cast<uint64_t>(c2) * mg.sy + c1) * mg.sx + c0) : 0u;
  float prev = 0.0f;
  bool active = alive && 0.0f < length;
  // the loop is kept wave-uniform
  bool any = false;
  while (__ballot(active))
  {
    // the axis of the smallest tmax, first minimum on ties (Eigen's minCoeff, voxel_map.cpp:252)
    const bool s1 = tmax1 < tmax0;
    const float m01 = s1 ? tmax1 : tmax0;
    const bool s2 = tmax2 < m01;
    const float dist = s2 ? tmax2 : m01;
    const float dd = __fsub_rn(fminf(dist, length), prev);
    const typename Acc::T piece = active ? acc.piece(dd) : typename Acc::T(0);
    const uint32_t key = piece != typename Acc::T(0) ? lin : 0xffffffffu;
    const int remi = s2 ? rem2 : (s1 ? rem1 : rem0);
    const bool adv = active & (remi != 0);
    const bool a2 = adv & s2, a1 = adv & s1 & !s2, a0 = adv & !s1 & !s2;
    tmax0 = a0 ? __fadd_rn(tmax0, tdelta0) : tmax0;
    tmax1 = a1 ? __fadd_rn(tmax1, tdelta1) : tmax1;
    tmax2 = a2 ? __fadd_rn(tmax2, tdelta2) : tmax2;
    rem0 -= a0 ? 1 : 0;
    rem1 -= a1 ? 1 : 0;
    rem2 -= a2 ? 1 : 0;
    lin += static_cast<uint32_t>(a0 ? lstep0 : (a1 ? lstep1 : (a2 ? lstep2 : 0)));
    prev = active ? dist : prev;
    active = adv & (dist < length);
    any |= ray_merge_runs<Acc>(key, piece, lane, cells);
  }
  if (any)
    *any_hit = 1u;
}

// max of a non-negative float array (order-preserving on the raw bits), for the old update rule (:1542)
__global__ __launch_bounds__(256) void k_max_nonneg(const float* __restrict__ v, uint64_t n, uint32_t* out)
{
  uint32_t m = 0;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const float x = v[i];
    if (x > 0.0f)
      m = max(m, __float_as_uint(x));
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1)
    m = max(m, __shfl_xor(m, s));
  if ((threadIdx.x & 63) == 0 && m)
    atomicMax(out, m);
}

// integer max of U, for the old update rule (:1542): the host converts it to max_val by the rule of the float view
__global__ __launch_bounds__(256) void k_max_units(const uint32_t* __restrict__ u, uint64_t n, uint32_t* out)
{
  uint32_t m = 0;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
    m = max(m, u[i]);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1)
    m = max(m, __shfl_xor(m, s));
  if ((threadIdx.x & 63) == 0 && m)
    atomicMax(out, m);
}

struct SweepParams
{
  float its_diff;
  float ray_score;
  float weighting_factor;  // new rule: coef / (sqrt(3)*vs)          (:1555-1556)
  float weight;            // old rule: coef                          (:1578)
  float max_val;           // old rule normaliser                      (:1542)
  int32_t new_rule;
};

// K15: fused update sweep (:1557-1602).  Reads flags + raycast (+ map where a ray passed), writes map,
// clears flags and the raycast accumulator (to zero bits).  Stores are issued only where a value actually changes.
// Launched as k_ray_sweep (AccFloat: r is the word itself, inv_scale is not read) and k_ray_sweep_exact (AccUnits: r = float(U) * 2^-S).
template <class Acc>
__global__ __launch_bounds__(256) void k_ray_sweep_t(const SweepParams sp, float inv_scale, uint64_t n, float* __restrict__ map, float* __restrict__ flags,
                                                     typename Acc::T* __restrict__ cells)
{
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const float flag = flags[i];
    const typename Acc::T c = cells[i];
    if (flag == 0.0f && Acc::touched(c))
    {
      const float r = Acc::metres(c, inv_scale);
      float w1;
      if (sp.new_rule)
      {
        const float n_int = __fmul_rn(sp.weighting_factor, r);
        w1 = static_cast<float>(exp2(static_cast<double>(__fmul_rn(-sp.its_diff, n_int))));  // std::pow(2, x) evaluates in double
      }
      else
      {
        const float norm_val = __fdiv_rn(r, sp.max_val);
        const float w_single = __fmul_rn(sp.weight, __fsqrt_rn(norm_val));
        w1 = fminf(fmaxf(powf(__fsub_rn(1.0f, w_single), sp.its_diff), 0.0f), 1.0f);
      }
      const float w2 = __fsub_rn(1.0f, w1);
      map[i] = __fadd_rn(__fmul_rn(w1, map[i]), __fmul_rn(w2, sp.ray_score));
    }
    if (flag != 0.0f)
      flags[i] = 0.0f;
    if (c != typename Acc::T(0))
      cells[i] = typename Acc::T(0);
  }
}

// ------------------------------------------------------------------ generic exclusive scan (u32)
constexpr int GS_EPT = 8;
constexpr int GS_EPB = 256 * GS_EPT;

__global__ __launch_bounds__(256) void k_gscan_a(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ bsum)
{
  const uint32_t base = blockIdx.x * GS_EPB + threadIdx.x * GS_EPT;
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < GS_EPT; k++)
    if (base + k < n)
      c += in[base + k];
  __shared__ uint32_t lds4[4];
  uint32_t total;
  block_excl_scan_256(c, lds4, &total);
  if (threadIdx.x == 0)
    bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_gscan_b(uint32_t* bsum, uint32_t nblk, uint32_t* total_out)
{
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry_s;
  if (threadIdx.x == 0)
    carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nblk; base += 1024)
  {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nblk ? bsum[i] : 0;
    const uint32_t incl = wave_incl_scan(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 63)
      wsum[wave] = incl;
    __syncthreads();
    uint32_t off = carry_s;
    for (int w = 0; w < wave; w++)
      off += wsum[w];
    if (i < nblk)
      bsum[i] = off + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023)
      carry_s = off + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0 && total_out)
    *total_out = carry_s;
}

// out has n+1 entries: out[i] = sum(in[0..i)), out[n] = total
__global__ __launch_bounds__(256) void k_gscan_c(const uint32_t* __restrict__ in, uint32_t n, const uint32_t* __restrict__ bsum, uint32_t* __restrict__ out)
{
  const uint32_t base = blockIdx.x * GS_EPB + threadIdx.x * GS_EPT;
  uint32_t vals[GS_EPT];
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < GS_EPT; k++)
  {
    vals[k] = (base + k < n) ? in[base + k] : 0u;
    c += vals[k];
  }
  __shared__ uint32_t lds4[4];
  uint32_t total;
  uint32_t run = block_excl_scan_256(c, lds4, &total) + bsum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < GS_EPT; k++)
  {
    if (base + k < n)
      out[base + k] = run;
    run += vals[k];
    if (base + k + 1 == n)
      out[n] = run;
  }
}

// ------------------------------------------------------------------ sepclusters

// K16: voxelsAsVoxelPC (voxel_map.cpp:187-212) enumerates the thresholded voxels x-outer / y / z-inner.  One lane
// owns one (x,y) column; lanes of a wave are consecutive in x, so the occupancy word of a (y,z) row is fetched
// once per wave and every lane tests its own bit.  Pass 1 counts the set bits per column into x-major order,
// a scan turns the counts into each column's first position, pass 2 writes the points (x,y,z as floats, map value)
// and the "sure" flags the counted grid's positional count consumes.
__global__ __launch_bounds__(256) void k_col_count(const MapGeom mg, const unsigned long long* __restrict__ mapbits, uint32_t* __restrict__ colcount_t)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ncol = static_cast<uint32_t>(mg.sx) * mg.sy;
  if (t >= ncol)
    return;
  const uint32_t x = t % mg.sx, y = t / mg.sx;
  const uint64_t plane = static_cast<uint64_t>(mg.sx) * mg.sy;
  uint32_t c = 0;
  uint64_t li = t;
  for (int z = 0; z < mg.sz; z++, li += plane)
    c += static_cast<uint32_t>((mapbits[li >> 6] >> (li & 63)) & 1ull);
  colcount_t[x * mg.sy + y] = c;
}

// voxelsAsPC (voxel_map.cpp:157-183): the debug clouds of the nodelet (background: map > new_obstacles; sure air: !(map >
// frontiers), vofod_nodelet.cpp:999-1013) in the reference's order, x outer / y / z inner, as world coordinates + map value.
// Same column walk as above, on the float map itself: ((m > threshold) == greater_than) needs no occupancy image.
__global__ __launch_bounds__(256) void k_col_count_thr(const MapGeom mg, const float* __restrict__ map, float threshold, int greater_than, uint32_t* __restrict__ colcount_t)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ncol = static_cast<uint32_t>(mg.sx) * mg.sy;
  if (t >= ncol)
    return;
  const uint32_t x = t % mg.sx, y = t / mg.sx;
  const uint64_t plane = static_cast<uint64_t>(mg.sx) * mg.sy;
  uint32_t c = 0;
  uint64_t li = t;
  for (int z = 0; z < mg.sz; z++, li += plane)
    c += ((map[li] > threshold) == (greater_than != 0)) ? 1u : 0u;
  colcount_t[x * mg.sy + y] = c;
}

__global__ __launch_bounds__(256) void k_col_emit_xyzi(const MapGeom mg, const float* __restrict__ map, float threshold, int greater_than, const uint32_t* __restrict__ colbase_t,
                                                       uint32_t cap, float4* __restrict__ out)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ncol = static_cast<uint32_t>(mg.sx) * mg.sy;
  if (t >= ncol)
    return;
  const uint32_t x = t % mg.sx, y = t / mg.sx;
  const uint64_t plane = static_cast<uint64_t>(mg.sx) * mg.sy;
  uint32_t pos = colbase_t[x * mg.sy + y];
  if (colbase_t[x * mg.sy + y + 1] == pos)
    return;  // empty column
  const float cx = __fadd_rn(__fmul_rn(__fadd_rn(static_cast<float>(x), 0.5f), mg.vs), mg.off[0]);  // idxToCoord voxel_map.cpp:610-613
  const float cy = __fadd_rn(__fmul_rn(__fadd_rn(static_cast<float>(y), 0.5f), mg.vs), mg.off[1]);
  uint64_t li = t;
  for (int z = 0; z < mg.sz; z++, li += plane)
  {
    const float m = map[li];
    if ((m > threshold) == (greater_than != 0))
    {
      if (pos < cap)
        out[pos] = make_float4(cx, cy, __fadd_rn(__fmul_rn(__fadd_rn(static_cast<float>(z), 0.5f), mg.vs), mg.off[2]), m);
      pos++;
    }
  }
}

__global__ __launch_bounds__(256) void k_col_emit(const MapGeom mg, const float* __restrict__ map, const unsigned long long* __restrict__ mapbits,
                                                  const uint32_t* __restrict__ colbase_t, float thr_sure, float* __restrict__ px, float* __restrict__ py,
                                                  float* __restrict__ pz, float* __restrict__ pi, uint32_t* __restrict__ sure)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ncol = static_cast<uint32_t>(mg.sx) * mg.sy;
  if (t >= ncol)
    return;
  const uint32_t x = t % mg.sx, y = t / mg.sx;
  const uint64_t plane = static_cast<uint64_t>(mg.sx) * mg.sy;
  uint32_t pos = colbase_t[x * mg.sy + y];
  if (colbase_t[x * mg.sy + y + 1] == pos)
    return;  // empty column
  uint64_t li = t;
  for (int z = 0; z < mg.sz; z++, li += plane)
    if ((mapbits[li >> 6] >> (li & 63)) & 1ull)
    {
      const float m = map[li];
      px[pos] = static_cast<float>(x);
      py[pos] = static_cast<float>(y);
      pz[pos] = static_cast<float>(z);
      pi[pos] = m;
      sure[pos] = m > thr_sure ? 1u : 0u;
      pos++;
    }
}

// per-voxel point counts of the weighted emission -> u32 array
__global__ __launch_bounds__(256) void k_voxel_counts(const FrameHdr* hdr, const float4* __restrict__ pts, uint32_t* __restrict__ out)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < hdr->V)
    out[v] = __float_as_uint(pts[v].w);
}

// K6': voxel_grid_counted.cpp:185-191: range_k = #{input positions p in [first_k, last_k): intensity_p > thr}
// with [first_k,last_k) the run of voxel k in the sorted index vector = exclusive prefix of the voxel sizes.
__global__ __launch_bounds__(256) void k_counted_range(const FrameHdr* hdr, const uint32_t* __restrict__ first, const uint32_t* __restrict__ sure_prefix, uint32_t n_points,
                                                       float4* __restrict__ pts)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= hdr->V)
    return;
  const uint32_t a = min(first[v], n_points), b = min(first[v + 1], n_points);
  pts[v].w = __uint_as_float(sure_prefix[b] - sure_prefix[a]);
}

// intensity > threshold flags of an arbitrary strided column (stateless counted grid)
__global__ __launch_bounds__(256) void k_flag_over(const char* __restrict__ col, uint64_t stride, uint32_t n, float thr, uint32_t* __restrict__ out)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    out[i] = *reinterpret_cast<const float*>(col + static_cast<uint64_t>(i) * stride) > thr ? 1u : 0u;
}

// sum of `range` per cluster (vofod_nodelet.cpp:1175-1183) + "any cluster sure" flag
__global__ __launch_bounds__(256) void k_cluster_sure(const FrameHdr* hdr, const float4* __restrict__ pts, const uint32_t* __restrict__ labels, uint32_t* __restrict__ n_sure)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t key = 0xffffffffu, r = 0;
  if (v < hdr->V)
  {
    r = __float_as_uint(pts[v].w);
    if (r)
      key = labels[v];
  }
  // consecutive voxels mostly share the cluster: one atomic per run of equal labels inside the wave
  int end;
  const bool head = run_heads(key, lane, end);
#pragma unroll
  for (int s2 = 1; s2 < 64; s2 <<= 1)
  {
    const uint32_t t = __shfl_down(r, s2);
    if (lane + s2 < end)
      r += t;
  }
  if (head && key != 0xffffffffu)
    atomicAdd(&n_sure[key], r);
}

__global__ __launch_bounds__(256) void k_any_sure(const FrameHdr* hdr, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ n_sure, uint32_t min_sure, uint32_t* out)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= hdr->V)
    return;
  if (labels[v] == v && n_sure[v] >= min_sure)
    out[0] = 1u;
  if (labels[v] == v)
    atomicMax(&out[1], n_sure[v]);
}

struct EraseParams
{
  float w1, w2, update_val;
  uint32_t min_sure;
  int32_t n_offsets;
};

// K17: erase stencil (vofod_nodelet.cpp:1244-1272).  Every (voxel of an unsure cluster, offset) pair applies
// m <- w1*m + w2*ray once; all applications are the same function, so applying them with an atomic
// compare-and-swap in any order reproduces the reference's sequential result bit for bit.
__global__ __launch_bounds__(256) void k_sep_erase(const EraseParams ep, const MapGeom mg, const FrameHdr* hdr, const float4* __restrict__ pts,
                                                   const uint32_t* __restrict__ labels, const uint32_t* __restrict__ n_sure, const int* __restrict__ offsets,
                                                   float* __restrict__ map)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= hdr->V)
    return;
  if (n_sure[labels[v]] >= ep.min_sure)
    return;
  const float4 p = pts[v];
  const int pos[3] = {static_cast<int>(p.x), static_cast<int>(p.y), static_cast<int>(p.z)};  // cast<int>() truncates (:1252)
  // (the stencil - thousands of offsets at small voxel sizes - is dealt over blockIdx.y: the voxels of unsure clusters are few,
  // one thread per voxel walking the whole stencil left the chip empty: 2.4 ms at 0.1 m)
  for (int o = blockIdx.y; o < ep.n_offsets; o += gridDim.y)
  {
    const int x = pos[0] + offsets[3 * o], y = pos[1] + offsets[3 * o + 1], z = pos[2] + offsets[3 * o + 2];
    if (x < 0 || x >= mg.sx || y < 0 || y >= mg.sy || z < 0 || z >= mg.sz)
      continue;
    uint32_t* a = reinterpret_cast<uint32_t*>(&map[(static_cast<uint64_t>(z) * mg.sy + y) * mg.sx + x]);
    uint32_t old = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (true)
    {
      const float m = __uint_as_float(old);
      const float nm = __fadd_rn(__fmul_rn(ep.w1, m), __fmul_rn(ep.w2, ep.update_val));
      const uint32_t prev = atomicCAS(a, old, __float_as_uint(nm));
      if (prev == old)
        break;
      old = prev;
    }
  }
}

// device buffers owned by the sepclusters stage
struct SepState
{
  unsigned long long* d_tbits = nullptr;
  uint32_t* d_tpop = nullptr;     // word popcounts, then reused
  uint32_t* d_tprefix = nullptr;  // n_words + 1
  uint32_t* d_bsum = nullptr;
  size_t words_cap = 0;
  float *d_px = nullptr, *d_py = nullptr, *d_pz = nullptr, *d_pi = nullptr;
  uint32_t* d_sure = nullptr;      // flags per input position
  uint32_t* d_sure_pre = nullptr;  // P + 1
  uint32_t* d_vcnt = nullptr;      // per ds voxel
  uint32_t* d_first = nullptr;     // V' + 1
  uint32_t* d_nsure = nullptr;     // per root
  size_t pts_cap = 0;
  int* d_offsets = nullptr;
  uint32_t* d_small = nullptr;  // [0] P total, [1] any sure, [2] max sure, [3] V total
  uint32_t* h_small = nullptr;  // pinned
  uint32_t P = 0;
  GridParams g{};
};

}  // namespace vr
