// Exact raycast accumulation (include/vofod.h, EXACT RAYCAST ACCUMULATION, vofod_set_raycast_exact): the raycast role with path
// lengths summed as fixed-point units in uint32 instead of float atomics.  With S = log2(units per metre) and QMAX of the handle
// (ray_exact_scale below), a piece dd - the float min(dist, length) - prev of k_raycast, unchanged - counts
//   q = min(rint(dd * 2^S), QMAX)          (the product is exact, rint is to nearest even; q == 0 leaves no trace)
// and U[v] = sum of q over the pieces laid into voxel v, in the raycast map's own buffer.  Integer addition is associative and
// n_pixels * QMAX fits in 32 bits, so U does not depend on the order of the atomics nor on how the wave groups its lanes into runs:
// two passes of one scan, and the passes of two handles, end with the same bits.  The float view of a voxel is r = float(U) * 2^-S
// (the conversion rounds to nearest even, the scaling is exact); the sweep, the old rule's max_val and vofod_read_map read that r.
//
// k_raycast_exact<MOTION, ALIGNED16>: one walk body behind two fronts - the rigid one of k_raycast (kernels_raycast.h:65-103) and the
// pose-per-column one of k_raycast_motion (raycast_motion.h).  Set-up and DDA step are k_raycast's expressions (kernels_raycast.h:80-103
// and :120-178), written out in the kernel on scalar locals; new in the step: the piece is quantised per lane BEFORE the run merge,
// the DPP segmented sum adds uint32 (64 lanes * QMAX < 2^32), and the run's last lane issues one relaxed agent-scope integer atomic
// whose result nobody reads.  One ray per lane; every lane of every wave stays in the loop (the DPP merge and its ballots need the
// full wave).  No LDS and no scratch - checked in the ISA: group segment 0, no ds_ instruction (k_raycast and k_raycast_motion keep
// their walk state in a RayWalk behind a reference, which the compiler parks in 16 KB of LDS per block; see the kernel).
// k_ray_sweep_exact: k_ray_sweep (kernels_raycast.h) reading U, forming r as defined, clearing to zero bits.  An all-zero map is the
// same map in both representations, so the driver's ray_dirty / fill_map bookkeeping is shared with the float pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels_raycast.h"
#include "raycast_motion.h"

namespace vr
{

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

// one step of the segmented inclusive sum: lanes whose flag is clear add the value CTRL brings, flags are or-ed
template <int CTRL, int MASK>
__device__ __forceinline__ void rx_segstep(uint32_t& run, uint32_t& f)
{
  const uint32_t t = dpp_mov0<CTRL, MASK>(run);
  const uint32_t ft = dpp_mov0<CTRL, MASK>(f);
  run = f ? run : run + t;
  f |= ft;
}

// one axis of forEachRay's set-up (voxel_map.cpp:229-263), kernels_raycast.h:92-99
__device__ __forceinline__ void rx_axis(float dir, float start, int cur, int lim, int lstride, float vs, float off, float half, float& tmax, float& tdelta, int& rem, int& lstep)
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

// MOTION: the front of k_raycast_motion (poses, shift and width are read), otherwise the front of k_raycast (they are not: nullptr, 0).
// ALIGNED16: the pose table is 16-byte aligned (rm_load_pose); without MOTION the driver instantiates <false, true> only.
template <bool MOTION, bool ALIGNED16>
__global__ __launch_bounds__(256) void k_raycast_exact(const RayParams rp, const MapGeom mg, const ExactScale xs, const char* __restrict__ intensity, const char* __restrict__ range,
                                                       uint64_t stride, const float* __restrict__ lut_dirs, const float* __restrict__ lut_offs, const uint8_t* __restrict__ mask,
                                                       const float* __restrict__ poses, const uint32_t* __restrict__ shift, uint32_t width, uint32_t* __restrict__ units,
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
    const uint32_t m = vrm::rm_column(row, idx - row * width, width, shift);
    const vrm::Pose T = vrm::rm_load_pose<ALIGNED16>(poses, m);
    const float d[3] = {dm[0], dm[1], dm[2]}, o[3] = {om[0], om[1], om[2]};
    rcm_pose_apply(T, d, o, dm, om);
  }
  // the call's tf, kernels_raycast.h:77-78
  float dir[3], start[3];
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
    const float* R = &rp.R[3 * r];
    dir[r] = __fadd_rn(__fadd_rn(__fmul_rn(R[0], dm[0]), __fmul_rn(R[1], dm[1])), __fmul_rn(R[2], dm[2]));
    start[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[0], om[0]), __fmul_rn(R[1], om[1])), __fmul_rn(R[2], om[2])), rp.origin[r]);
  }
  // The walk state lives in scalar locals of the kernel, and the step below is written out here and not in a function on a RayWalk&:
  // behind a reference the compiler folds `s2 ? rem[2] : (s1 ? rem[1] : rem[0])` into one load through a selected ADDRESS, cannot
  // split the struct into registers any more and parks it in LDS (64 B per lane, read and written every step - k_raycast and
  // k_raycast_motion carry that: 16 384 B of LDS per block in their resource remarks).  Here everything stays in VGPRs: no LDS.
  // kernels_raycast.h:80-103, the same expressions one axis at a time (rx_axis)
  const float ray_dist = __fmul_rn(0.001f, static_cast<float>(rng));                                             // :1455-1456
  const float length = ray_dist == 0.0f ? rp.max_dist : fminf(__fsub_rn(ray_dist, rp.voxel_size), rp.max_dist);  // :1457
  const int c0 = c2i(start[0], mg.off[0], mg.vs_inv), c1 = c2i(start[1], mg.off[1], mg.vs_inv), c2 = c2i(start[2], mg.off[2], mg.vs_inv);
  if (c0 < 0 || c0 >= mg.sx || c1 < 0 || c1 >= mg.sy || c2 < 0 || c2 >= mg.sz)  // :1482
    alive = false;
  const float half = mg.vs / 2.0f;
  float tmax0, tmax1, tmax2, tdelta0, tdelta1, tdelta2;
  int rem0, rem1, rem2, lstep0, lstep1, lstep2;
  rx_axis(dir[0], start[0], c0, mg.sx, 1, mg.vs, mg.off[0], half, tmax0, tdelta0, rem0, lstep0);
  rx_axis(dir[1], start[1], c1, mg.sy, mg.sx, mg.vs, mg.off[1], half, tmax1, tdelta1, rem1, lstep1);
  rx_axis(dir[2], start[2], c2, mg.sz, mg.sx * mg.sy, mg.vs, mg.off[2], half, tmax2, tdelta2, rem2, lstep2);
  uint32_t lin = alive ? static_cast<uint32_t>((static_cast<uint64_t>(c2) * mg.sy + c1) * mg.sx + c0) : 0u;
  float prev = 0.0f;
  bool active = alive && 0.0f < length;
  // wave-uniform loop, as k_raycast's; the step is kernels_raycast.h:120-178 with the accumulation of this file
  bool any = false;
  while (__ballot(active))
  {
    // the axis of the smallest tmax, first minimum on ties (Eigen's minCoeff, voxel_map.cpp:252)
    const bool s1 = tmax1 < tmax0;
    const float m01 = s1 ? tmax1 : tmax0;
    const bool s2 = tmax2 < m01;
    const float dist = s2 ? tmax2 : m01;
    const float dd = __fsub_rn(fminf(dist, length), prev);
    const uint32_t q = active ? rx_units(dd, xs) : 0u;  // quantised per lane, BEFORE the run merge
    const uint32_t key = q != 0u ? lin : 0xffffffffu;
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
    // Runs of lanes in one voxel: segmented inclusive sum with DPP moves (row_shr 1 / 2 / 4 / 8, row_bcast 15 / 31: vector ALU
    // only, no LDS crossbar), on uint32: 64 lanes * QMAX fits.  The last lane of a run holds its total and issues the atomic.
    const uint32_t kprev = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(~key), static_cast<int>(key), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
    const bool head = lane == 0 || kprev != key;
    uint32_t f = head ? 1u : 0u;
    uint32_t run = q;
    rx_segstep<0x111, 0xf>(run, f);
    rx_segstep<0x112, 0xf>(run, f);
    rx_segstep<0x114, 0xf>(run, f);
    rx_segstep<0x118, 0xf>(run, f);
    rx_segstep<0x142, 0xa>(run, f);
    rx_segstep<0x143, 0xc>(run, f);
    const unsigned long long H = __ballot(head);
    const bool tail = lane == 63 || ((H >> (lane + 1)) & 1ull);
    if (tail && key != 0xffffffffu)  // (every lane of such a run counts at least one unit: the total is non-zero)
    {
      (void)__hip_atomic_fetch_add(&units[key], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      any = true;
    }
  }
  if (any)
    *any_hit = 1u;
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

// K15 on units: k_ray_sweep (kernels_raycast.h) with r = float(U) * 2^-S; the accumulator is cleared to zero bits
__global__ __launch_bounds__(256) void k_ray_sweep_exact(const SweepParams sp, float inv_scale, uint64_t n, float* __restrict__ map, float* __restrict__ flags,
                                                         uint32_t* __restrict__ units)
{
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
  {
    const float flag = flags[i];
    const uint32_t u = units[i];
    if (flag == 0.0f && u != 0u)
    {
      const float r = __fmul_rn(__uint2float_rn(u), inv_scale);
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
    if (u != 0u)
      units[i] = 0u;
  }
}

}  // namespace vr
