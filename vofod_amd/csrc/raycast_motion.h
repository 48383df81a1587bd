// Motion-compensated rays (include/vofod.h, MOTION COMPENSATION, vofod_set_raycast_motion): the raycast role for a scan that carries
// a pose per measurement column.  Pixel i = row * width + col was measured in column m = (col + shift_by_row[row]) mod width (the
// handle keeps the shifts reduced to [0, width)), and with T = col_tfs[m], d = lut_dirs[3i..], o = lut_offs[3i..], every operation
// IEEE float32, rounded once, nothing fused:
//   d'[k] = ((T[k][0]*d[0]) + (T[k][1]*d[1])) + (T[k][2]*d[2])
//   o'[k] = (((T[k][0]*o[0]) + (T[k][1]*o[1])) + (T[k][2]*o[2])) + T[k][3]
// From there on the ray is k_raycast's (kernels_raycast.h) with d', o' in place of the LUT entries: dir = R d', start = (R o') + t
// in the association of kernels_raycast.h:77-78, the gates, the length, the in-limits test of the ray's own start, the DDA.  The
// association is the one of those two lines, so an identity table gives d' == d and o' == o as values (a zero may change sign; the
// walk reads only the magnitude of a zero component and compares it).  The two matrices are never multiplied together; no
// exclude-box rule (the reference casts the airframe's short rays too, length <= 0 stops them).
//
// k_raycast's walk is the body of that kernel, so this one restates it: rcm_setup restates kernels_raycast.h:80-103 (length, first
// voxel, tmax / tdelta / rem / lstep) and rcm_step restates :120-178 (one DDA step and the DPP run merge, RAY_ACC == 0) - token for
// token where the names allow; tests/test_gpu_raycast_motion.py (identity table against k_raycast) holds the two to each other.
// What is new is the front: row = idx / width (one 32-bit division), m with one compare for the wrap, the pose, the two transforms.
//
// Lanes of a wave are 64 consecutive columns of one ring: their 64 poses are 3 KB of consecutive memory except where m wraps or the
// wave spans a row end.  <POSE16>: the table is 16-byte aligned and a pose is three 16-byte loads, otherwise twelve 4-byte loads
// (range_motion.h: rm_load_pose).  One ray per lane, no LDS, no scratch; every lane of every wave stays in the loop (the DPP merge
// and its ballots need the full wave: a lane beyond n or behind a gate is carried as an inactive ray, never returned early).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_raycast.h"
#include "range_motion.h"

namespace vr
{

// d' and o' of the definition above
__device__ __forceinline__ void rcm_pose_apply(const vrm::Pose& T, const float d[3], const float o[3], float dm[3], float om[3])
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

// kernels_raycast.h:80-103 restated: the state of one ray's walk from its world-frame direction and start
__device__ __forceinline__ void rcm_setup(RayWalk& w, bool alive, const float dir[3], const float start[3], uint32_t rng, const RayParams& rp, const MapGeom& mg)
{
  const float ray_dist = __fmul_rn(0.001f, static_cast<float>(rng));                                        // :1455-1456
  w.length = ray_dist == 0.0f ? rp.max_dist : fminf(__fsub_rn(ray_dist, rp.voxel_size), rp.max_dist);       // :1457
  const int cur[3] = {c2i(start[0], mg.off[0], mg.vs_inv), c2i(start[1], mg.off[1], mg.vs_inv), c2i(start[2], mg.off[2], mg.vs_inv)};
  const int lim[3] = {mg.sx, mg.sy, mg.sz};
  if (cur[0] < 0 || cur[0] >= lim[0] || cur[1] < 0 || cur[1] >= lim[1] || cur[2] < 0 || cur[2] >= lim[2])  // :1482
    alive = false;
  // forEachRay voxel_map.cpp:229-263
  const float half = mg.vs / 2.0f;
  const int lstride[3] = {1, mg.sx, mg.sx * mg.sy};
#pragma unroll
  for (int a = 0; a < 3; a++)
  {
    const float absdir = fabsf(dir[a]);
    const int step = (dir[a] > 0.0f) - (dir[a] < 0.0f);
    w.tdelta[a] = __fmul_rn(__fdiv_rn(1.0f, absdir), mg.vs);
    const float ctr = __fadd_rn(__fmul_rn(__fadd_rn(static_cast<float>(cur[a]), 0.5f), mg.vs), mg.off[a]);
    const float ctr_offset = __fsub_rn(ctr, start[a]);
    w.tmax[a] = __fdiv_rn(__fadd_rn(half, __fmul_rn(static_cast<float>(step), ctr_offset)), absdir);
    w.rem[a] = step > 0 ? lim[a] - 1 - cur[a] : cur[a];  // (last[a] = step > 0 ? lim - 1 : 0, :246)
    w.lstep[a] = step * lstride[a];
  }
  w.lin = alive ? static_cast<uint32_t>((static_cast<uint64_t>(cur[2]) * mg.sy + cur[1]) * mg.sx + cur[0]) : 0u;
  w.prev = 0.0f;
  w.active = alive && 0.0f < w.length;
}

// kernels_raycast.h:120-178 restated (RAY_ACC == 0): one DDA step of the lane's ray, then the wave merges the runs of lanes that sit
// in one voxel and the last lane of a run issues the float atomic.  Called by every lane of the wave; returns whether this lane added.
__device__ __forceinline__ bool rcm_step(RayWalk& r, int lane, float* __restrict__ ray)
{
  // the axis of the smallest tmax, first minimum on ties (Eigen's minCoeff, voxel_map.cpp:252)
  const bool s1 = r.tmax[1] < r.tmax[0];
  const float m01 = s1 ? r.tmax[1] : r.tmax[0];
  const bool s2 = r.tmax[2] < m01;
  const float dist = s2 ? r.tmax[2] : m01;
  float dd = __fsub_rn(fminf(dist, r.length), r.prev);
  dd = r.active ? dd : 0.0f;
  const uint32_t key = dd != 0.0f ? r.lin : 0xffffffffu;
  const int remi = s2 ? r.rem[2] : (s1 ? r.rem[1] : r.rem[0]);
  const bool adv = r.active & (remi != 0);
  const bool a2 = adv & s2, a1 = adv & s1 & !s2, a0 = adv & !s1 & !s2;
  r.tmax[0] = a0 ? __fadd_rn(r.tmax[0], r.tdelta[0]) : r.tmax[0];
  r.tmax[1] = a1 ? __fadd_rn(r.tmax[1], r.tdelta[1]) : r.tmax[1];
  r.tmax[2] = a2 ? __fadd_rn(r.tmax[2], r.tdelta[2]) : r.tmax[2];
  r.rem[0] -= a0 ? 1 : 0;
  r.rem[1] -= a1 ? 1 : 0;
  r.rem[2] -= a2 ? 1 : 0;
  r.lin += static_cast<uint32_t>(a0 ? r.lstep[0] : (a1 ? r.lstep[1] : (a2 ? r.lstep[2] : 0)));
  r.prev = r.active ? dist : r.prev;
  r.active = adv & (dist < r.length);
  // Runs of lanes in one voxel: segmented inclusive sum with DPP moves (row_shr 1 / 2 / 4 / 8, row_bcast 15 / 31: vector ALU
  // only, no LDS crossbar).  The last lane of a run holds its total and issues the atomic.
  const uint32_t kprev = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(~key), static_cast<int>(key), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
  const bool head = lane == 0 || kprev != key;
  uint32_t f = head ? 1u : 0u;
  float run = dd;
  auto segstep = [&](auto ctrl_tag, auto mask_tag) {
    constexpr int CTRL = decltype(ctrl_tag)::value, MASK = decltype(mask_tag)::value;
    const float t = __uint_as_float(dpp_mov0<CTRL, MASK>(__float_as_uint(run)));
    const uint32_t ft = dpp_mov0<CTRL, MASK>(f);
    run = f ? run : __fadd_rn(run, t);
    f |= ft;
  };
  segstep(std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
  segstep(std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
  segstep(std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
  segstep(std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
  segstep(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
  segstep(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
  const unsigned long long H = __ballot(head);
  const bool tail = lane == 63 || ((H >> (lane + 1)) & 1ull);
  if (tail && key != 0xffffffffu)
  {
    unsafeAtomicAdd(&ray[key], run);
    return true;
  }
  return false;
}

template <bool POSE16>
__global__ __launch_bounds__(256) void k_raycast_motion(const RayParams rp, const MapGeom mg, const char* __restrict__ intensity, const char* __restrict__ range, uint64_t stride,
                                                        const float* __restrict__ lut_dirs, const float* __restrict__ lut_offs, const uint8_t* __restrict__ mask,
                                                        const float* __restrict__ poses, const uint32_t* __restrict__ shift, uint32_t width, float* __restrict__ ray,
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
  // the pose of the pixel's measurement column, applied to the beam's direction and offset
  const uint32_t row = idx / width;
  const uint32_t m = vrm::rm_column(row, idx - row * width, width, shift);
  const vrm::Pose T = vrm::rm_load_pose<POSE16>(poses, m);
  const float d[3] = {lut_dirs[3 * idx], lut_dirs[3 * idx + 1], lut_dirs[3 * idx + 2]};
  const float o[3] = {lut_offs[3 * idx], lut_offs[3 * idx + 1], lut_offs[3 * idx + 2]};
  float dm[3], om[3];
  rcm_pose_apply(T, d, o, dm, om);
  // the call's tf, as kernels_raycast.h:77-78 with d', o' in place of the LUT entries
  float dir[3], start[3];
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
    const float* R = &rp.R[3 * r];
    dir[r] = __fadd_rn(__fadd_rn(__fmul_rn(R[0], dm[0]), __fmul_rn(R[1], dm[1])), __fmul_rn(R[2], dm[2]));
    start[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[0], om[0]), __fmul_rn(R[1], om[1])), __fmul_rn(R[2], om[2])), rp.origin[r]);
  }
  RayWalk w;
  rcm_setup(w, alive, dir, start, rng, rp, mg);
  // wave-uniform loop, as k_raycast's
  bool any = false;
  while (__ballot(w.active))
    any |= rcm_step(w, lane, ray);
  if (any)
    *any_hit = 1u;
}

}  // namespace vr
