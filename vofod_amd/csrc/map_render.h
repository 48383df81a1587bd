// Map render (include/vofod.h, MAP RENDER; vofod_map_render): the voxel map as the sensor would see it from a pose - the read side
// of the raycast role.  One lane per ray walks the map with the DDA of VoxelMap::forEachRay (voxel_map.cpp:229-263) exactly as
// k_raycast_t does - the front (dir = R d, start = (R o) + t), c2i and ray_axis are those of kernels_raycast.h, included, not
// copied - and stops at the first voxel whose value is above the threshold.  Nothing is written to any map: no atomics, no DPP run
// merge, no LDS, so a lane leaves its loop as soon as its ray is decided (k_raycast_t has to keep the full wave for its ballots).
//
// What is engineered here: the address of the next voxel never depends on a map value, only the exit does.  A loop that loads a
// voxel, tests it and then steps pays one load latency per step (~200 cycles from L2, ~545 from the Infinity Cache, ~900 from HBM;
// a 0.25 m OS1-128 map is 78 MB: beyond any L2, inside the Infinity Cache).  So the walk goes in BURSTS of K steps: the DDA
// advances K times, keeping the K linear indices and the K dist values in registers, the K loads are issued together, and then
// they are tested in walk order - the first hit of the burst wins and the state reported is that step's.  A burst is cut where the
// walk would stop by END (the length ran out inside the voxel) or LEFT (the next step would leave the map): the steps behind the cut
// do not advance, their index is the cut voxel's own, so no index outside the map is ever formed and every load of a burst reads a
// voxel of the map (a cut burst reads its last voxel again: the same cache line).  K is a template parameter.  Measured
// (profiles/r27_map_render.txt; OS1-128 at 0.25 m, one view, 20 m): 43.9 / 39.1 / 36.5 / 33.9 us for K = 1 / 2 / 4 / 8
// beside 223 us of k_raycast on the same scan; 64 views 993 / 960 / 894 / 894 us; OS2-128 x 2048 at 0.1 m 147.1 / 132.1 / 113.7 /
// 104.8 us.  MR_BURST = 8 is kept: the fastest at one view, level with 4 at 64, 62 VGPRs, no scratch, still 8 waves per SIMD.
//
// Walk state in scalar locals, the step written out in the kernel body and every per-step array indexed by unrolled constants: the
// comment above k_raycast_t says what a struct behind a reference cost there (LDS parking); a runtime index would cost scratch here.
// Lanes of a wave are consecutive columns of one ring (pixel = blockIdx.x * 256 + threadIdx.x, view = blockIdx.y): their walks touch
// neighbouring voxels.  The view poses are a small device table of 12 floats per view, read through a wave-uniform address; the
// launch has one kernel argument block whatever n_views is.
//
// Scans against the map (include/vofod.h, SCANS AGAINST THE MAP; vofod_map_render_scans): the same kernel template with the views
// given as SCANS - Views = ScanViews.  Two things vary, as MOTION and Acc vary in k_raycast_t: where the beam comes from (a view whose
// scan carries col_tfs casts every ray from the pose of its measurement column: measurement_column, load_pose and ray_pose_apply of
// column_pose.h / kernels_raycast.h, included, in front of the unchanged rigid front) and what the epilogue does (the verdict of the
// measured range against the piece the walk reports, and the per-view counts of the verdicts).  The per-view data is a device table
// of ViewEntry read through blockIdx.y: the tf, the pose table or null, the range column and its stride.  The walk between the two
// is one text.  The rigid instantiation (Views = RigidViews, the default) keeps its argument block, its early return and its
// registers; with ScanViews a lane beyond n is carried as a dead ray to the end, because the count reduction is a block's work:
// ballots and popcounts per wave and class, 32 bytes of LDS per block, at most seven atomics per block into the view's slots.
// Measured (profiles/r30_map_render_scans.txt; OS1-128 at 0.25 m, a table per view, beside k_map_render of a library
// built from the parent commit): 1 view 33.5 us with tables, 35.8 us with verdict and counts, against 35.3 us; 64 views 906.9 and
// 920.4 against 890.1 us.  58 VGPRs at K = 8, no scratch, 8 waves per SIMD.
//
// Out of scope: reading d_mapbits when the threshold happens to be the occupancy image's; shortening a walk by the measured range.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "column_pose.h"
#include "common.h"
#include "device_mem.h"
#include "kernels_raycast.h"

namespace vmr
{
using namespace vk;

constexpr int MR_THREADS = 256;
constexpr int MR_BURST = 8;             // steps per burst of the production launch (VOFOD_RENDER_BURST=1|2|4|8 selects another: diagnostics, tools/map_render_bench.py)
constexpr uint32_t MR_MAX_VIEWS = 65535;  // gridDim.y

struct RenderParams
{
  float threshold, length;
  uint32_t n;  // pixels per view (w * h)
};

// the caller's four outputs, each nullable, indexed view * n + pixel (t_in_out: two floats per pixel)
struct RenderOut
{
  uint32_t* range;
  uint32_t* voxel;
  uint8_t* what;
  float2* t_in_out;
};

// one view of vofod_map_render_scans: 72 bytes, read through a wave-uniform address
struct ViewEntry
{
  float tf[12];        // the view's row-major [R | t]
  const float* poses;  // the scan's col_tfs on the device (width poses, 4-byte aligned), nullptr: the rigid ray
  const char* range;   // the scan's range column on the device, nullptr when neither verdict nor counts is asked for
  uint64_t stride;     // ... and its stride in bytes
};

// where the views come from.  RigidViews: vofod_map_render's pose table, nothing else.
struct RigidViews
{
  static constexpr bool SCANS = false;
  const float* poses;  // 12 floats per view
  __host__ __device__ RigidViews(const float* p) : poses(p) {}  // (vofod_map_render's launch passes the table itself, as it did)
};
// ScanViews: the view table, the handle's column shifts and mask, and the epilogue's two outputs
struct ScanViews
{
  static constexpr bool SCANS = true;
  const ViewEntry* views;
  const uint32_t* shift;  // one shift per row, reduced to [0, width)
  const uint8_t* mask;
  uint32_t width;
  float tolerance;
  uint8_t* verdict;  // view * n + pixel, nullable
  uint32_t* counts;  // 8 per view, cleared before the launch, nullable
};

// the workspace of the two calls, owned by the handle and grown to the largest seen: the pose table and, for host outputs, the
// staging the kernel writes; for vofod_map_render_scans the view table (h_views: where it is written, d_views: where the kernel
// reads it), the verdicts and the counts.  The host scans' pose tables and range columns are staged by the query calls' one
// ScanStage (scan_stage.h).
struct Workspace
{
  DevBuf<float> d_poses;
  DevBuf<uint32_t> d_range, d_voxel;
  DevBuf<uint8_t> d_what;
  DevBuf<float2> d_tio;
  DevBuf<ViewEntry> d_views;
  DevBuf<uint8_t> d_verdict;
  DevBuf<uint32_t> d_counts;
  std::vector<ViewEntry> h_views;
};

// the sensor's millimetres of the middle of the piece [t_in, t_out], ties to even, never the 0 of "no return"
__device__ __forceinline__ uint32_t render_range_mm(float t_in, float t_out)
{
  const float mm = rintf(__fmul_rn(__fmul_rn(__fadd_rn(t_in, t_out), 0.5f), 1000.0f));
  // (clamped into [0, 2^32 - 256] before the conversion, as rx_units does)
  return max(1u, static_cast<uint32_t>(fminf(fmaxf(mm, 0.0f), 4294967040.0f)));
}

// the verdict of a measured range r (mm, 0: no return) against the render (what, t_in, t_out) of the same pixel: include/vofod.h,
// SCANS AGAINST THE MAP.  Float compares: a NaN makes them false.
__device__ __forceinline__ uint32_t scan_verdict(uint32_t what, float t_in, float t_out, uint32_t r, bool masked_in, float tol)
{
  if (what == 0u)
    return 0u;  // VOFOD_VERDICT_NONE
  if (r == 0u)
    return !masked_in ? 0u : (what == 1u ? 5u /* MISSING */ : 2u /* EMPTY */);
  const float rm = __fmul_rn(static_cast<float>(r), 0.001f);
  const float near = __fadd_rn(rm, tol);
  if (what == 1u)
    return near < t_in ? 3u /* NEARER */ : (rm > __fadd_rn(t_out, tol) ? 4u /* THROUGH */ : 1u /* AGREES */);
  return near < t_out ? 3u /* NEARER */ : 6u /* BEYOND */;
}

template <int K, class Views = RigidViews>
__global__ __launch_bounds__(MR_THREADS) void k_map_render(const RenderParams rp, const MapGeom mg, const float* __restrict__ map, const float* __restrict__ lut_dirs,
                                                          const float* __restrict__ lut_offs, const Views views, const RenderOut out)
{
  constexpr bool SCANS = Views::SCANS;
  const uint32_t idx = blockIdx.x * MR_THREADS + threadIdx.x;
  // a lane beyond n: gone at once from a rigid render; carried to the block's count reduction, casting nothing, with scans
  const bool alive = idx < rp.n;
  if constexpr (!SCANS)
    if (!alive)
      return;
  uint32_t what = 0u /* VOFOD_RENDER_NOT_CAST */, hit_voxel = 0xffffffffu;
  float t_in = 0.0f, t_out = 0.0f;
  if (alive)
  {
    const float* tf;  // wave-uniform: the view's row-major [R | t]
    if constexpr (SCANS)
      tf = views.views[blockIdx.y].tf;
    else
      tf = views.poses + 12u * blockIdx.y;
    float dm[3] = {lut_dirs[3 * idx], lut_dirs[3 * idx + 1], lut_dirs[3 * idx + 2]};
    float om[3] = {lut_offs[3 * idx], lut_offs[3 * idx + 1], lut_offs[3 * idx + 2]};
    if constexpr (SCANS)
    {
      // the pose of the pixel's measurement column, applied to the beam's direction and offset (k_raycast_t's MOTION front)
      const float* poses = views.views[blockIdx.y].poses;
      if (poses)
      {
        const uint32_t row = idx / views.width;
        const uint32_t m = measurement_column(row, idx - row * views.width, views.width, views.shift);
        const Pose T = (reinterpret_cast<uintptr_t>(poses) & 15u) == 0 ? load_pose<true>(poses, m) : load_pose<false>(poses, m);
        const float d[3] = {dm[0], dm[1], dm[2]}, o[3] = {om[0], om[1], om[2]};
        vr::ray_pose_apply(T, d, o, dm, om);
      }
    }
    // the view's tf, in the association of k_raycast_t's front
    float dir[3], start[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
    {
      const float* R = tf + 4 * r;
      dir[r] = __fadd_rn(__fadd_rn(__fmul_rn(R[0], dm[0]), __fmul_rn(R[1], dm[1])), __fmul_rn(R[2], dm[2]));
      start[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[0], om[0]), __fmul_rn(R[1], om[1])), __fmul_rn(R[2], om[2])), R[3]);
    }
    const float length = rp.length;
    const int c0 = vr::c2i(start[0], mg.off[0], mg.vs_inv), c1 = vr::c2i(start[1], mg.off[1], mg.vs_inv), c2 = vr::c2i(start[2], mg.off[2], mg.vs_inv);
    if (c0 >= 0 && c0 < mg.sx && c1 >= 0 && c1 < mg.sy && c2 >= 0 && c2 < mg.sz)
    {
      const float half = mg.vs / 2.0f;
      float tmax0, tmax1, tmax2, tdelta0, tdelta1, tdelta2;
      int rem0, rem1, rem2, lstep0, lstep1, lstep2;
      vr::ray_axis(dir[0], start[0], c0, mg.sx, 1, mg.vs, mg.off[0], half, tmax0, tdelta0, rem0, lstep0);
      vr::ray_axis(dir[1], start[1], c1, mg.sy, mg.sx, mg.vs, mg.off[1], half, tmax1, tdelta1, rem1, lstep1);
      vr::ray_axis(dir[2], start[2], c2, mg.sz, mg.sx * mg.sy, mg.vs, mg.off[2], half, tmax2, tdelta2, rem2, lstep2);
      uint32_t lin = static_cast<uint32_t>((static_cast<uint64_t>(c2) * mg.sy + c1) * mg.sx + c0);
      float prev = 0.0f;
      while (what == 0u)
      {
        // ---- the burst: K steps of the DDA, nothing read.  A step is live while the walk goes on; the step that ends the walk
        // (END or LEFT) is the last live one, the steps behind it stay where it stood.
        uint32_t at[K];
        float dist_at[K];
        const float prev_at0 = prev;
        int n_live = 0;
        uint32_t stop = 0u;       // how the last live step ends the walk, 0 while it goes on
        float stop_prev = 0.0f, stop_dist = 0.0f;  // prev and dist of the last live step
        bool live = true;
#pragma unroll
        for (int k = 0; k < K; k++)
        {
          // the axis of the smallest tmax, first minimum on ties (Eigen's minCoeff, voxel_map.cpp:252)
          const bool s1 = tmax1 < tmax0;
          const float m01 = s1 ? tmax1 : tmax0;
          const bool s2 = tmax2 < m01;
          const float dist = s2 ? tmax2 : m01;
          const int remi = s2 ? rem2 : (s1 ? rem1 : rem0);
          at[k] = lin;
          dist_at[k] = dist;
          const uint32_t ends = !(dist < length) ? 2u /* END */ : (remi == 0 ? 3u /* LEFT */ : 0u);
          stop = live ? ends : stop;
          stop_prev = live ? prev : stop_prev;
          stop_dist = live ? dist : stop_dist;
          n_live += live ? 1 : 0;
          const bool adv = live & (ends == 0u);
          const bool a2 = adv & s2, a1 = adv & s1 & !s2, a0 = adv & !s1 & !s2;
          tmax0 = a0 ? __fadd_rn(tmax0, tdelta0) : tmax0;
          tmax1 = a1 ? __fadd_rn(tmax1, tdelta1) : tmax1;
          tmax2 = a2 ? __fadd_rn(tmax2, tdelta2) : tmax2;
          rem0 -= a0 ? 1 : 0;
          rem1 -= a1 ? 1 : 0;
          rem2 -= a2 ? 1 : 0;
          lin += static_cast<uint32_t>(a0 ? lstep0 : (a1 ? lstep1 : (a2 ? lstep2 : 0)));
          prev = adv ? dist : prev;
          live = adv;
        }
        // ---- the K loads, together (every index is a voxel of the map)
        float m[K];
#pragma unroll
        for (int k = 0; k < K; k++)
          m[k] = map[at[k]];
        // ---- the tests, in walk order: the first hit wins (a NaN is never above the threshold, +inf is, an equal value is not)
#pragma unroll
        for (int k = 0; k < K; k++)
          if (what == 0u && k < n_live && m[k] > rp.threshold)
          {
            what = 1u;  // VOFOD_RENDER_HIT
            hit_voxel = at[k];
            t_in = k == 0 ? prev_at0 : dist_at[k > 0 ? k - 1 : 0];  // (inside a burst, a step's prev is the dist of the step before)
            t_out = fminf(dist_at[k], length);
          }
        if (what == 0u && stop != 0u)
        {
          what = stop;  // the last voxel looked at
          t_in = stop_prev;
          t_out = fminf(stop_dist, length);
        }
      }
    }
  }
  const uint64_t o = static_cast<uint64_t>(blockIdx.y) * rp.n + idx;
  if (alive)
  {
    if (out.range)
      out.range[o] = what == 1u ? render_range_mm(t_in, t_out) : 0u;
    if (out.voxel)
      out.voxel[o] = hit_voxel;
    if (out.what)
      out.what[o] = static_cast<uint8_t>(what);
    if (out.t_in_out)
      out.t_in_out[o] = make_float2(t_in, t_out);
  }
  if constexpr (SCANS)
  {
    const char* range = views.views[blockIdx.y].range;  // (block-uniform; null when neither verdict nor counts is asked for)
    if (!range)
      return;
    uint32_t verdict = 0u;
    if (alive)
    {
      const uint32_t r = *reinterpret_cast<const uint32_t*>(range + static_cast<uint64_t>(idx) * views.views[blockIdx.y].stride);
      const bool masked_in = r != 0u || views.mask[idx] != 0;  // (the mask matters to a pixel without a return only)
      verdict = scan_verdict(what, t_in, t_out, r, masked_in, views.tolerance);
      if (views.verdict)
        views.verdict[o] = static_cast<uint8_t>(verdict);
    }
    if (views.counts)  // (a kernel argument: the whole block goes one way)
    {
      // every lane of the block is here, the dead ones of the tail too: they count nothing, not NONE
      __shared__ uint32_t s_count[8];
      if (threadIdx.x < 8)
        s_count[threadIdx.x] = 0u;
      __syncthreads();
#pragma unroll
      for (uint32_t c = 0; c < 7; c++)
      {
        const uint32_t k = static_cast<uint32_t>(__popcll(__ballot(alive && verdict == c)));
        if ((threadIdx.x & 63) == 0 && k)
          atomicAdd(&s_count[c], k);
      }
      __syncthreads();
      if (threadIdx.x < 7 && s_count[threadIdx.x])
        atomicAdd(&views.counts[8u * blockIdx.y + threadIdx.x], s_count[threadIdx.x]);
    }
  }
}

}  // namespace vmr
