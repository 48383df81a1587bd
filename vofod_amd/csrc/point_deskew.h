// Motion-compensated point scans (include/vofod.h, MOTION COMPENSATION OF POINT SCANS; vofod_set_point_motion, vofod_deskew_points): a
// point scan whose vofod_scan carries col_tfs has the pose of its measurement column applied to every point, in front of the unchanged
// pipeline.  Pixel i = row * width + col was measured in column m = (col + shift_by_row[row]) mod width (column_pose.h), T = col_tfs[m],
// q = (x[i], y[i], z[i]) as given, and, every operation IEEE float32, rounded once, nothing fused, the rules in this order:
//   p = (+0, +0, +0)                                                  when q[0] == 0 && q[1] == 0 && q[2] == 0 (either sign of zero)
//   p = (qNaN, qNaN, qNaN)                                            when any q[a] is not finite
//   p = (qNaN, qNaN, qNaN)                                            when q lies in the closed exclude box of the first crop
//   p[k] = T[k][0]*q[0] + (T[k][1]*q[1] + (T[k][2]*q[2] + T[k][3]))   otherwise (rd_row of range_decode.h: the decode's own association)
//
// ONE kernel template, k_point_deskew_t<VEC, SPAN>, launched once per batch under the profiler name k_point_deskew over the
// job list of the batch's point scans with poses (blockIdx.y = the job).  A job reads x, y, z at a common byte stride - the caller's
// device memory, never written, or the staged copy of a host scan - and writes the packed x | y | z columns of the frame's staging
// slot.  Source and destination may be the same columns (host columns staged into the slot): the kernel is element-wise, a thread
// reads its own pixels before it stores them, and no pointer to the points is __restrict__.
//   <true, .>   a thread owns 4 consecutive pixels, 16-byte loads and stores: stride 4, every base on 16 bytes, w * h % 4 == 0
//   <false, .>  one pixel per thread, 4-byte accesses: every other stride (structs of 12, 16, 48 bytes) and base
// The thread-to-pixel map is chosen for the poses: a wave covers consecutive pixels of the row-major image - 64 (scalar) or 256 (vector)
// consecutive columns of one row, whose poses are as many consecutive table entries (3 KB / 12 KB) up to one wrap of m; a wave that
// straddles a row end reads one such piece per row, and where width is below the wave's span it covers several rows.
//   <., true>   SPAN, every pose table of the batch 16-byte aligned (POSE16 of column_pose.h): every lane computes the measurement
//               columns of its own pixels and leaves them in LDS; the wave then fetches the poses of its pixels into LDS with
//               lane-consecutive 16-byte loads - element e of the span (pixel e / 3, row e % 3 of its pose) by lane e % 64, so that
//               consecutive lanes read consecutive 16 bytes wherever m runs on, whatever the width, twelve (three) independent
//               loads per lane in flight - and every lane takes the poses of its own pixels from LDS.
//   <., false>  a table off 16 bytes: every lane loads the poses of its pixels from the table with 4-byte loads (load_pose<false>).
// Measured (profiles/r21_point_motion.txt): the span form against the same lane-by-lane loads on aligned tables (three 16-byte loads
// per pose, 192 B from the neighbour lane's) 0.198 against 0.370 ms per batch of 256 OS1-128 frames; the latter form was dropped.
// No whole-table LDS scheme (the width may be 2 048), no atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "column_pose.h"
#include "range_decode.h"

namespace vpd
{
using vk::Pose;
using vrd::MotionArgs;

constexpr int PD_THREADS = 256;
constexpr int PD_WAVES = PD_THREADS / 64;

struct PointJob
{
  const char *x, *y, *z;  // float, pixel i at + i * stride
  float* dst;             // x column; y at dst + col_pitch, z at dst + 2 * col_pitch (floats)
  uint64_t stride;
  const float* poses;  // width row-major 3x4 matrices
};
static_assert(sizeof(PointJob) == 48, "PointJob: six words of 8 bytes");

// measurement column of pixel p0 + k, (row0, col0) being pixel p0 (a few steps where width is below the wave's span, one at most otherwise)
__device__ __forceinline__ uint32_t pd_column(uint32_t row0, uint32_t col0, uint32_t k, const MotionArgs& ma)
{
  uint32_t row = row0, col = col0 + k;
  while (col >= ma.width)
    col -= ma.width, row++;
  return vk::measurement_column(row, col, ma.width, ma.shift);
}

// one point: the rules of the definition in their order (the pose part is computed for every pixel and selected where the last rule
// applies: no branch for the loads of T to hide behind)
__device__ __forceinline__ void pd_point(float q0, float q1, float q2, const Pose& T, const MotionArgs& ma, float& x, float& y, float& z)
{
  const bool zero = q0 == 0.0f && q1 == 0.0f && q2 == 0.0f;
  const float inf = __uint_as_float(0x7f800000u), nan = __uint_as_float(0x7fc00000u);
  const bool finite = fabsf(q0) < inf && fabsf(q1) < inf && fabsf(q2) < inf;  // (false for a NaN)
  const bool inside = q0 >= ma.lo[0] && q0 <= ma.hi[0] && q1 >= ma.lo[1] && q1 <= ma.hi[1] && q2 >= ma.lo[2] && q2 <= ma.hi[2];
  const bool drop = !finite || inside;
  const float p0 = vrd::rd_row(T.r0, q0, q1, q2), p1 = vrd::rd_row(T.r1, q0, q1, q2), p2 = vrd::rd_row(T.r2, q0, q1, q2);
  x = zero ? 0.0f : drop ? nan : p0;
  y = zero ? 0.0f : drop ? nan : p1;
  z = zero ? 0.0f : drop ? nan : p2;
}

template <bool VEC, bool SPAN>
__global__ __launch_bounds__(PD_THREADS) void k_point_deskew_t(const PointJob* __restrict__ jobs, uint32_t n_px, uint32_t col_pitch, const MotionArgs ma)
{
  constexpr uint32_t PPT = VEC ? 4u : 1u, WPX = 64u * PPT;  // pixels per thread and per wave
  __shared__ float4 span[SPAN ? PD_WAVES * 3u * WPX : 1u];  // per wave: the poses of its pixels, pixel k at [3k, 3k + 3)
  __shared__ uint32_t cols[SPAN ? PD_WAVES * WPX : 1u];     // per wave: the measurement columns of its pixels
  const PointJob job = jobs[blockIdx.y];
  const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
  const uint32_t p0 = (blockIdx.x * PD_WAVES + wave) * WPX;  // the wave's first pixel (the grid's last wave may start beyond n_px)
  const uint32_t row0 = p0 / ma.width, col0 = p0 - row0 * ma.width;
  const uint32_t k0 = lane * PPT, px = p0 + k0;
  const bool live = px < n_px;  // (VEC: n_px is a multiple of 4, a thread's four pixels are inside together)
  // the thread's own pixels: their coordinates (the loads go out first) and their measurement columns
  float qx[PPT] = {}, qy[PPT] = {}, qz[PPT] = {};
  uint32_t m[PPT] = {};
  if (live)
  {
    if constexpr (VEC)
    {
      const size_t at = 4u * static_cast<size_t>(px);
      const float4 a = vk::ldg_f4(job.x + at), b = vk::ldg_f4(job.y + at), c = vk::ldg_f4(job.z + at);
      qx[0] = a.x, qx[1] = a.y, qx[2] = a.z, qx[3] = a.w;
      qy[0] = b.x, qy[1] = b.y, qy[2] = b.z, qy[3] = b.w;
      qz[0] = c.x, qz[1] = c.y, qz[2] = c.z, qz[3] = c.w;
    }
    else
    {
      const uint64_t at = static_cast<uint64_t>(px) * job.stride;
      qx[0] = vk::ldg_f32(job.x + at), qy[0] = vk::ldg_f32(job.y + at), qz[0] = vk::ldg_f32(job.z + at);
    }
#pragma unroll
    for (uint32_t i = 0; i < PPT; i++)
      m[i] = pd_column(row0, col0, k0 + i, ma);
  }
  Pose T[PPT] = {};
  if constexpr (SPAN)
  {
    // the wave's columns go to LDS, so that lane e % 64 can fetch element e of the span - row e % 3 of the pose of pixel e / 3 - and
    // consecutive lanes read consecutive 16 bytes of the table wherever m runs on; the loads of a lane depend on no other load
    uint32_t* wm = cols + wave * WPX;
    float4* w4 = span + wave * 3u * WPX;
    const char* t4 = reinterpret_cast<const char*>(job.poses);
#pragma unroll
    for (uint32_t i = 0; i < PPT; i++)
      wm[k0 + i] = m[i];  // (a pixel beyond the image: column 0, fetched and never used - no branch in the fetch)
    __syncthreads();      // (every thread of the block arrives at both: nobody leaves before the end)
#pragma unroll
    for (uint32_t t = 0; t < 3u * PPT; t++)
    {
      const uint32_t e = lane + 64u * t, k = e / 3u;
      w4[e] = vk::ldg_f4(t4 + 16u * (3u * static_cast<size_t>(wm[k]) + (e - 3u * k)));
    }
    __syncthreads();
    if (live)
#pragma unroll
      for (uint32_t i = 0; i < PPT; i++)
        T[i] = vk::load_pose<true>(reinterpret_cast<const float*>(w4), k0 + i);
  }
  else if (live)
  {
#pragma unroll
    for (uint32_t i = 0; i < PPT; i++)
      T[i] = vk::load_pose<false>(job.poses, m[i]);
  }
  if (!live)
    return;
  float x[PPT], y[PPT], z[PPT];
#pragma unroll
  for (uint32_t i = 0; i < PPT; i++)
    pd_point(qx[i], qy[i], qz[i], T[i], ma, x[i], y[i], z[i]);
  if constexpr (VEC)
  {
    const uint32_t t = px / 4u;
    reinterpret_cast<float4*>(job.dst)[t] = make_float4(x[0], x[1], x[2], x[3]);
    reinterpret_cast<float4*>(job.dst + col_pitch)[t] = make_float4(y[0], y[1], y[2], y[3]);
    reinterpret_cast<float4*>(job.dst + 2u * static_cast<size_t>(col_pitch))[t] = make_float4(z[0], z[1], z[2], z[3]);
  }
  else
  {
    job.dst[px] = x[0];
    job.dst[col_pitch + static_cast<size_t>(px)] = y[0];
    job.dst[2u * static_cast<size_t>(col_pitch) + px] = z[0];
  }
}

}  // namespace vpd
