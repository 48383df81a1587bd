// Range images (include/vofod.h: a vofod_scan with x == y == z == NULL): the points of a scan rebuilt on the device from the
// sensor's range column and the handle's direction / offset LUT, the model check_sensor_params holds a cloud to
// (vofod_nodelet.cpp:1869-1917).  Per pixel i, every operation IEEE float32, rounded once, nothing fused:
//   r = float(range[i]) * 0.001f;   p[a] = (lut_dirs[3i+a] * r) + lut_offs[3i+a];   p = (+0, +0, +0) when range[i] == 0
//
// Motion-compensated range images (a range image whose vofod_scan carries col_tfs; MOTION): the decode above followed, per pixel, by
// the pose of the measurement column the pixel was taken in.  Pixel i = row * width + col was measured in column
// m = (col + shift_by_row[row]) mod width (vofod_set_column_shift; the handle keeps the shifts reduced to [0, width)), and,
// every operation IEEE float32, rounded once, nothing fused:
//   r = float(range[i]) * 0.001f;   q[a] = (lut_dirs[3i+a] * r) + lut_offs[3i+a]
//   p = (+0, +0, +0)                                             when range[i] == 0      (no pose applied)
//   p = (qNaN, qNaN, qNaN)                                       when q lies in the closed exclude box of the first crop: the
//                                                                airframe, seen in the frame of the instant it was measured
//   p[k] = T[k][0]*q[0] + (T[k][1]*q[1] + (T[k][2]*q[2] + T[k][3]))   otherwise, T = col_tfs[m] (PCL's association)
//
// ONE kernel template, k_range_decode_t<VEC, MOTION, POSE16>: one thread-to-pixel map, one LUT load, one job loop, one per-pixel
// function (rd_point) that computes r and q once and applies the pose part under MOTION.  The driver launches six instantiations
// under two profiler names, one launch each per batch: k_range_decode (<., false, true>) over the batch's range images without
// poses, k_range_decode_motion (<., true, .>) over those with.
//   <true, ., .>    A thread owns 4 consecutive pixels: their interleaved LUT entries are 48 contiguous bytes per table, loaded once
//                   with three 16-byte loads each (MOTION: and the four column indices computed once); then, for every frame of
//                   its chunk of the job list, one 16-byte load of ranges (MOTION: the four poses) and three 16-byte stores (x, y,
//                   z columns).  The LUT (24 B per pixel, 3 MB at OS1-128) is read once per chunk of frames instead of once per
//                   frame, and those re-reads are served by the L2 / Infinity Cache.
//   <false, ., .>   the same with one pixel per thread and 4-byte accesses: ranges at a stride other than 4, a base or a column
//                   pitch off 16 bytes, w * h no multiple of 4.
//   <., true, true> every pose table of the batch is 16-byte aligned: a pose is three 16-byte loads; otherwise twelve 4-byte loads
//                   (column_pose.h).  The plain instantiations read no pose and fix POSE16 to true.
//
// m is computed per pixel: a quad straddles a row end when width % 4 != 0, and the wrap of m falls anywhere.
// The job list holds the range images of the batch only (a batch may mix them with point scans): source, stride, destination and
// the pose table (nullptr: none) - the jobs with a table first, each kind in frame order, one launch over each span.
// Not part of the frame kernel's sources: the decode writes packed columns, every kernel behind it runs unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "column_pose.h"

namespace vrd
{
using vk::Pose;

constexpr int RD_THREADS = 256;
constexpr uint32_t RD_CHUNK_MAX = 8;  // frames per thread: LUT re-reads are 24 / (16 * 8) = 19 % of the streamed bytes, all cache hits

struct RangeJob
{
  const char* src;     // uint32 millimetres, pixel i at src + i * stride
  float* dst;          // x column; y at dst + col_pitch, z at dst + 2 * col_pitch (floats)
  uint64_t stride;
  const float* poses;  // width row-major 3x4 matrices; nullptr: a range image without poses
};
static_assert(sizeof(RangeJob) == 32, "RangeJob: four words of 8 bytes");

struct MotionArgs  // what only the MOTION instantiations read
{
  const uint32_t* shift;  // the reduced shift of every row
  uint32_t width;
  float lo[3], hi[3];  // closed exclude box of the first crop (GridParams::ex_min / ex_max)
};

__device__ __forceinline__ float rd_row(const float4 t, float q0, float q1, float q2)
{
  return __fadd_rn(__fmul_rn(t.x, q0), __fadd_rn(__fmul_rn(t.y, q1), __fadd_rn(__fmul_rn(t.z, q2), t.w)));
}

// one pixel: range, its LUT entries and (MOTION) column m of the job's pose table to the point
template <bool MOTION, bool POSE16>
__device__ __forceinline__ void rd_point(uint32_t rng, float dx, float dy, float dz, float ox, float oy, float oz, const float* __restrict__ poses, uint32_t m, const MotionArgs& ma, float& x,
                                         float& y, float& z)
{
  const float r = __fmul_rn(static_cast<float>(rng), 0.001f);
  const float q0 = __fadd_rn(__fmul_rn(dx, r), ox), q1 = __fadd_rn(__fmul_rn(dy, r), oy), q2 = __fadd_rn(__fmul_rn(dz, r), oz);
  if constexpr (MOTION)
  {
    const Pose T = vk::load_pose<POSE16>(poses, m);
    const bool inside = q0 >= ma.lo[0] && q0 <= ma.hi[0] && q1 >= ma.lo[1] && q1 <= ma.hi[1] && q2 >= ma.lo[2] && q2 <= ma.hi[2];
    const float nan = __uint_as_float(0x7fc00000u);
    x = rng == 0 ? 0.0f : inside ? nan : rd_row(T.r0, q0, q1, q2);
    y = rng == 0 ? 0.0f : inside ? nan : rd_row(T.r1, q0, q1, q2);
    z = rng == 0 ? 0.0f : inside ? nan : rd_row(T.r2, q0, q1, q2);
  }
  else
    x = rng ? q0 : 0.0f, y = rng ? q1 : 0.0f, z = rng ? q2 : 0.0f;
}

template <bool VEC, bool MOTION, bool POSE16>
__global__ __launch_bounds__(RD_THREADS) void k_range_decode_t(const RangeJob* __restrict__ jobs, uint32_t n_jobs, uint32_t chunk, uint32_t n_px, uint32_t col_pitch,
                                                               const float* __restrict__ lut_dirs, const float* __restrict__ lut_offs, const MotionArgs ma)
{
  constexpr int UNROLL = MOTION ? 2 : 4;
  const uint32_t t = blockIdx.x * RD_THREADS + threadIdx.x;
  const uint32_t j0 = blockIdx.y * chunk, j1 = min(j0 + chunk, n_jobs);
  if constexpr (VEC)
  {
    if (t >= n_px / 4u)  // (n_px is a multiple of 4 here)
      return;
    const float4* d4 = reinterpret_cast<const float4*>(lut_dirs) + 3u * static_cast<size_t>(t);
    const float4* o4 = reinterpret_cast<const float4*>(lut_offs) + 3u * static_cast<size_t>(t);
    // pixels 4t..4t+3: (x0 y0 z0 x1) (y1 z1 x2 y2) (z2 x3 y3 z3)
    const float4 da = d4[0], db = d4[1], dc = d4[2];
    const float4 oa = o4[0], ob = o4[1], oc = o4[2];
    uint32_t m[4] = {};
    if constexpr (MOTION)
    {
      uint32_t row = (4u * t) / ma.width, col = 4u * t - row * ma.width;
#pragma unroll
      for (int k = 0; k < 4; k++)
      {
        while (col >= ma.width)  // (a quad may straddle a row end; more than once only where width < 4)
          col -= ma.width, row++;
        m[k] = vk::measurement_column(row, col, ma.width, ma.shift);
        col++;
      }
    }
#pragma unroll UNROLL
    for (uint32_t j = j0; j < j1; j++)
    {
      const RangeJob job = jobs[j];
      const uint4 rg = reinterpret_cast<const uint4*>(job.src)[t];
      float4 x, y, z;
      rd_point<MOTION, POSE16>(rg.x, da.x, da.y, da.z, oa.x, oa.y, oa.z, job.poses, m[0], ma, x.x, y.x, z.x);
      rd_point<MOTION, POSE16>(rg.y, da.w, db.x, db.y, oa.w, ob.x, ob.y, job.poses, m[1], ma, x.y, y.y, z.y);
      rd_point<MOTION, POSE16>(rg.z, db.z, db.w, dc.x, ob.z, ob.w, oc.x, job.poses, m[2], ma, x.z, y.z, z.z);
      rd_point<MOTION, POSE16>(rg.w, dc.y, dc.z, dc.w, oc.y, oc.z, oc.w, job.poses, m[3], ma, x.w, y.w, z.w);
      reinterpret_cast<float4*>(job.dst)[t] = x;
      reinterpret_cast<float4*>(job.dst + col_pitch)[t] = y;
      reinterpret_cast<float4*>(job.dst + 2u * static_cast<size_t>(col_pitch))[t] = z;
    }
  }
  else
  {
    if (t >= n_px)
      return;
    const float dx = lut_dirs[3u * static_cast<size_t>(t)], dy = lut_dirs[3u * static_cast<size_t>(t) + 1], dz = lut_dirs[3u * static_cast<size_t>(t) + 2];
    const float ox = lut_offs[3u * static_cast<size_t>(t)], oy = lut_offs[3u * static_cast<size_t>(t) + 1], oz = lut_offs[3u * static_cast<size_t>(t) + 2];
    uint32_t m = 0;
    if constexpr (MOTION)
    {
      const uint32_t row = t / ma.width;
      m = vk::measurement_column(row, t - row * ma.width, ma.width, ma.shift);
    }
    for (uint32_t j = j0; j < j1; j++)
    {
      const RangeJob job = jobs[j];
      const uint32_t rng = *reinterpret_cast<const uint32_t*>(job.src + static_cast<uint64_t>(t) * job.stride);
      float x, y, z;
      rd_point<MOTION, POSE16>(rng, dx, dy, dz, ox, oy, oz, job.poses, m, ma, x, y, z);
      job.dst[t] = x;
      job.dst[col_pitch + static_cast<size_t>(t)] = y;
      job.dst[2u * static_cast<size_t>(col_pitch) + t] = z;
    }
  }
}

}  // namespace vrd
