// Motion-compensated range images (include/vofod.h: a range image whose vofod_scan carries col_tfs): the decode of range_decode.h
// followed, per pixel, by the pose of the measurement column the pixel was taken in.  Pixel i = row * width + col was measured in
// column m = (col + shift_by_row[row]) mod width (vofod_set_column_shift; the handle keeps the shifts reduced to [0, width)), and,
// every operation IEEE float32, rounded once, nothing fused:
//   r = float(range[i]) * 0.001f;   q[a] = (lut_dirs[3i+a] * r) + lut_offs[3i+a]
//   p = (+0, +0, +0)                                             when range[i] == 0      (no pose applied)
//   p = (qNaN, qNaN, qNaN)                                       when q lies in the closed exclude box of the first crop: the
//                                                                airframe, seen in the frame of the instant it was measured
//   p[k] = T[k][0]*q[0] + (T[k][1]*q[1] + (T[k][2]*q[2] + T[k][3]))   otherwise, T = col_tfs[m] (PCL's association)
//
//   k_range_decode_motion<true, .>   one launch per batch.  A thread owns 4 consecutive pixels: the LUT entries and the four column
//                                    indices are loaded / computed once, then, for every frame of its chunk of the job list, one
//                                    16-byte load of ranges, the four poses and three 16-byte stores (x, y, z columns).
//   k_range_decode_motion<false, .>  one pixel per thread, 4-byte accesses: the layouts k_range_decode<false> serves.
//   <., true>                        every pose table of the batch is 16-byte aligned: a pose is three 16-byte loads; otherwise
//                                    twelve 4-byte loads.  A table is width * 48 B per frame and read by every row: cache hits.
//
// m is computed per pixel: a quad straddles a row end when width % 4 != 0, and the wrap of m falls anywhere.
// A kernel of its own with a job list of its own: k_range_decode and its launch are what they were for frames without poses.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vrm
{

constexpr int RM_THREADS = 256;
constexpr uint32_t RM_CHUNK_MAX = 8;  // frames per thread, as RD_CHUNK_MAX

struct MotionJob
{
  const char* src;     // uint32 millimetres, pixel i at src + i * stride
  float* dst;          // x column; y at dst + col_pitch, z at dst + 2 * col_pitch (floats)
  uint64_t stride;
  const float* poses;  // width row-major 3x4 matrices
};
static_assert(sizeof(MotionJob) == 32, "MotionJob: four words of 8 bytes");

struct MotionBox  // closed exclude box of the first crop (GridParams::ex_min / ex_max)
{
  float lo[3], hi[3];
};

struct Pose
{
  float4 r0, r1, r2;  // rows of [R|t]
};

template <bool POSE16>
__device__ __forceinline__ Pose rm_load_pose(const float* __restrict__ poses, uint32_t m)
{
  Pose p;
  if constexpr (POSE16)
  {
    const float4* p4 = reinterpret_cast<const float4*>(poses) + 3u * static_cast<size_t>(m);
    p.r0 = p4[0], p.r1 = p4[1], p.r2 = p4[2];
  }
  else
  {
    const float* s = poses + 12u * static_cast<size_t>(m);
    p.r0 = make_float4(s[0], s[1], s[2], s[3]);
    p.r1 = make_float4(s[4], s[5], s[6], s[7]);
    p.r2 = make_float4(s[8], s[9], s[10], s[11]);
  }
  return p;
}

__device__ __forceinline__ float rm_row(const float4 t, float q0, float q1, float q2)
{
  return __fadd_rn(__fmul_rn(t.x, q0), __fadd_rn(__fmul_rn(t.y, q1), __fadd_rn(__fmul_rn(t.z, q2), t.w)));
}

__device__ __forceinline__ void rm_point(uint32_t rng, float dx, float dy, float dz, float ox, float oy, float oz, const Pose& T, const MotionBox& box, float& x, float& y, float& z)
{
  const float r = __fmul_rn(static_cast<float>(rng), 0.001f);
  const float q0 = __fadd_rn(__fmul_rn(dx, r), ox), q1 = __fadd_rn(__fmul_rn(dy, r), oy), q2 = __fadd_rn(__fmul_rn(dz, r), oz);
  const bool inside = q0 >= box.lo[0] && q0 <= box.hi[0] && q1 >= box.lo[1] && q1 <= box.hi[1] && q2 >= box.lo[2] && q2 <= box.hi[2];
  const float nan = __uint_as_float(0x7fc00000u);
  x = rng == 0 ? 0.0f : inside ? nan : rm_row(T.r0, q0, q1, q2);
  y = rng == 0 ? 0.0f : inside ? nan : rm_row(T.r1, q0, q1, q2);
  z = rng == 0 ? 0.0f : inside ? nan : rm_row(T.r2, q0, q1, q2);
}

// measurement column of pixel (row, col): shift[] holds the shifts reduced to [0, width)
__device__ __forceinline__ uint32_t rm_column(uint32_t row, uint32_t col, uint32_t width, const uint32_t* __restrict__ shift)
{
  const uint32_t m = col + shift[row];  // (< 2 * width <= 2^32: width is an int32)
  return m >= width ? m - width : m;
}

template <bool VEC, bool POSE16>
__global__ __launch_bounds__(RM_THREADS) void k_range_decode_motion(const MotionJob* __restrict__ jobs, uint32_t n_jobs, uint32_t chunk, uint32_t n_px, uint32_t width, uint32_t col_pitch,
                                                                    const float* __restrict__ lut_dirs, const float* __restrict__ lut_offs, const uint32_t* __restrict__ shift,
                                                                    const MotionBox box)
{
  const uint32_t t = blockIdx.x * RM_THREADS + threadIdx.x;
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
    uint32_t m[4];
    {
      uint32_t row = (4u * t) / width, col = 4u * t - row * width;
#pragma unroll
      for (int k = 0; k < 4; k++)
      {
        while (col >= width)  // (a quad may straddle a row end; more than once only where width < 4)
          col -= width, row++;
        m[k] = rm_column(row, col, width, shift);
        col++;
      }
    }
#pragma unroll 2
    for (uint32_t j = j0; j < j1; j++)
    {
      const MotionJob job = jobs[j];
      const uint4 rg = reinterpret_cast<const uint4*>(job.src)[t];
      float4 x, y, z;
      rm_point(rg.x, da.x, da.y, da.z, oa.x, oa.y, oa.z, rm_load_pose<POSE16>(job.poses, m[0]), box, x.x, y.x, z.x);
      rm_point(rg.y, da.w, db.x, db.y, oa.w, ob.x, ob.y, rm_load_pose<POSE16>(job.poses, m[1]), box, x.y, y.y, z.y);
      rm_point(rg.z, db.z, db.w, dc.x, ob.z, ob.w, oc.x, rm_load_pose<POSE16>(job.poses, m[2]), box, x.z, y.z, z.z);
      rm_point(rg.w, dc.y, dc.z, dc.w, oc.y, oc.z, oc.w, rm_load_pose<POSE16>(job.poses, m[3]), box, x.w, y.w, z.w);
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
    const uint32_t row = t / width;
    const uint32_t m = rm_column(row, t - row * width, width, shift);
    for (uint32_t j = j0; j < j1; j++)
    {
      const MotionJob job = jobs[j];
      const uint32_t rng = *reinterpret_cast<const uint32_t*>(job.src + static_cast<uint64_t>(t) * job.stride);
      float x, y, z;
      rm_point(rng, dx, dy, dz, ox, oy, oz, rm_load_pose<POSE16>(job.poses, m), box, x, y, z);
      job.dst[t] = x;
      job.dst[col_pitch + static_cast<size_t>(t)] = y;
      job.dst[2u * static_cast<size_t>(col_pitch) + t] = z;
    }
  }
}

}  // namespace vrm
