// The per-column sensor model of a motion-compensated scan (include/vofod.h: vofod_scan::col_tfs, vofod_set_column_shift), shared by the
// range-image decode (range_decode.h), the point-scan compensation (point_deskew.h) and the raycast role (kernels_raycast.h).  Pixel
// i = row * width + col was measured in column m = (col + shift_by_row[row]) mod width (the handle keeps the shifts reduced to
// [0, width)); its pose is T = col_tfs[m], a row-major 3x4 matrix.  A table is width * 48 B per frame and read by every row: cache hits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vk
{

struct Pose
{
  float4 r0, r1, r2;  // rows of [R|t]
};

// 16-byte load through the global address space (the column pointers come out of a struct in memory: the compiler would
// otherwise emit flat loads, which also probe the LDS aperture)
__device__ __forceinline__ float4 ldg_f4(const char* p)
{
  typedef float gf4 __attribute__((ext_vector_type(4)));
  const gf4 v = *reinterpret_cast<const __attribute__((address_space(1))) gf4*>(reinterpret_cast<uintptr_t>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

// ... and the 4-byte load
__device__ __forceinline__ float ldg_f32(const char* p) { return *reinterpret_cast<const __attribute__((address_space(1))) float*>(reinterpret_cast<uintptr_t>(p)); }

// POSE16: the table is 16-byte aligned and a pose is three 16-byte loads; otherwise twelve 4-byte loads
template <bool POSE16>
__device__ __forceinline__ Pose load_pose(const float* __restrict__ poses, uint32_t m)
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

// measurement column of pixel (row, col): shift[] holds the shifts reduced to [0, width)
__device__ __forceinline__ uint32_t measurement_column(uint32_t row, uint32_t col, uint32_t width, const uint32_t* __restrict__ shift)
{
  const uint32_t m = col + shift[row];  // (< 2 * width <= 2^32: width is an int32)
  return m >= width ? m - width : m;
}

}  // namespace vk
