// Range images (include/vofod.h: a vofod_scan with x == y == z == NULL): the points of a scan rebuilt on the device from the
// sensor's range column and the handle's direction / offset LUT, the model check_sensor_params holds a cloud to
// (vofod_nodelet.cpp:1869-1917).  Per pixel i, every operation IEEE float32, rounded once, nothing fused:
//   r = float(range[i]) * 0.001f;   p[a] = (lut_dirs[3i+a] * r) + lut_offs[3i+a];   p = (+0, +0, +0) when range[i] == 0
//
//   k_range_decode<true>   one launch per batch.  A thread owns 4 consecutive pixels: their interleaved LUT entries are 48
//                          contiguous bytes per table, loaded once with three 16-byte loads each; then, for every frame of its
//                          chunk of the job list, one 16-byte load of ranges and three 16-byte stores (x, y, z columns).  The LUT
//                          (24 B per pixel, 3 MB at OS1-128) is read once per chunk of frames instead of once per frame, and
//                          those re-reads are served by the L2 / Infinity Cache.
//   k_range_decode<false>  the same with one pixel per thread and 4-byte accesses: ranges at a stride other than 4, a base or
//                          a column pitch off 16 bytes, w * h no multiple of 4.
//
// The job list holds the range images of the batch only (a batch may mix them with point scans): source, stride, destination.
// Not part of the frame kernel's sources: the decode writes packed columns, every kernel behind it runs unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vrd
{

constexpr int RD_THREADS = 256;
constexpr uint32_t RD_CHUNK_MAX = 8;  // frames per thread: LUT re-reads are 24 / (16 * 8) = 19 % of the streamed bytes, all cache hits

struct RangeJob
{
  const char* src;  // uint32 millimetres, pixel i at src + i * stride
  float* dst;       // x column; y at dst + col_pitch, z at dst + 2 * col_pitch (floats)
  uint64_t stride;
  uint64_t pad_;
};
static_assert(sizeof(RangeJob) == 32, "RangeJob: four words of 8 bytes");

__device__ __forceinline__ float rd_point(uint32_t rng, float r, float dir, float off) { return rng ? __fadd_rn(__fmul_rn(dir, r), off) : 0.0f; }

template <bool VEC>
__global__ __launch_bounds__(RD_THREADS) void k_range_decode(const RangeJob* __restrict__ jobs, uint32_t n_jobs, uint32_t chunk, uint32_t n_px, uint32_t col_pitch,
                                                             const float* __restrict__ lut_dirs, const float* __restrict__ lut_offs)
{
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
#pragma unroll 4
    for (uint32_t j = j0; j < j1; j++)
    {
      const RangeJob job = jobs[j];
      const uint4 rg = reinterpret_cast<const uint4*>(job.src)[t];
      const float r0 = __fmul_rn(static_cast<float>(rg.x), 0.001f), r1 = __fmul_rn(static_cast<float>(rg.y), 0.001f);
      const float r2 = __fmul_rn(static_cast<float>(rg.z), 0.001f), r3 = __fmul_rn(static_cast<float>(rg.w), 0.001f);
      float4 x, y, z;
      x.x = rd_point(rg.x, r0, da.x, oa.x), y.x = rd_point(rg.x, r0, da.y, oa.y), z.x = rd_point(rg.x, r0, da.z, oa.z);
      x.y = rd_point(rg.y, r1, da.w, oa.w), y.y = rd_point(rg.y, r1, db.x, ob.x), z.y = rd_point(rg.y, r1, db.y, ob.y);
      x.z = rd_point(rg.z, r2, db.z, ob.z), y.z = rd_point(rg.z, r2, db.w, ob.w), z.z = rd_point(rg.z, r2, dc.x, oc.x);
      x.w = rd_point(rg.w, r3, dc.y, oc.y), y.w = rd_point(rg.w, r3, dc.z, oc.z), z.w = rd_point(rg.w, r3, dc.w, oc.w);
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
    for (uint32_t j = j0; j < j1; j++)
    {
      const RangeJob job = jobs[j];
      const uint32_t rng = *reinterpret_cast<const uint32_t*>(job.src + static_cast<uint64_t>(t) * job.stride);
      const float r = __fmul_rn(static_cast<float>(rng), 0.001f);
      job.dst[t] = rd_point(rng, r, dx, ox);
      job.dst[col_pitch + static_cast<size_t>(t)] = rd_point(rng, r, dy, oy);
      job.dst[2u * static_cast<size_t>(col_pitch) + t] = rd_point(rng, r, dz, oz);
    }
  }
}

}  // namespace vrd
