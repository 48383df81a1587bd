// Map distance (include/vofod.h, MAP DISTANCE; vofod_map_distance, vofod_map_match_field): the squared Euclidean distance, in
// voxels, from every voxel to the nearest occupied one, clamped at R * R - and candidate poses scored by it.  The values are
// integers: every result below is exact, whatever the order it was computed in.
//
// The transform is separable: min over u of (dx^2 + dy^2 + dz^2) = min over dz of (dz^2 + min over dy of (dy^2 + min over dx of dx^2)),
// and a true d2 <= R * R has every axis offset <= R, so each axis searches a window of R and the clamp keeps the result exact.  Three
// launches behind k_match_bits (map_match.h, included and called: the occupancy image of THIS call's threshold):
//
//   k_dist_x   from the bit image.  One lane per voxel of a row; the nearest set bit to the right (self included) and to the left
//              within R by word scans - __ffsll / __clzll over at most ceil(R / 64) + 1 words each way, not a sweep.  Rows do not
//              start on word boundaries: the first and the last word of a search are masked to [lo, hi], which is the window
//              clamped to the ROW, so a row never sees the bits that its words share with its neighbours.  Writes
//              min(R * R, dx * dx) as uint16 - "nothing within R" is a distance beyond every radius, and the min is the clamp.
//   k_dist_y   out[y] = min over |d| <= R of (in[y + d] + d * d) along y.  A block owns 64 columns x MD_TY rows of one z plane and
//              stages the rows [y0 - R, y0 + MD_TY + R), clamped to the axis, in LDS (uint16, lanes along x: coalesced loads, two
//              lanes per bank word, no conflict); a lane owns a column and every fourth row.  The search leaves as soon as
//              d * d >= the best so far: in[] <= R * R, so that is at d = R at the latest, and next to a surface after a step or two.
//              HALO (16 / 64 / 255) is the largest radius an instantiation has LDS rows for: 8 / 20 / 68 KiB.
//   k_dist_z   the same along z, read from global memory: lanes run along the plane (x fastest), a step of d is one coalesced load
//              a plane further - neighbouring planes are L2 / Infinity-Cache traffic.
//
// No pass runs in place: bits -> A -> B -> the caller's device buffer, or A again when the output goes to the host.  No index
// outside an allocation is ever formed: every window is clamped to its axis BEFORE an address is made, nothing is loaded and
// discarded.  The work is O(N * R) in the worst case (open space far from everything at a large R); times: tools/map_distance_bench.py, DESIGN.md 5.22.
//
// Scoring by the field (vofod_map_match_field, profiler label k_match_field) is map_match.h's one walk, vmm::k_match<U, LookField>:
// the policy there says what a look-up of the field counts and why its sum cannot wrap.  Nothing of that walk is restated here.
// Out of scope: a feature transform (the nearest voxel's index), an O(N) lower-envelope scan, a field patched by the map update.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device_mem.h"
#include "map_match.h"

namespace vmd
{
using namespace vk;

constexpr uint32_t MD_MAX_RADIUS = 255;   // R * R <= 65025 fits uint16_t
constexpr uint32_t MD_NOT_FOUND = 256;    // k_dist_x: an x distance beyond every radius (its square, 65536, is above every clamp)
constexpr uint32_t MD_TX = 64, MD_TY = 32, MD_YSTEP = 4;  // k_dist_y: columns and rows of a block's tile; 256 threads = 64 x 4
constexpr uint32_t MD_MAX_GRID = 65535;   // gridDim.y: a longer list of rows / tiles / planes folds into gridDim.z

// the workspace of the two calls, owned by the handle and grown to the largest seen (the occupancy image is vmm::Workspace's)
struct Workspace
{
  DevBuf<uint16_t> d_a, d_b;          // the passes' intermediate fields, n_voxels each; d_a is also the staging of a host output
  DevBuf<uint16_t> d_field;           // vofod_map_match_field: a host field
  DevBuf<unsigned long long> d_cost;  // one sum per candidate
  std::vector<unsigned long long> h_cost;
};

__global__ __launch_bounds__(256) void k_dist_x(const unsigned long long* __restrict__ bits, uint32_t sx, uint32_t n_rows, uint32_t R, uint16_t* __restrict__ out)
{
  const uint32_t row = blockIdx.z * gridDim.y + blockIdx.y;  // z * sy + y
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (row >= n_rows || x >= sx)
    return;
  const uint64_t first = static_cast<uint64_t>(row) * sx, p = first + x;  // the row's first bit, this voxel's bit
  // the window, clamped to the row: the only bits a search may see
  const uint64_t lo = x > R ? p - R : first, hi = x + R < sx ? p + R : first + sx - 1u;
  uint32_t dx = MD_NOT_FOUND;
  {  // to the right, self included: the lowest set bit of [p, hi]
    uint64_t w = p >> 6;
    const uint64_t w_end = hi >> 6;
    unsigned long long m = bits[w] & (~0ull << (p & 63u));
    for (;;)
    {
      if (w == w_end)
        m &= ~0ull >> (63u - (hi & 63u));
      if (m)
      {
        dx = static_cast<uint32_t>((w << 6) + static_cast<uint32_t>(__ffsll(m) - 1) - p);
        break;
      }
      if (w == w_end)
        break;
      m = bits[++w];
    }
  }
  if (dx > 1u)
  {  // to the left: the highest set bit of [lo, p]
    uint64_t w = p >> 6;
    const uint64_t w_end = lo >> 6;
    unsigned long long m = bits[w] & (~0ull >> (63u - (p & 63u)));
    for (;;)
    {
      if (w == w_end)
        m &= ~0ull << (lo & 63u);
      if (m)
      {
        dx = min(dx, static_cast<uint32_t>(p - ((w << 6) + 63u - static_cast<uint32_t>(__clzll(m)))));
        break;
      }
      if (w == w_end)
        break;
      m = bits[--w];
    }
  }
  out[p] = static_cast<uint16_t>(min(R * R, dx * dx));  // (the clamp: nothing within R is R * R)
}

template <uint32_t HALO>
__global__ __launch_bounds__(256) void k_dist_y(const uint16_t* __restrict__ in, uint32_t sx, uint32_t sy, uint32_t y_tiles, uint32_t n_tiles, uint32_t R, uint16_t* __restrict__ out)
{
  __shared__ uint16_t s_col[(MD_TY + 2u * HALO) * MD_TX];
  const uint32_t t = blockIdx.z * gridDim.y + blockIdx.y;  // z * y_tiles + the tile along y
  if (t >= n_tiles)
    return;  // (the whole block)
  const uint32_t z = t / y_tiles, y0 = (t - z * y_tiles) * MD_TY;
  const uint32_t lx = threadIdx.x & 63u, ly = threadIdx.x >> 6;
  const uint32_t x = blockIdx.x * MD_TX + lx;
  // the staged rows [ya, yb): the tile and R rows either side, clamped to the axis; R <= HALO, so at most MD_TY + 2 * HALO of them
  const uint32_t ya = y0 > R ? y0 - R : 0u, yb = min(sy, y0 + MD_TY + R), ye = min(sy, y0 + MD_TY);
  const uint64_t plane = static_cast<uint64_t>(z) * sy * sx;
  if (x < sx)
    for (uint32_t y = ya + ly; y < yb; y += MD_YSTEP)
      s_col[(y - ya) * MD_TX + lx] = in[plane + static_cast<uint64_t>(y) * sx + x];
  __syncthreads();
  if (x >= sx)
    return;
  for (uint32_t y = y0 + ly; y < ye; y += MD_YSTEP)
  {
    uint32_t best = s_col[(y - ya) * MD_TX + lx];
    for (uint32_t d = 1; d <= R && d * d < best; d++)
    {
      if (y >= ya + d)  // (y - d is a staged row: ya is 0 or y0 - R, and d <= R)
        best = min(best, s_col[(y - d - ya) * MD_TX + lx] + d * d);
      if (y + d < yb)
        best = min(best, s_col[(y + d - ya) * MD_TX + lx] + d * d);
    }
    out[plane + static_cast<uint64_t>(y) * sx + x] = static_cast<uint16_t>(best);
  }
}

__global__ __launch_bounds__(256) void k_dist_z(const uint16_t* __restrict__ in, uint64_t plane, uint32_t sz, uint32_t R, uint16_t* __restrict__ out)
{
  const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;  // y * sx + x
  const uint32_t z = blockIdx.z * gridDim.y + blockIdx.y;
  if (p >= plane || z >= sz)
    return;
  const uint16_t* col = in + p;
  uint32_t best = col[z * plane];
  for (uint32_t d = 1; d <= R && d * d < best; d++)
  {
    if (z >= d)
      best = min(best, col[(z - d) * plane] + d * d);
    if (z + d < sz)
      best = min(best, col[(z + d) * plane] + d * d);
  }
  out[z * plane + p] = static_cast<uint16_t>(best);
}

}  // namespace vmd
