// Rolling operation area (include/vofod.h, vofod_map_shift): the three dense maps move by a whole number of voxels and keep what
// they hold about the overlap.  The reference has no counterpart: its maps are resized once, in onInit (voxel_map.cpp:11-48).
//
//   area_geometry  the one place where an operation_area/offset becomes the centres, the map origin and the map sizes
//                  (vofod_nodelet.cpp:204, :212, :229; VoxelMap::resize voxel_map.cpp:11-48).  vofod_create and vofod_map_shift both
//                  call it, so a shifted handle holds bit for bit the geometry of a handle created at the new offset.  Plain host
//                  code on plain structs: it compiles without the HIP runtime.
//   k_map_shift    dst[i] = src[i + D] where the voxel i + shift is inside the map, the map's init value elsewhere;
//                  D = s0 + s1*sx + s2*sx*sy.  OUT OF PLACE: dst is the handle's spare buffer (4 * M bytes, allocated on the first
//                  shift, freed by vofod_destroy); the driver then swaps the two owners, so the spare of the next map is the old
//                  buffer of this one.  (An in-place shift races between workgroups wherever source and destination ranges overlap.)
//                  The destination is walked as a linear array in tiles of SH_TILE consecutive voxels, grid-stride with a capped grid;
//                  a lane owns SH_QPL quads of 4 voxels per tile, loads all of them and only then stores - one 16-byte aligned store
//                  per quad (the last quad of a map whose M is no multiple of 4: element stores).  A tile's first voxel is
//                  decomposed into (ix, iy, iz) once with 64-bit arithmetic (uniform over the workgroup); a quad's own coordinates
//                  follow from its offset inside the tile with 32-bit arithmetic.
//                  Rows are sx = ceil(size / vs) + 1 voxels long - usually odd - so a quad may straddle a row end or a plane end:
//                  validity is decided per voxel.  Loads: a quad of four valid voxels is one 16-byte load (global_load_dwordx4; its
//                  address is only 4-byte aligned when D % 4 != 0, which the type Quad4 tells the compiler; the hardware takes
//                  either).  A valid voxel's source index is that of a voxel of the map, so such a quad lies inside [0, M).  The
//                  lanes of every other quad load too, so that no branch stands between the loads of a tile, but from an address
//                  CLAMPED to the first quad of the source, and drop what they get; those quads follow voxel by voxel behind the
//                  16-byte stores, reading valid voxels only.  No load is issued for an address outside the source, not even one
//                  whose value is dropped.
//                  No atomics, no LDS.  hipcc's resource remarks (gfx950): tools/DESIGN.in.md, section 5.10.
//
// Scratch that is indexed by map voxel and outlives a call, and why each is safe behind a shift (vofod_map_shift refuses while a
// submitted batch, a raycast pass or a sepclusters pass is pending, so nothing below is in use during the call):
//   d_mapbits, d_mapclose, d_bgcount   occupancy image, its dilation and nVoxelsOver: mapbits_valid = false rebuilds the first and
//                                      the third on next use and advances mapbits_gen, which the dilated image is keyed on.
//   ExploreBufs::d_overlay, d_visited  frontier overlay and visited bits of the flood fills: k_explore / k_tail_far leave both
//                                      all-zero when they end (kernels_classify.h "leave the overlay clean"); zero shifts to zero.
//   MapSyncState::d_shadow             what the owner exported last: the chain ends (chain_gen = 0, applied_gen = 0), the next delta is
//                                      refused and a full export rewrites every word of the shadow before anything compares with it.
//   sepws (cluster list of a pass)     map indices of a sepclusters pass between begin and finish: refused while sep_pending.
//   d_ray under raycast_pending        the ray lengths of a pass between begin and finish: refused while raycast_pending; outside a
//                                      pass the map is zero or marked ray_dirty, and both states survive a shift as they are.
//   vws::Store (world_store.h)         NOT indexed by map voxel but by world index (window origin K + voxel): untouched by the swap; the
//                                      shift itself writes the leaving rim into it and reads the entering rim from it, and advances K.
//   Workspace::det_refs                detections vofod_detection_points would answer for belong to the old area: det_valid cleared.
// The voxel-grid lattices, the reference lattice of the frame kernel, the world crop and the cluster tables are derived from the
// handle's geometry inside every call (fill_grid_params, frame_plan / fill_ref_lattice, map_cmax): nothing of them is kept.
// Nothing caches the map pointers either: every launch takes h->d_map / d_flags / d_ray at call time and MapSyncState holds none.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/vofod.h"

namespace vsh
{

// what vofod_create derives from the static parameters' boxes
struct AreaGeometry
{
  float exclude_center[3], oparea_center[3];
  uint64_t background_min_sufficient_pts;
  float map_off[3];  // VoxelMap::origin
  int map_size[3];   // VoxelMap::sizesIdx
};

inline void area_geometry(const vofod_static_params& sp, AreaGeometry& g)
{
  for (int a = 0; a < 3; a++)
  {
    g.exclude_center[a] = sp.exclude_offset[a];
    g.oparea_center[a] = sp.oparea_offset[a];
  }
  g.exclude_center[2] = sp.exclude_offset[2] + sp.exclude_size[2] / 2.0f;  // vofod_nodelet.cpp:204
  g.oparea_center[2] = sp.oparea_offset[2] + sp.oparea_size[2] / 2.0f;     // :212
  const float n_voxels_xy = sp.oparea_size[0] / sp.voxel_size * sp.oparea_size[1] / sp.voxel_size;  // :229
  g.background_min_sufficient_pts = static_cast<uint64_t>(n_voxels_xy * sp.background_sufficient_points_ratio);
  // VoxelMap::resize voxel_map.cpp:11-48
  const float inv = 1.0f / sp.voxel_size;
  for (int a = 0; a < 3; a++)
  {
    g.map_off[a] = g.oparea_center[a] - sp.oparea_size[a] / 2.0f;
    g.map_size[a] = static_cast<int>(std::ceil(inv * sp.oparea_size[a])) + 1;
  }
}

constexpr int SH_THREADS = 256;
constexpr int SH_QPL = 4;                                // quads (16-byte loads) per lane and tile, all issued before the first store
constexpr uint32_t SH_TILE = 4u * SH_QPL * SH_THREADS;   // voxels per tile (4096: 16 KiB of map)
// cap of the workgroups that grid-stride over the tiles: eight are resident per CU, the others follow as those end (19.5 M voxels
// are 4 757 tiles, one each: 29.6 us per map against 33.0 us with 2 048 workgroups of two or three tiles, profiles/r14_map_shift.txt)
constexpr uint32_t SH_GRID = 8192;
constexpr uint32_t SH_WIDE = 16u;

struct ShiftParams
{
  uint64_t n;          // M = sx * sy * sz
  int64_t delta;       // s0 + s1*sx + s2*sx*sy
  int32_t sx, sy, sz;
  int32_t s0, s1, s2;  // |s[a]| <= S[a] (the driver clamps: a shift of S or more leaves nothing valid)
  uint32_t init;       // bit pattern of the map's init value
  uint32_t ntiles;
};

// 16 bytes at an address that is only known to be 4-byte aligned
struct __attribute__((packed, aligned(4))) Quad4
{
  uint32_t x, y, z, w;
};

__global__ __launch_bounds__(SH_THREADS) void k_map_shift(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const ShiftParams p)
{
  const uint32_t usx = static_cast<uint32_t>(p.sx), usy = static_cast<uint32_t>(p.sy), usz = static_cast<uint32_t>(p.sz);
  for (uint32_t t = blockIdx.x; t < p.ntiles; t += gridDim.x)
  {
    // tile prologue: the tile's first voxel as (ix0, iy0, iz0) - uniform over the workgroup
    const uint64_t base = static_cast<uint64_t>(t) * SH_TILE;
    const uint64_t row0 = base / usx;
    const uint32_t ix0 = static_cast<uint32_t>(base - row0 * usx);
    const uint64_t pl0 = row0 / usy;
    const uint32_t iy0 = static_cast<uint32_t>(row0 - pl0 * usy);
    const uint32_t iz0 = static_cast<uint32_t>(pl0);  // (< sz + 1)
    uint4 v[SH_QPL];
    uint32_t ok[SH_QPL];  // SH_WIDE: the quad went through the 16-byte load; otherwise bit e: voxel e takes the source's value
#pragma unroll
    for (int k = 0; k < SH_QPL; k++)
    {
      const uint32_t off = 4u * (static_cast<uint32_t>(k) * SH_THREADS + threadIdx.x);  // < SH_TILE
      // coordinates of the quad's first voxel: at most SH_TILE + sx - 1 past the row start, so 32 bits carry it
      uint32_t x = ix0 + off;
      const uint32_t dy = x / usx;
      x -= dy * usx;
      uint32_t y = iy0 + dy;
      const uint32_t dz = y / usy;
      y -= dz * usy;
      uint32_t z = iz0 + dz;
      uint32_t m = 0;
#pragma unroll
      for (int e = 0; e < 4; e++)
      {
        // (unsigned compare: a negative coordinate wraps above every size.)  z < sz keeps voxels past the end of the map out.
        const bool in = static_cast<uint32_t>(static_cast<int32_t>(x) + p.s0) < usx && static_cast<uint32_t>(static_cast<int32_t>(y) + p.s1) < usy &&
                        static_cast<uint32_t>(static_cast<int32_t>(z) + p.s2) < usz && z < usz;
        m |= static_cast<uint32_t>(in) << e;
        if (++x == usx)
        {
          x = 0;
          if (++y == usy)
          {
            y = 0;
            ++z;
          }
        }
      }
      // Four valid voxels: one 16-byte load.  Their source indices are voxels of the map, so the quad lies inside the source, and so
      // does the destination quad inside the map; the bounds are tested all the same.  Every other lane's ADDRESS is clamped to the
      // first quad of the source (vofod_create allocates at least four voxels per map) and what it loads is dropped: no branch
      // stands between the tile's loads, so all SH_QPL of them are in flight before the first store.
      const int64_t j = static_cast<int64_t>(base + off) + p.delta;
      const bool wide = m == 15u && j >= 0 && j + 4 <= static_cast<int64_t>(p.n);
      ok[k] = wide ? SH_WIDE : m;
      const uint32_t* q = src + (wide ? j : 0);
      const Quad4 u = *reinterpret_cast<const Quad4*>(q);
      v[k] = make_uint4(u.x, u.y, u.z, u.w);
    }
    // (an unconditional use of every loaded quad: the optimiser otherwise sinks each load into the branch of its store, and a wave
    // then waits for one load at a time)
#pragma unroll
    for (int k = 0; k < SH_QPL; k++)
      asm volatile("" : "+v"(v[k].x), "+v"(v[k].y), "+v"(v[k].z), "+v"(v[k].w));
#pragma unroll
    for (int k = 0; k < SH_QPL; k++)
      if (ok[k] == SH_WIDE)
        *reinterpret_cast<uint4*>(dst + base + 4u * (static_cast<uint32_t>(k) * SH_THREADS + threadIdx.x)) = v[k];
    // The other quads - across a row end, a plane end, the rim or the end of the map - voxel by voxel: only valid voxels are read
    // (a valid voxel's source index is a voxel's: inside [0, M)), the others take the init value.
#pragma unroll
    for (int k = 0; k < SH_QPL; k++)
    {
      const uint32_t m = ok[k];
      const uint64_t i = base + 4u * (static_cast<uint32_t>(k) * SH_THREADS + threadIdx.x);
      if (m == SH_WIDE || i >= p.n)
        continue;
      const uint32_t* e = src + (static_cast<int64_t>(i) + p.delta);
      uint4 o = make_uint4(p.init, p.init, p.init, p.init);
      if (m & 1u)
        o.x = e[0];
      if (m & 2u)
        o.y = e[1];
      if (m & 4u)
        o.z = e[2];
      if (m & 8u)
        o.w = e[3];
      if (i + 4 <= p.n)
        *reinterpret_cast<uint4*>(dst + i) = o;
      else
      {
        dst[i] = o.x;
        if (i + 1 < p.n)
          dst[i + 1] = o.y;
        if (i + 2 < p.n)
          dst[i + 2] = o.z;
      }
    }
  }
}

}  // namespace vsh
