// The member voxels and the AABB of every detection (include/vofod.h, vofod_detection_points): cluster_t::pc / pc_indices and
// detection_t::aabb of the reference (vofod_nodelet.cpp:110-130), gathered on the device from what every route leaves in the
// workspace - the frame's candidate member list (CandMember{root, v}, FrameHdr::n_cand entries) and its voxel records (float4:
// centre + bits(count), the layout of vofod_point_xyzr).  Nothing else is read: the kernel does not know which route ran.
//
//   k_det_points   one workgroup of 256 threads per detection.
//     1. walk the frame's list [0, n_cand) 256 entries at a time (one 8-byte load per lane, consecutive lanes consecutive entries)
//        and keep the entries whose root is the detection's: ballot + mbcnt inside a wave, the waves' counts through LDS, a
//        running offset per workgroup.  The kept voxel indices go to an LDS list of DP_CAP entries;
//     2. rank every kept v by counting the kept v below it (a voxel appears once in the list: the ranks are a permutation).  The
//        close-first frame kernel and k_far_final write a cluster's members ascending already, k_finalize, the full frame kernel
//        and the lists beyond the tail's capacities do not - the kernel asks nobody;
//     3. pts[v] (one 16-byte load, one 16-byte store) and v go to first + rank;
//     4. float min / max of the centres: per thread, across the wave by shuffles, across the waves through LDS.  No atomics: the
//        result is the plain float min / max getMinMax3D computes, whatever the order;
//     5. the number of members found is reported with the box: the host holds it against the detection's n_points
//        (VOFOD_ERR_DEVICE when they differ); a workgroup that finds another number stores no point at all, so nothing is ever
//        written outside [first, first + n_points).
//   A detection of more than DP_CAP members takes one pass per DP_CAP of them: the pass walks the list for its share of the kept
//   entries, then once more, tile by tile through LDS, to count every kept entry below each of them.
//
// Is [0, n_cand) dense?  Yes, on every route.  Each writer either takes its slots with an atomic add on n_cand / a workgroup
// counter and fills every slot it took (k_finalize, the full frame kernel's label pass, the unordered branches of the close-first
// kernel and of k_far_final), or places n_cand staged keys by counting, a permutation of [0, n_cand) (the ordered branches).
// ClusterRec::cand is a 0 / 1 flag in all of them - there are no per-cluster slot ranges with gaps between them (the comment on
// that field in common.h describes a layout the kernels no longer write).  A frame whose status is not VOFOD_OK has no
// detections, so its n_cand is never looked at; the kernel clamps n_cand and every v to the frame's slot all the same.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

namespace vdp
{

constexpr int DP_THREADS = 256;
constexpr int DP_WAVES = DP_THREADS / vk::WAVE;
constexpr uint32_t DP_CAP = 512;  // members ranked from one LDS list (detections are small: max_size bounds them to a few hundred voxels)
constexpr int DP_PER = DP_CAP / DP_THREADS;

// one detection: host -> device
struct DetDesc
{
  uint32_t frame;     // frame slot of the workspace
  uint32_t root;      // label of the cluster (CandMember::root of its members)
  uint32_t first;     // where its members go in the output
  uint32_t n_points;  // how many the tail counted
};

// ... and back
struct DetBox
{
  float aabb_min[3], aabb_max[3];
  uint32_t found;  // members in the list; the box and the points are valid when it equals n_points
  uint32_t pad_;
};
static_assert(sizeof(DetDesc) == 16 && sizeof(DetBox) == 32, "detection descriptors: whole 16-byte words");

// Position of this lane's entry among the kept entries of the walk (valid where `keep`); `seen` counts the kept entries of the
// tiles so far and is the same in every thread.  One barrier per tile: the waves' counts alternate between two rows, and a wave
// two tiles ahead has passed the barrier every reader of the row's previous use had to reach first.
__device__ __forceinline__ uint32_t dp_slot(bool keep, uint32_t (*s_wcnt)[DP_WAVES], uint32_t& tile, uint32_t& seen)
{
  const unsigned long long m = __ballot(keep);
  const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
  const uint32_t wave = threadIdx.x / vk::WAVE, row = tile++ & 1u;
  if ((threadIdx.x & (vk::WAVE - 1)) == 0)
    s_wcnt[row][wave] = static_cast<uint32_t>(__popcll(m));
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < static_cast<uint32_t>(DP_WAVES); w++)
  {
    const uint32_t c = s_wcnt[row][w];
    before += w < wave ? c : 0u;
    all += c;
  }
  const uint32_t pos = seen + before + below;
  seen += all;
  return pos;
}

__global__ __launch_bounds__(DP_THREADS) void k_det_points(const vk::FrameHdr* __restrict__ hdrs, const vk::CandMember* __restrict__ cand_all, const float4* __restrict__ pts_all, uint32_t vox_cap,
                                                           const DetDesc* __restrict__ descs, float4* __restrict__ out_pts, uint32_t* __restrict__ out_idx, DetBox* __restrict__ boxes)
{
  __shared__ uint32_t s_v[DP_CAP];
  __shared__ uint32_t s_t[DP_THREADS];
  __shared__ uint32_t s_wcnt[2][DP_WAVES];
  __shared__ float s_red[DP_WAVES][6];
  const DetDesc d = descs[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const vk::CandMember* cand = cand_all + static_cast<size_t>(d.frame) * vox_cap;
  const float4* pts = pts_all + static_cast<size_t>(d.frame) * vox_cap;
  const uint32_t n = min(hdrs[d.frame].n_cand, vox_cap);
  const uint32_t n_tiles = (n + DP_THREADS - 1u) / DP_THREADS;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  uint32_t found = 0, tile = 0;
  // (the loop's conditions are the same in every thread: `found` is a sum of counts all threads read from LDS)
  for (uint32_t q0 = 0; q0 == 0 || q0 < found; q0 += DP_CAP)
  {
    // 1: the kept entries number q0 .. q0 + DP_CAP - 1 of the list
    uint32_t seen = 0;
    for (uint32_t t = 0; t < n_tiles; t++)
    {
      const uint32_t i = t * DP_THREADS + tid;
      vk::CandMember cm{0xffffffffu, 0xffffffffu};
      if (i < n)
        cm = cand[i];
      const bool keep = i < n && cm.root == d.root && cm.v < vox_cap;
      const uint32_t pos = dp_slot(keep, s_wcnt, tile, seen);
      if (keep && pos >= q0 && pos - q0 < DP_CAP)
        s_v[pos - q0] = cm.v;
    }
    found = seen;
    if (found != d.n_points)
      break;  // 5: not the cluster the tail counted - nothing is stored
    __syncthreads();
    const uint32_t nq = min(found - q0, DP_CAP);
    // 2: ranks by counting
    uint32_t mine[DP_PER], rank[DP_PER];
#pragma unroll
    for (int k = 0; k < DP_PER; k++)
    {
      const uint32_t i = tid + k * DP_THREADS;
      mine[k] = i < nq ? s_v[i] : 0u;  // (nothing is below 0: the ranks of the unused slots stay 0 and are not stored)
      rank[k] = 0;
    }
    if (found <= DP_CAP)
    {
      for (uint32_t j = 0; j < nq; j++)
      {
        const uint32_t vj = s_v[j];  // (one address for the whole wave: a broadcast)
#pragma unroll
        for (int k = 0; k < DP_PER; k++)
          rank[k] += vj < mine[k] ? 1u : 0u;
      }
    }
    else
    {
      uint32_t seen2 = 0;
      for (uint32_t t = 0; t < n_tiles; t++)
      {
        const uint32_t i = t * DP_THREADS + tid;
        vk::CandMember cm{0xffffffffu, 0xffffffffu};
        if (i < n)
          cm = cand[i];
        const bool keep = i < n && cm.root == d.root && cm.v < vox_cap;
        const uint32_t base = seen2;
        const uint32_t pos = dp_slot(keep, s_wcnt, tile, seen2);
        if (keep)
          s_t[pos - base] = cm.v;
        __syncthreads();
        const uint32_t nt = seen2 - base;
        for (uint32_t j = 0; j < nt; j++)
        {
          const uint32_t vj = s_t[j];
#pragma unroll
          for (int k = 0; k < DP_PER; k++)
            rank[k] += vj < mine[k] ? 1u : 0u;
        }
        __syncthreads();  // (the next tile overwrites s_t)
      }
    }
    // 3 + 4: the records to their places, the box
#pragma unroll
    for (int k = 0; k < DP_PER; k++)
    {
      const uint32_t i = tid + k * DP_THREADS;
      if (i < nq)
      {
        const float4 p = pts[mine[k]];
        const size_t o = static_cast<size_t>(d.first) + rank[k];  // (rank < found == n_points)
        out_pts[o] = p;
        out_idx[o] = mine[k];
        mn[0] = fminf(mn[0], p.x), mn[1] = fminf(mn[1], p.y), mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x), mx[1] = fmaxf(mx[1], p.y), mx[2] = fmaxf(mx[2], p.z);
      }
    }
    __syncthreads();  // (the next pass overwrites s_v)
  }
  // 4: across the wave, then across the waves
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int s = vk::WAVE / 2; s > 0; s >>= 1)
    {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], s));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], s));
    }
  if ((tid & (vk::WAVE - 1)) == 0)
    for (int a = 0; a < 3; a++)
    {
      s_red[tid / vk::WAVE][a] = mn[a];
      s_red[tid / vk::WAVE][3 + a] = mx[a];
    }
  __syncthreads();
  if (tid == 0)
  {
    DetBox b;
    for (int a = 0; a < 3; a++)
    {
      b.aabb_min[a] = fminf(fminf(s_red[0][a], s_red[1][a]), fminf(s_red[2][a], s_red[3][a]));
      b.aabb_max[a] = fmaxf(fmaxf(s_red[0][3 + a], s_red[1][3 + a]), fmaxf(s_red[2][3 + a], s_red[3][3 + a]));
    }
    b.found = found;
    b.pad_ = 0;
    boxes[blockIdx.x] = b;
  }
  static_assert(DP_WAVES == 4, "the last reduction step names the four waves");
}

}  // namespace vdp
