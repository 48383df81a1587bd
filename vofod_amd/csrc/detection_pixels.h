// The raw returns of every detection (include/vofod.h, vofod_detection_pixels): which pixels i = row * width + col of the organised
// scan fell into the detection's member voxels, with the point the pipeline consumed.  Answered on the device from what every route
// leaves in the workspace after a production call:
//   ws.d_args      the frame's arguments: tf and the x / y / z columns the kernels read - the caller's device memory, the struct
//                  block of a host scan (d_stage_aos), or the frame's staging slot (d_stage: copied, decoded or deskewed points);
//   ws.d_hdrs      the frame's own VoxelGridWeighted lattice (FrameHdr::offset, div_b: k_grid, or the frame kernel's lattice step);
//   ws.d_cand      the candidate member list, ws.va.pts the voxel records (centre + bits(weight)): as in detection_points.h;
//   ws.det_g       the GridParams of the launch (crop boxes, leaf), kept by the record builders beside the DetRef list.
// fetch_point and cell_key (kernels_voxelize.h) say "which cell does pixel i fall in" here as they do in the pipeline.
//
//   k_det_pixel_sizes   one workgroup per detection: the sum of bits(pts[v].w) over its members, and how many members the list holds.
//                       One round trip gives the host every count, the prefix `first` and the capacity decision before a pixel is read.
//   k_det_pixels        one workgroup of 256 threads per detection.
//     1. gather the members as k_det_points does (ballot + mbcnt walk of [0, n_cand)).  A member's cell comes from its record's
//        centre and the frame's offset: k = floor((c - offset) * inv), accepted (or k - 1, k + 1) only when re-centring it,
//        (k + 0.5) * leaf + offset in the pipeline's own float expression, reproduces the centre's bits; a centre no cell
//        reproduces is reported (VOFOD_ERR_DEVICE).  The key is cell_key's: i0 + i1 * div_b[0] + i2 * div_b[0] * div_b[1].
//        The keys are sorted by counting (a voxel owns its cell: the keys of a detection are distinct, the positions a permutation)
//        into an LDS list of PX_CAP entries, beside each key the member's rank by v - its position in the list
//        vofod_detection_points returns.  The float box of the centres, widened by one leaf, is the reject box of step 2.
//     2. walk the frame's pixels in order, PX_PPT * 256 per step: fetch_point for the step's PX_PPT pixels of every thread first
//        (unconditional loads at a clamped index: all of a step's loads are in flight before the first use), then the box reject
//        (almost every pixel ends here), then cell_key and a binary search in the sorted list.
//     3. the hits of a step are placed by ballot + mbcnt per wave, the waves' counts through LDS and a running workgroup offset:
//        pixels ascend because the walk does.  No atomics decide an order anywhere.
//     4. the number found is reported; the host holds it against the sum of the weights.  Nothing is ever stored outside
//        [first, first + count).
//   A detection of more than PX_CAP members takes one pass of step 1 per PX_CAP of them, as k_det_points does: each pass ranks its
//   share against the whole list (tile by tile through LDS) and puts it at its sorted positions in a staging list in global memory
//   (ws.d_pxkey / d_pxrank, the detection's own range).  When the last pass is through, the ONE pixel walk of steps 2-4 searches that
//   list instead of the LDS copy (the search is the same code on a generic pointer; only the pixels inside the box reach it) - so
//   the output is one ascending list whatever the number of passes.
//
// Who writes the inputs between a launch and the end of det_valid?
//   d_args                   launch_frame_args (launch_voxelize / launch_lattice), once per launch from h_args.  A launch clears
//                            det_valid first (launch_frames, stage_inputs).  The cloud voxelisers (vofod_voxel_grid_*) and
//                            sepclusters use workspaces of their own (h->aux, h->sepws).  stage_cloud called by
//                            raycast_begin_locked rewrites h_args[0] on the HOST only; nothing uploads it before the next launch.
//   the slot's x, y, z       stage_inputs (2-D copy, stage_cloud / stage_host_column), k_range_decode, k_point_deskew: all inside
//   (d_stage columns 0-2)    a launch, or inside vofod_range_to_points / vofod_deskew_points, which go through stage_inputs and
//                            so end the validity.  raycast_begin_locked (vofod_raycast_begin, VOFOD_SCAN_AUTO_RAYCAST) takes slot 0
//                            of the synchronous workspace for a host scan, but stages the two columns its kernel reads only -
//                            intensity and range, columns 3-4 - for a range image and for a point scan alike (it hands
//                            stage_cloud no x, y, z): columns 0-2 stay the launch's, also where they hold deskewed points.
//   d_stage_aos              stage_cloud inside a launch only (raycast_begin_locked passes intensity and range: the gather path).
//   caller's device columns  the caller: they are read in place, and must be left unchanged until the call has been made.  The
//                            count check of step 4 is what notices when they were not.
//   d_hdrs, d_cand, va.pts   as in detection_points.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "detection_points.h"
#include "kernels_voxelize.h"

namespace vpx
{

constexpr int PX_THREADS = vdp::DP_THREADS;
constexpr int PX_WAVES = PX_THREADS / vk::WAVE;
constexpr uint32_t PX_CAP = 512;  // member cells searched in LDS; a larger detection builds its sorted list in global memory
constexpr int PX_PER = PX_CAP / PX_THREADS;
constexpr int PX_PPT = 4;  // pixels per thread and step of the walk
constexpr uint32_t PX_STEP = PX_THREADS * PX_PPT;

// one detection: host -> device (the sizing kernel reads frame and root only)
struct PixDesc
{
  uint32_t frame;     // frame slot of the workspace
  uint32_t root;      // label of the cluster
  uint32_t n_points;  // member voxels the tail counted
  uint32_t mfirst;    // where its sorted member list goes in the staging lists
  uint32_t first;     // where its pixels go in the output
  uint32_t count;     // the sum of its members' weights
  uint32_t pad_[2];
};

// ... and back
struct PixSize
{
  uint32_t count, members;
};
struct PixFound
{
  uint32_t pixels;   // returns found; the output is valid when it equals count
  uint32_t members;  // entries of the frame's member list
  uint32_t bad;      // members whose centre no cell of the frame's lattice reproduces
  uint32_t pad_;
};
static_assert(sizeof(PixDesc) == 32 && sizeof(PixSize) == 8 && sizeof(PixFound) == 16, "pixel descriptors: whole words");

__global__ __launch_bounds__(PX_THREADS) void k_det_pixel_sizes(const vk::FrameHdr* __restrict__ hdrs, const vk::CandMember* __restrict__ cand_all, const float4* __restrict__ pts_all, uint32_t vox_cap,
                                                                const PixDesc* __restrict__ descs, PixSize* __restrict__ sizes)
{
  __shared__ uint32_t s_red[PX_WAVES][2];
  const PixDesc d = descs[blockIdx.x];
  const vk::CandMember* cand = cand_all + static_cast<size_t>(d.frame) * vox_cap;
  const float4* pts = pts_all + static_cast<size_t>(d.frame) * vox_cap;
  const uint32_t n = min(hdrs[d.frame].n_cand, vox_cap);
  uint32_t cnt = 0, mem = 0;
  for (uint32_t i = threadIdx.x; i < n; i += PX_THREADS)
  {
    const vk::CandMember cm = cand[i];
    if (cm.root == d.root && cm.v < vox_cap)
    {
      mem++;
      cnt += __float_as_uint(pts[cm.v].w);
    }
  }
  cnt = vk::wave_sum(cnt);
  mem = vk::wave_sum(mem);
  if ((threadIdx.x & (vk::WAVE - 1)) == 0)
  {
    s_red[threadIdx.x / vk::WAVE][0] = cnt;
    s_red[threadIdx.x / vk::WAVE][1] = mem;
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    PixSize s{0, 0};
    for (int w = 0; w < PX_WAVES; w++)
    {
      s.count += s_red[w][0];
      s.members += s_red[w][1];
    }
    sizes[blockIdx.x] = s;
  }
}

// the cell along one axis whose centre (kernels_voxelize.h, k_emit: (k + 0.5) * leaf + offset, every op rounded) is `c` bit for bit
__device__ __forceinline__ bool cell_of_centre(float c, float off, float leaf, float inv, int& k)
{
  const int e = static_cast<int>(floorf(__fmul_rn(__fsub_rn(c, off), inv)));
#pragma unroll
  for (int t = 0; t < 3; t++)
  {
    const int kk = e + (t == 0 ? 0 : t == 1 ? -1 : 1);
    const float r = __fadd_rn(__fmul_rn(__fadd_rn(static_cast<float>(kk), 0.5f), leaf), off);
    if (__float_as_uint(r) == __float_as_uint(c))
    {
      k = kk;
      return true;
    }
  }
  k = e;
  return false;
}

// cell_key's key of the member voxel with record `p`
__device__ __forceinline__ uint32_t member_key(const vk::FrameHdr& h, const vk::GridParams& g, const float4& p, bool& ok)
{
  int i0, i1, i2;
  ok = cell_of_centre(p.x, h.offset[0], g.leaf[0], g.inv[0], i0);
  ok = cell_of_centre(p.y, h.offset[1], g.leaf[1], g.inv[1], i1) && ok;
  ok = cell_of_centre(p.z, h.offset[2], g.leaf[2], g.inv[2], i2) && ok;
  return static_cast<uint32_t>(i0 + i1 * h.div_b[0] + i2 * h.div_b[0] * h.div_b[1]);
}

__global__ __launch_bounds__(PX_THREADS) void k_det_pixels(const vk::FrameArgs* __restrict__ args, const vk::GridParams g, const vk::FrameHdr* __restrict__ hdrs,
                                                           const vk::CandMember* __restrict__ cand_all, const float4* __restrict__ pts_all, uint32_t vox_cap, const PixDesc* __restrict__ descs,
                                                           uint32_t* gkey, uint32_t* grank, uint32_t* __restrict__ out_px, uint32_t* __restrict__ out_member, float* __restrict__ out_xyz,
                                                           PixFound* __restrict__ found_out)
{
  __shared__ uint32_t s_v[PX_CAP], s_k[PX_CAP];    // the pass's share of the members, in list order
  __shared__ uint32_t s_sk[PX_CAP], s_sr[PX_CAP];  // keys ascending, and the rank by v beside each (detections of PX_CAP members at most)
  __shared__ uint32_t s_tv[PX_THREADS], s_tk[PX_THREADS];
  __shared__ uint32_t s_w1[2][vdp::DP_WAVES];
  __shared__ uint32_t s_wcnt[2][PX_PPT][PX_WAVES];
  __shared__ float s_red[PX_WAVES][6];
  __shared__ uint32_t s_bad;
  const PixDesc d = descs[blockIdx.x];
  const uint32_t tid = threadIdx.x, wave = tid / vk::WAVE;
  const vk::FrameHdr h = hdrs[d.frame];
  const vk::CandMember* cand = cand_all + static_cast<size_t>(d.frame) * vox_cap;
  const float4* pts = pts_all + static_cast<size_t>(d.frame) * vox_cap;
  const uint32_t n = min(h.n_cand, vox_cap);
  const uint32_t n_tiles = (n + PX_THREADS - 1u) / PX_THREADS;
  const bool big = d.n_points > PX_CAP;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  uint32_t found = 0, tile = 0, bad = 0;
  if (tid == 0)
    s_bad = 0;
  // ---- 1: the members' cells, sorted (the loop's conditions are the same in every thread, as in k_det_points)
  for (uint32_t q0 = 0; q0 == 0 || q0 < found; q0 += PX_CAP)
  {
    uint32_t seen = 0;
    for (uint32_t t = 0; t < n_tiles; t++)
    {
      const uint32_t i = t * PX_THREADS + tid;
      vk::CandMember cm{0xffffffffu, 0xffffffffu};
      if (i < n)
        cm = cand[i];
      const bool keep = i < n && cm.root == d.root && cm.v < vox_cap;
      const uint32_t pos = vdp::dp_slot(keep, s_w1, tile, seen);
      if (keep && pos >= q0 && pos - q0 < PX_CAP)
      {
        const float4 p = pts[cm.v];
        bool ok;
        s_v[pos - q0] = cm.v;
        s_k[pos - q0] = member_key(h, g, p, ok);
        bad += ok ? 0u : 1u;
        mn[0] = fminf(mn[0], p.x), mn[1] = fminf(mn[1], p.y), mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x), mx[1] = fmaxf(mx[1], p.y), mx[2] = fmaxf(mx[2], p.z);
      }
    }
    found = seen;
    if (found != d.n_points)
      break;  // not the cluster the tail counted: no pixel is read
    __syncthreads();
    const uint32_t nq = min(found - q0, PX_CAP);
    uint32_t mine_v[PX_PER], mine_k[PX_PER], rank[PX_PER], at[PX_PER];
#pragma unroll
    for (int k = 0; k < PX_PER; k++)
    {
      const uint32_t i = tid + k * PX_THREADS;
      mine_v[k] = i < nq ? s_v[i] : 0u;  // (nothing is below 0: the counts of the unused slots stay 0 and are not stored)
      mine_k[k] = i < nq ? s_k[i] : 0u;
      rank[k] = at[k] = 0;
    }
    if (!big)
    {
      for (uint32_t j = 0; j < nq; j++)
      {
        const uint32_t vj = s_v[j], kj = s_k[j];  // (one address for the whole wave: a broadcast)
#pragma unroll
        for (int k = 0; k < PX_PER; k++)
        {
          rank[k] += vj < mine_v[k] ? 1u : 0u;
          at[k] += kj < mine_k[k] ? 1u : 0u;
        }
      }
    }
    else
    {
      uint32_t seen2 = 0;
      for (uint32_t t = 0; t < n_tiles; t++)
      {
        const uint32_t i = t * PX_THREADS + tid;
        vk::CandMember cm{0xffffffffu, 0xffffffffu};
        if (i < n)
          cm = cand[i];
        const bool keep = i < n && cm.root == d.root && cm.v < vox_cap;
        const uint32_t base = seen2;
        const uint32_t pos = vdp::dp_slot(keep, s_w1, tile, seen2);
        if (keep)
        {
          bool ok;
          s_tv[pos - base] = cm.v;
          s_tk[pos - base] = member_key(h, g, pts[cm.v], ok);
        }
        __syncthreads();
        const uint32_t nt = seen2 - base;
        for (uint32_t j = 0; j < nt; j++)
        {
          const uint32_t vj = s_tv[j], kj = s_tk[j];
#pragma unroll
          for (int k = 0; k < PX_PER; k++)
          {
            rank[k] += vj < mine_v[k] ? 1u : 0u;
            at[k] += kj < mine_k[k] ? 1u : 0u;
          }
        }
        __syncthreads();  // (the next tile overwrites s_tv / s_tk)
      }
    }
#pragma unroll
    for (int k = 0; k < PX_PER; k++)
    {
      const uint32_t i = tid + k * PX_THREADS;
      if (i >= nq)
        continue;
      if (big)  // (at < found == n_points: inside the detection's range of the staging lists)
      {
        gkey[static_cast<size_t>(d.mfirst) + at[k]] = mine_k[k];
        grank[static_cast<size_t>(d.mfirst) + at[k]] = rank[k];
      }
      else  // (at < nq <= PX_CAP)
      {
        s_sk[at[k]] = mine_k[k];
        s_sr[at[k]] = rank[k];
      }
    }
    __syncthreads();  // (the next pass overwrites s_v / s_k; the walk below reads the sorted list)
  }
  if (bad)
    atomicAdd(&s_bad, bad);
  // the members' float box, across the wave, then across the waves
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
      s_red[wave][a] = mn[a];
      s_red[wave][3 + a] = mx[a];
    }
  __syncthreads();
  static_assert(PX_WAVES == 4, "the last reduction step names the four waves");
  float lo[3], hi[3];
  for (int a = 0; a < 3; a++)
  {
    // a point of a member cell lies within half a leaf (and the roundings of the centre) of its centre: one leaf is generous
    lo[a] = fminf(fminf(s_red[0][a], s_red[1][a]), fminf(s_red[2][a], s_red[3][a])) - g.leaf[a];
    hi[a] = fmaxf(fmaxf(s_red[0][3 + a], s_red[1][3 + a]), fmaxf(s_red[2][3 + a], s_red[3][3 + a])) + g.leaf[a];
  }
  const uint32_t n_bad = s_bad;
  uint32_t placed = 0;
  if (found == d.n_points && n_bad == 0 && found > 0)
  {
    // ---- 2-4: the walk
    const vk::FrameArgs a = args[d.frame];
    const uint32_t* keys = big ? gkey + d.mfirst : s_sk;
    const uint32_t* ranks = big ? grank + d.mfirst : s_sr;
    const uint32_t nm = found;
    uint32_t row = 0;
    for (uint32_t base = 0; base < a.n; base += PX_STEP)
    {
      float q[PX_PPT][3];
      bool hit[PX_PPT];
      uint32_t rk[PX_PPT];
#pragma unroll
      for (int j = 0; j < PX_PPT; j++)
      {
        const uint32_t i = base + j * PX_THREADS + tid;
        hit[j] = vk::fetch_point(a, g, min(i, a.n - 1u), q[j]) && i < a.n;
        rk[j] = 0;
      }
#pragma unroll
      for (int j = 0; j < PX_PPT; j++)
      {
        if (!hit[j])
          continue;
        hit[j] = false;
        if (q[j][0] < lo[0] || q[j][1] < lo[1] || q[j][2] < lo[2] || q[j][0] > hi[0] || q[j][1] > hi[1] || q[j][2] > hi[2])
          continue;
        const uint32_t key = vk::cell_key(h, g, q[j]);
        uint32_t l = 0, r = nm;  // first entry >= key
        while (l < r)
        {
          const uint32_t m = (l + r) >> 1;
          if (keys[m] < key)
            l = m + 1;
          else
            r = m;
        }
        if (l < nm && keys[l] == key)
        {
          hit[j] = true;
          rk[j] = ranks[l];
        }
      }
      // 3: positions - the step's sub-tiles in order, inside a sub-tile the waves in order, inside a wave the lanes
      unsigned long long m[PX_PPT];
#pragma unroll
      for (int j = 0; j < PX_PPT; j++)
      {
        m[j] = __ballot(hit[j]);
        if ((tid & (vk::WAVE - 1)) == 0)
          s_wcnt[row][j][wave] = static_cast<uint32_t>(__popcll(m[j]));
      }
      __syncthreads();  // (one barrier per step: the rows alternate, see dp_slot)
      uint32_t run = placed;
#pragma unroll
      for (int j = 0; j < PX_PPT; j++)
      {
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < static_cast<uint32_t>(PX_WAVES); w++)
        {
          const uint32_t c = s_wcnt[row][j][w];
          before += w < wave ? c : 0u;
          all += c;
        }
        if (hit[j])
        {
          const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m[j] >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m[j]), 0u));
          const uint32_t pos = run + before + below;
          if (pos < d.count)  // (more returns than the weights say: counted, reported, not stored)
          {
            const size_t o = static_cast<size_t>(d.first) + pos;
            out_px[o] = base + j * PX_THREADS + tid;
            out_member[o] = rk[j];
            out_xyz[3 * o + 0] = q[j][0];
            out_xyz[3 * o + 1] = q[j][1];
            out_xyz[3 * o + 2] = q[j][2];
          }
        }
        run += all;
      }
      placed = run;
      row ^= 1u;
    }
  }
  if (tid == 0)
    found_out[blockIdx.x] = PixFound{placed, found, n_bad, 0u};
}

}  // namespace vpx
