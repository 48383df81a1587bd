// Device-side classification tail (gfx950): classify_cluster's boxes and gates (vofod_nodelet.cpp:1648-1696), the flood fills
// and the selection of the detections (extractDetections :834-879), so that the host only reads the few detection records
// back.  It takes every call nobody debugs that is a read-only batch of four frames or more, or one map-updating scan.
// Two chains, chosen per batch by launch_device_tail:
//   k_tail_far                               close-first frames (k_frame_lds_far, or k_far_final for a single scan): the
//                                            candidate clusters head the cluster table in canonical order and their members
//                                            follow cluster by cluster, so one wave per frame does the whole tail - boxes
//                                            and gates, the frame's flood fills (vc::explore_frame), the records;
//   k_tail_prep -> k_explore -> k_tail_finish  frames that went through the full clustering (no dilated map image, a cold map,
//                                            VOFOD_CLOSE_FIRST=0): k_tail_prep finds the candidates in the table and sorts their
//                                            members (bitonic sort in LDS) into the canonical order (size descending, smallest
//                                            member ascending: SURVEY H3), then boxes, gates and explore jobs, one lane per cluster;
//                                            k_explore (kernels_classify.h) runs the flood fills, k_tail_finish writes the records.
// What the two share is stated once: boxes, gates and the explore job's radius and box are vt::classify_gates (host_tail.h: the
// very function of the host tail), a lane's place among the wave's is rank_in_wave, the records and the slot's header are
// write_records / put_header.
// A frame beyond a capacity here (members, clusters, detections, Manhattan radius, flood-fill work list) sets a flag in its
// record slot: the host tail (frames_collect.h) then redoes the batch from the full tables.  The host tail also serves what
// never comes here: calls with debug output, batches of fewer than four frames, VOFOD_DEVICE_TAIL=0.
#pragma once
#include <hip/hip_runtime.h>

#include "host_tail.h"
#include "kernels_classify.h"
#include "kernels_voxelize.h"

namespace vtd
{

#ifndef TAIL_WPB_DEF
#define TAIL_WPB_DEF 8
#endif
constexpr int TAIL_WPB = TAIL_WPB_DEF;  // frames (waves) per workgroup of k_tail_far
#if TAIL_WPB_DEF >= 16
#define TAIL_OCC_ATTR
#else
#define TAIL_OCC_ATTR __attribute__((amdgpu_waves_per_eu(5, 5)))
#endif
using namespace vk;

constexpr int TAIL_STAGE = 512;  // candidate members per frame whose centres k_tail_far keeps in LDS (6 KB per wave)
constexpr int TP_THREADS = 256;
constexpr int TP_MAXM = TAIL_MAXM;  // candidate members per frame
constexpr int TP_MAXC = TAIL_MAXC;  // candidate clusters per frame (one lane each)
constexpr int TP_MAXD = 16;    // detections per frame read back

using vt::TailParams;

struct TailCluster
{
  uint32_t root, n_members;
  float obb_center[3];
  int32_t job;  // result slot of the cluster's explore job, or -1
};

struct DetRaw
{
  uint32_t root, n_points;
  float center[3];
  uint32_t pad;
  double conf_sum;
};

struct FrameDets
{
  uint32_t n;         // detections of the frame (cluster order)
  uint32_t fallback;  // a capacity was exceeded: the host tail must redo this batch
  int32_t status;     // FrameHdr::status
  uint32_t n_jobs;
  DetRaw d[TP_MAXD];
};

enum : uint32_t { TAIL_FB_MEMBERS = 1u, TAIL_FB_CLUSTERS = 2u, TAIL_FB_RADIUS = 4u, TAIL_FB_DETS = 8u, TAIL_FB_EXPLORE = 16u };

// a lane's place among the lanes of the wave that raise `flag` (cluster order = lane order), and how many do
__device__ __forceinline__ uint32_t rank_in_wave(bool flag, int lane, uint32_t& count)
{
  const unsigned long long m = __ballot(flag);
  count = __popcll(m);
  return __popcll(m & ((1ull << lane) - 1ull));
}

// the header of a frame's record slot, twice: to the workspace (device memory, read by the capacity fall-back) and, where the
// caller gave one, to the pinned host slot (one lane calls this)
__device__ __forceinline__ void put_header(FrameDets& out, FrameDets* hout, uint32_t f, uint32_t n, uint32_t fb, int32_t status, uint32_t n_jobs)
{
  out.n = n;
  out.fallback = fb;
  out.status = status;
  out.n_jobs = n_jobs;
  if (hout)
  {
    hout[f].n = n;
    hout[f].fallback = fb;
    hout[f].status = status;
    hout[f].n_jobs = n_jobs;
  }
}

// The floating clusters (extractDetections :843-846) of a frame as raw detection records in cluster order, lane c = cluster c
// of the canonical order.  Returns what the slot's header says of them: their number and the capacities they exceeded (the
// caller's lane 0 passes both on to put_header).
__device__ __forceinline__ void write_records(const TailCluster& tc, const vc::ExploreResult* __restrict__ results, int lane, FrameDets& out, FrameDets* hout, uint32_t f, uint32_t& n, uint32_t& fb)
{
  bool det = false, bad = false;
  double conf = 0.0;
  if (tc.job >= 0)
  {
    const vc::ExploreResult r = results[tc.job];
    det = r.floating != 0u;
    bad = r.overflow != 0u;
    conf = r.conf_sum;
  }
  const uint32_t pos = rank_in_wave(det, lane, n);
  const unsigned long long bm = __ballot(bad);
  if (det && pos < TP_MAXD)
  {
    DetRaw d;
    d.root = tc.root;
    d.n_points = tc.n_members;
    for (int q = 0; q < 3; q++)
      d.center[q] = tc.obb_center[q];
    d.pad = 0;
    d.conf_sum = conf;
    out.d[pos] = d;
    if (hout)
      hout[f].d[pos] = d;
  }
  fb = (n > TP_MAXD ? TAIL_FB_DETS : 0u) | (bm ? TAIL_FB_EXPLORE : 0u);
}

// One lane's cluster through vt::classify_gates; a cluster that reaches its flood fill fills in its explore job (all but the
// result slot) and stores its members' map voxels.  `get(i, p)` fetches the centre of the cluster's member i, m_begin is its
// first member's place among the frame's candidate members.
template <class Get>
__device__ __forceinline__ bool gate_cluster(uint32_t f, uint32_t m_begin, uint32_t m_count, Get get, const float* tf, const MapGeom& mg, const TailParams& tp, int* __restrict__ members_out, TailCluster& tc,
                                             vc::ExploreJob& job, uint32_t& fallback)
{
  const int s3[3] = {mg.sx, mg.sy, mg.sz};
  const vt::Gates gt = vt::classify_gates(m_count, get, tf, tp, mg.off, mg.vs_inv, s3);
  for (int q = 0; q < 3; q++)
    tc.obb_center[q] = gt.obb_center[q];
  if (!gt.explore)
    return false;
  job.frame = f;
  job.n_members = m_count;
  job.member_off = f * TP_MAXM + m_begin;
  job.R = gt.R;
  if (job.R > vc::EX_MAX_R || job.R < 0)
    fallback |= TAIL_FB_RADIUS;
  for (int q = 0; q < 3; q++)
  {
    job.box_lo[q] = gt.box_lo[q];
    job.box_hi[q] = gt.box_hi[q];
  }
  for (uint32_t i = 0; i < m_count; i++)
  {
    float p[3];
    get(i, p);
    int* o = members_out + 3 * static_cast<size_t>(job.member_off + i);
    for (int q = 0; q < 3; q++)
      o[q] = vt::map_cell(p[q], mg.off[q], mg.vs_inv);
  }
  return true;
}

__global__ __launch_bounds__(TP_THREADS) void k_tail_prep(const GridParams g, const FrameHdr* __restrict__ hdrs, const FrameArgs* __restrict__ args, const ClusterRec* __restrict__ table_all,
                                                         const CandMember* __restrict__ cand_all, VoxelArrays va_all, const MapGeom mg, const TailParams tp, vc::ExploreJob* __restrict__ jobs,
                                                         uint32_t* __restrict__ job_begin, uint32_t* __restrict__ job_end, int* __restrict__ members_out, TailCluster* __restrict__ tailc,
                                                         FrameDets* __restrict__ dets)
{
  __shared__ unsigned long long s_key[TP_MAXM];  // (cluster root << 32) | voxel rank, sorted ascending
  __shared__ ClusterRec s_rec[TP_MAXC];
  __shared__ uint32_t s_ord[TP_MAXC];
  __shared__ uint32_t s_nc;
  const uint32_t f = blockIdx.x;
  const FrameHdr h = hdrs[f];
  const int tid = threadIdx.x;
  FrameDets& out = dets[f];
  uint32_t fallback = 0;
  if (tid == 0)
  {
    s_nc = 0;
    job_begin[f] = f * TP_MAXC;
    job_end[f] = f * TP_MAXC;
  }
  __syncthreads();
  const uint32_t n_cand = h.status == VOFOD_OK ? h.n_cand : 0u;
  const uint32_t C = h.status == VOFOD_OK ? h.C : 0u;
  if (n_cand > TP_MAXM)
    fallback |= TAIL_FB_MEMBERS;
  // candidate clusters of the frame (any order in the table)
  const ClusterRec* table = table_all + static_cast<size_t>(f) * g.vox_cap;
  for (uint32_t c = tid; c < C; c += TP_THREADS)
  {
    const ClusterRec r = table[c];
    if (r.cand && !r.close)
    {
      const uint32_t pos = atomicAdd(&s_nc, 1u);
      if (pos < TP_MAXC)
        s_rec[pos] = r;
    }
  }
  // members: sort by (root, voxel rank)
  uint32_t np2 = 1;
  while (np2 < n_cand && np2 < TP_MAXM)
    np2 <<= 1;
  const CandMember* cands = cand_all + static_cast<size_t>(f) * g.vox_cap;
  if (!(fallback & TAIL_FB_MEMBERS))
    for (uint32_t i = tid; i < np2; i += TP_THREADS)
    {
      unsigned long long k = ~0ull;
      if (i < n_cand)
      {
        const CandMember cm = cands[i];
        k = (static_cast<unsigned long long>(cm.root) << 32) | cm.v;
      }
      s_key[i] = k;
    }
  __syncthreads();
  if (!(fallback & TAIL_FB_MEMBERS) && n_cand > 1)
    for (uint32_t k = 2; k <= np2; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1)
      {
        for (uint32_t i = tid; i < np2; i += TP_THREADS)
        {
          const uint32_t l = i ^ j;
          if (l > i)
          {
            const unsigned long long a = s_key[i], b = s_key[l];
            const bool up = (i & k) == 0;
            if ((a > b) == up)
            {
              s_key[i] = b;
              s_key[l] = a;
            }
          }
        }
        __syncthreads();
      }
  const uint32_t nc_all = s_nc;
  if (nc_all > TP_MAXC)
    fallback |= TAIL_FB_CLUSTERS;
  const uint32_t nc = fallback ? 0u : nc_all;
  // canonical order: size descending, smallest member (= root) ascending; rank by counting (<= 64 clusters)
  if (tid < static_cast<int>(nc))
  {
    const ClusterRec me = s_rec[tid];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < nc; j++)
    {
      const ClusterRec o = s_rec[j];
      rank += (o.size > me.size || (o.size == me.size && o.root < me.root)) ? 1u : 0u;
    }
    s_ord[rank] = tid;
  }
  __syncthreads();
  if (tid >= 64)
    return;  // one wave goes on: a lane per cluster, in canonical order
  const int lane = tid;
  bool live = lane < static_cast<int>(nc);
  const VoxelArrays va = frame_voxels(va_all, f, g.vox_cap);
  const FrameArgs& a = args[f];
  bool wants_job = false;
  vc::ExploreJob job{};
  TailCluster tc{};
  tc.job = -1;
  uint32_t m_begin = 0, m_count = 0;
  if (live)
  {
    const ClusterRec rec = s_rec[s_ord[lane]];
    tc.root = rec.root;
    // the cluster's members: the run of keys with this root
    uint32_t lo = 0, hi = n_cand;
    const unsigned long long want = static_cast<unsigned long long>(rec.root) << 32;
    while (lo < hi)
    {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_key[mid] < want)
        lo = mid + 1;
      else
        hi = mid;
    }
    m_begin = lo;
    while (m_begin + m_count < n_cand && static_cast<uint32_t>(s_key[m_begin + m_count] >> 32) == rec.root)
      m_count++;
    tc.n_members = m_count;
    auto get = [&](size_t i, float p[3]) {
      const float4 q = va.pts[static_cast<uint32_t>(s_key[m_begin + i])];
      p[0] = q.x;
      p[1] = q.y;
      p[2] = q.z;
    };
    wants_job = gate_cluster(f, m_begin, m_count, get, a.tf, mg, tp, members_out, tc, job, fallback);
  }
  // jobs in cluster order
  uint32_t n_jobs;
  const uint32_t slot = f * TP_MAXC + rank_in_wave(wants_job, lane, n_jobs);
  if (wants_job)
  {
    job.result_slot = slot;
    jobs[slot] = job;
    tc.job = static_cast<int32_t>(slot);
  }
  uint32_t fb_all = fallback;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1)
    fb_all |= __shfl_xor(fb_all, s);
  if (live)
    tailc[f * TP_MAXC + lane] = tc;
  if (lane == 0)
  {
    put_header(out, nullptr, f, 0u, fb_all, h.status, fb_all ? 0u : n_jobs);
    if (!fb_all)
      job_end[f] = f * TP_MAXC + n_jobs;
  }
  if (!live && lane < TP_MAXC)  // clusters past nc are marked empty for k_tail_finish
  {
    TailCluster e{};
    e.job = -1;
    tailc[f * TP_MAXC + lane] = e;
  }
}

// ---- the whole tail of a close-first frame in one kernel, one wave per frame, 256 bytes of LDS (round 4) --------------------------
// k_frame_lds_far leaves the candidate clusters at the head of the frame's cluster table in the canonical order and their
// members cluster by cluster with ascending rank: no sorting here, hence no LDS to speak of - the wave fits a CU beside a frame
// workgroup of the next batch (k_tail_prep's 11 KB had to wait for a CU to come free: 50 us alone, 150-200 us in company, and
// the three tail kernels of a batch, one after the other on the tail stream, had become the pace of the pipeline).
// Lane c = candidate cluster c: boxes + gates + explore job as k_tail_prep; then the wave runs the frame's flood fills
// (explore_frame: the code of k_explore) and writes the detection records as k_tail_finish.
// Round 5: TAIL_WPB waves (frames) per workgroup.  With one wave per workgroup the 256 tails of a batch were dealt out one by one,
// each to the next CU a frame workgroup had just left - and a CU that holds even one such wave has no room for the next frame
// workgroup (4 x 128 registers on every SIMD): the tails kept ~15 % of the CUs away from the frame kernels (967 k frames/s without
// the tail kernel, 819 k with it).  Whole workgroups of tails fill a few CUs instead.
// (five waves per SIMD = at most 96 registers: one of this kernel's waves then fits beside the four 104-register waves a frame
// workgroup keeps on every SIMD - 4 x 104 + 96 = 512 - instead of waiting for a CU without one)
__global__ TAIL_OCC_ATTR __launch_bounds__(64 * TAIL_WPB) void k_tail_far(const GridParams g, const FrameHdr* __restrict__ hdrs, const FrameArgs* __restrict__ args, const ClusterRec* __restrict__ table_all,
                                                const CandMember* __restrict__ cand_all, VoxelArrays va_all, const MapGeom mg, const TailParams tp, const vc::ExploreParams ep, vc::ExploreJob* __restrict__ jobs,
                                                int* __restrict__ members_out, float* __restrict__ map, unsigned long long* __restrict__ overlay_all, uint32_t* __restrict__ stack_all,
                                                uint32_t* __restrict__ explored_all, uint32_t* __restrict__ touched_all, uint32_t* __restrict__ ovl_list_all, uint32_t* __restrict__ ovl_count_all,
                                                vc::ExploreResult* __restrict__ results, uint32_t* __restrict__ visited_all, FrameDets* __restrict__ dets, FrameDets* __restrict__ hout,
                                                TailCluster* __restrict__ tailc, unsigned long long* __restrict__ prof)
{
  __shared__ uint8_t s_float_all[TAIL_WPB][TP_MAXC];
  __shared__ uint8_t s_walk_all[TAIL_WPB][6 * 32];
  __shared__ float s_pts_all[TAIL_WPB][TAIL_STAGE][3];
  const uint32_t f = blockIdx.x * TAIL_WPB + (threadIdx.x >> 6);  // one wave per frame, TAIL_WPB frames per workgroup
  if (f >= g.n_frames)
    return;
  uint8_t* s_float = s_float_all[threadIdx.x >> 6];
  uint8_t* s_walk = s_walk_all[threadIdx.x >> 6];
  const FrameHdr h = hdrs[f];
  const int lane = threadIdx.x & 63;
  // (diagnostics, VOFOD_LDS_PROF=2: slots 22 / 23 of the frame's stamps - start, then boxes | explore | end as 20-bit offsets in 10 ns)
  const unsigned long long tp0 = prof ? wall_clock64() : 0ull;
  unsigned long long tp1 = 0ull, tp2 = 0ull;
  FrameDets& out = dets[f];
  uint32_t fallback = 0;
  const bool ok = h.status == VOFOD_OK;
  const uint32_t n_cand = ok ? h.n_cand : 0u;
  const uint32_t nc_all = ok ? h.n_cand_clusters : 0u;
  if (n_cand > static_cast<uint32_t>(TP_MAXM))
    fallback |= TAIL_FB_MEMBERS;
  if (nc_all > static_cast<uint32_t>(TP_MAXC))
    fallback |= TAIL_FB_CLUSTERS;
  const uint32_t nc = fallback ? 0u : nc_all;
  const bool live = lane < static_cast<int>(nc);
  const ClusterRec* table = table_all + static_cast<size_t>(f) * g.vox_cap;
  const CandMember* cands = cand_all + static_cast<size_t>(f) * g.vox_cap;
  const VoxelArrays va = frame_voxels(va_all, f, g.vox_cap);
  const FrameArgs& a = args[f];
  ClusterRec rec{};
  if (live)
    rec = table[lane];
  // the cluster's members: the run behind those of the clusters in front (a candidate's members are all its voxels)
  uint32_t m_count = live ? rec.size : 0u, m_begin = 0;
  {
    uint32_t incl = m_count;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1)
    {
      const uint32_t t = __shfl_up(incl, s);
      if (lane >= s)
        incl += t;
    }
    m_begin = incl - m_count;
  }
  // Round 5: the candidates' member centres are fetched ONCE, by all 64 lanes together, into the wave's own LDS; boxes_of_n walks
  // a cluster's members three times (mean, covariance, OBB extents), one lane per cluster, and every visit was two dependent
  // global loads (member list -> voxel record): ~34 us per frame of nothing but latency.  Members beyond the staging area (a
  // frame with more than TAIL_STAGE candidate members) are read from global memory as before - same values either way.
  float (*s_pts)[3] = s_pts_all[threadIdx.x >> 6];
  {
    const uint32_t total = min(static_cast<uint32_t>(__shfl(m_begin + m_count, 63)), static_cast<uint32_t>(TAIL_STAGE));
    for (uint32_t i = lane; i < total; i += 64)
    {
      const float4 q = va.pts[cands[i].v];
      s_pts[i][0] = q.x;
      s_pts[i][1] = q.y;
      s_pts[i][2] = q.z;
    }
    vc::wave_sync();
  }
  bool wants_job = false;
  vc::ExploreJob job{};
  TailCluster tc{};
  tc.job = -1;
  if (live)
  {
    tc.root = rec.root;
    tc.n_members = m_count;
    auto get = [&](size_t i, float p[3]) {
      const uint32_t k = m_begin + static_cast<uint32_t>(i);
      if (k < static_cast<uint32_t>(TAIL_STAGE))
      {
        p[0] = s_pts[k][0];
        p[1] = s_pts[k][1];
        p[2] = s_pts[k][2];
        return;
      }
      const float4 q = va.pts[cands[k].v];
      p[0] = q.x;
      p[1] = q.y;
      p[2] = q.z;
    };
    wants_job = gate_cluster(f, m_begin, m_count, get, a.tf, mg, tp, members_out, tc, job, fallback);
  }
  // jobs in cluster order
  uint32_t n_jobs;
  const uint32_t jb = f * TP_MAXC;
  const uint32_t slot = jb + rank_in_wave(wants_job, lane, n_jobs);
  if (wants_job)
  {
    job.result_slot = slot;
    jobs[slot] = job;
    tc.job = static_cast<int32_t>(slot);
  }
  if (tailc)  // (a map-updating scan: the host rebuilds the detections from these when the record slots overflow)
  {
    if (!live)
    {
      tc = TailCluster{};
      tc.job = -1;
    }
    tailc[f * TP_MAXC + lane] = tc;
  }
  uint32_t fb_all = fallback;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1)
    fb_all |= __shfl_xor(fb_all, s);
  if (fb_all)
  {
    if (lane == 0)
      put_header(out, hout, f, 0u, fb_all, h.status, 0u);
    return;
  }
  __threadfence_block();
  vc::wave_sync();  // the jobs and their members' map voxels are written: the wave reads them back
  if (prof)
    tp1 = wall_clock64();
  vc::explore_frame(ep, mg, jobs, jb, jb + n_jobs, members_out, map, overlay_all, stack_all, explored_all, touched_all, ovl_list_all, ovl_count_all, results, visited_all, f, s_float, s_walk);
  __threadfence_block();
  vc::wave_sync();
  if (prof)
    tp2 = wall_clock64();
  uint32_t n, fb;
  write_records(tc, results, lane, out, hout, f, n, fb);
  if (lane == 0)
  {
    put_header(out, hout, f, n, fb, h.status, n_jobs);
    if (prof)
    {
      const unsigned long long te = wall_clock64();
      auto d20 = [&](unsigned long long t) { return (t - tp0) > 0xfffffull ? 0xfffffull : (t - tp0); };
      prof[static_cast<size_t>(f) * 32 + 22] = tp0;
      prof[static_cast<size_t>(f) * 32 + 23] = d20(tp1) | (d20(tp2) << 20) | (d20(te) << 40) | (static_cast<unsigned long long>(n_jobs > 15u ? 15u : n_jobs) << 60);
    }
  }
}

// one wave per frame: the floating clusters (extractDetections :843-846) in cluster order.  The frame's record is written
// twice: to the workspace (device memory, read by the capacity fall-back) and straight into the caller-visible pinned host
// slot `hout` (135 KB per 256 frames over PCIe).  No copy command follows the tail: a D2H hipMemcpyAsync queued behind kernels
// occupies an SDMA engine while it waits, the runtime then brings up a further engine for the next batch's copy, and each
// first use of an engine blocked vofod_batch_submit for 6-7 ms (three times within the first twenty batches of a process).
__global__ __launch_bounds__(64) void k_tail_finish(const TailCluster* __restrict__ tailc, const vc::ExploreResult* __restrict__ results, FrameDets* __restrict__ dets, FrameDets* __restrict__ hout)
{
  const uint32_t f = blockIdx.x;
  const int lane = threadIdx.x;
  FrameDets& out = dets[f];
  const uint32_t fb_in = out.fallback;
  if (fb_in)
  {
    if (lane == 0)
      put_header(out, hout, f, 0u, fb_in, out.status, out.n_jobs);
    return;
  }
  const TailCluster tc = tailc[f * TP_MAXC + lane];
  uint32_t n, fb;
  write_records(tc, results, lane, out, hout, f, n, fb);
  if (lane == 0)
    put_header(out, hout, f, n, fb, out.status, out.n_jobs);
}

}  // namespace vtd
