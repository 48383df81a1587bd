// vofod_map_match (included by vofod_hip.hip after api_render.h): the classes of one scan's returns under a list of candidate poses,
// counted on the device by one map look-up per return and pose.  Contract: include/vofod.h, MAP MATCH; kernels and the account of
// their three launches: map_match.h.
#pragma once

#include "api_query.h"

namespace
{

// the refusals that the scan and the candidate list decide (include/vofod.h, MAP MATCH), before the lock: shared by vofod_map_match
// and vofod_map_match_field (api_distance.h)
inline int match_refusal(const vofod_handle* h, const vofod_scan* scan, const float* tfs, size_t n_poses, const uint32_t* counts)
{
  if (!h || !scan || !tfs || !counts || n_poses == 0 || n_poses > vmm::MM_MAX_POSES)
    return VOFOD_ERR_INVALID_ARG;
  const vofod_scan& s = *scan;
  if (s.memspace != VOFOD_MEM_HOST && s.memspace != VOFOD_MEM_DEVICE)
    return VOFOD_ERR_INVALID_ARG;
  const int n_null = !s.x + !s.y + !s.z;
  if (n_null == 1 || n_null == 2 || (n_null == 3 && !s.range))
    return VOFOD_ERR_INVALID_ARG;
  const bool is_range = n_null == 3, dev = s.memspace == VOFOD_MEM_DEVICE;
  if (!is_range && s.col_tfs)
    return VOFOD_ERR_INVALID_ARG;  // (whatever vofod_set_point_motion says: the call has no deskew step)
  if (dev)
  {
    const uintptr_t cols = is_range ? reinterpret_cast<uintptr_t>(s.range) : reinterpret_cast<uintptr_t>(s.x) | reinterpret_cast<uintptr_t>(s.y) | reinterpret_cast<uintptr_t>(s.z);
    if (((cols | s.stride_bytes) & 3) || (reinterpret_cast<uintptr_t>(s.col_tfs) & 3))
      return VOFOD_ERR_INVALID_ARG;
  }
  if (s.height != h->sp.sensor_vrays || s.width != h->sp.sensor_hrays)
    return VOFOD_ERR_SIZE_MISMATCH;
  return VOFOD_OK;
}

// the live list of a scan that passed match_refusal, under the lock: device-resident columns and tables are read in place, host-resident
// ones are staged; the candidates go to w.d_poses, n_live and every candidate's slots (w.d_out) are cleared on the
// stream, and k_match_points fills w.d_points
inline int match_live_list(vofod_handle* h, vmm::Workspace& w, const vofod_scan& s, const float* tfs, size_t n_poses)
{
  const int n_null = !s.x + !s.y + !s.z;
  const bool is_range = n_null == 3;
  const uint32_t width = static_cast<uint32_t>(h->sp.sensor_hrays);
  const uint32_t n = width * static_cast<uint32_t>(h->sp.sensor_vrays);
  const size_t n_out = vmm::MM_HEAD + 4 * n_poses;
  HIPCHK(w.d_points.reserve(n));
  HIPCHK(w.d_poses.reserve(n_poses * 12));
  HIPCHK(w.d_out.reserve(n_out));
  // ---- the scan: device-resident columns and tables are read in place, host-resident ones are staged (stage_scans, api_query.h)
  VCHK(stage_scans(h, &s, 1, vss::WANT_TABLES | (is_range ? vss::WANT_RANGE : vss::WANT_POINTS)));
  const vmm::ScanSource& src = h->qstage.at[0];
  HIPCHK(hipMemcpyAsync(w.d_poses, tfs, n_poses * 12 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(w.d_out, 0, n_out * sizeof(uint32_t), h->stream));  // n_live and every candidate's slots
  vrd::MotionArgs ma{};
  ma.shift = h->d_col_shift.p;
  ma.width = width;
  exclude_box(h, ma.lo, ma.hi);
  const bool pose16 = (reinterpret_cast<uintptr_t>(src.poses) & 15) == 0;
  auto points = !is_range ? vmm::k_match_points<vmm::SRC_POINTS, true>
                : !src.poses ? vmm::k_match_points<vmm::SRC_RANGE, true>
                : pose16     ? vmm::k_match_points<vmm::SRC_MOTION, true>
                             : vmm::k_match_points<vmm::SRC_MOTION, false>;
  KLAUNCH_AS(h, "k_match_points", points, dim3((n + 255) / 256), dim3(256), src, n, static_cast<const float*>(h->d_lut_dirs.p), static_cast<const float*>(h->d_lut_offs.p), ma, w.d_points.p,
             w.d_out.p);
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// the occupancy image of `threshold` in h->match.d_bits (k_match_bits): vofod_map_match scores by it, vofod_map_distance starts from it
inline int match_bits(vofod_handle* h, float threshold)
{
  vmm::Workspace& w = h->match;
  HIPCHK(w.d_bits.reserve((h->mg.n + 63) / 64));
  KLAUNCH_AS(h, "k_match_bits", vmm::k_match_bits, dim3(static_cast<uint32_t>((h->mg.n + 255) / 256)), dim3(256), static_cast<const float*>(h->d_map.p), h->mg.n, threshold, w.d_bits.p);
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// the scoring walk over the live list of match_live_list, by either policy, under its profiler label, and what it leaves: the launch
// is sized for width * height, the blocks beyond n_live leave at once (a chunk below n / 65535 is raised to it: gridDim.y); chunk and
// burst are read per call.  n_live and the counts arrive in h->match.h_out - and the field's sums in h->dist.h_cost - with the call's
// only synchronisation, behind which the staged inputs are free.
template <class Look>
inline int match_score(vofod_handle* h, const char* label, const Look& look, size_t n_poses)
{
  vmm::Workspace& w = h->match;
  const uint32_t n = static_cast<uint32_t>(h->sp.sensor_hrays) * static_cast<uint32_t>(h->sp.sensor_vrays), np = static_cast<uint32_t>(n_poses);
  const size_t n_out = vmm::MM_HEAD + 4 * n_poses;
  const uint32_t chunk = std::max(env_int("VOFOD_MATCH_CHUNK", vmm::MM_CHUNK), (n + vmm::MM_MAX_CHUNKS - 1) / vmm::MM_MAX_CHUNKS);
  const vmm::ScoreParams sp{np, chunk, static_cast<float>(h->mg.sx), static_cast<float>(h->mg.sy), static_cast<float>(h->mg.sz)};
  const dim3 grid((np + vmm::MM_THREADS - 1) / vmm::MM_THREADS, (n + chunk - 1) / chunk), block(vmm::MM_THREADS);
  with_burst<vmm::MM_BURST>(env_int("VOFOD_MATCH_BURST", vmm::MM_BURST), [&](auto U) {
    auto kern = vmm::k_match<decltype(U)::value, Look>;
    KLAUNCH_AS(h, label, kern, grid, block, sp, h->mg, look, static_cast<const float4*>(w.d_points.p), static_cast<const float*>(w.d_poses.p), w.d_out.p);
  });
  HIPCHK(hipGetLastError());
  w.h_out.resize(n_out);
  HIPCHK(hipMemcpyAsync(w.h_out.data(), w.d_out, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if constexpr (std::is_same_v<Look, vmm::LookField>)
  {
    h->dist.h_cost.resize(n_poses);
    HIPCHK(hipMemcpyAsync(h->dist.h_cost.data(), look.cost, n_poses * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return VOFOD_OK;
}

}  // namespace

extern "C" {

int vofod_map_match(vofod_handle* h, const vofod_scan* scan, const float* tfs, size_t n_poses, float threshold, uint32_t* counts, int32_t* best)
{
  if (std::isnan(threshold))
    return VOFOD_ERR_INVALID_ARG;
  VCHK(match_refusal(h, scan, tfs, n_poses, counts));
  const vofod_scan& s = *scan;
  ApiLock lock(h);
  // as vofod_map_render: the voxel map is read, nothing is written but this call's own workspace (host inputs are staged THERE, not
  // in a ticket's workspace), so it is admitted with tickets in flight and with a raycast or sepclusters pass pending
  VCHK(admit(h, NEEDS_NOTHING));
  const uint32_t n = static_cast<uint32_t>(h->sp.sensor_hrays) * static_cast<uint32_t>(h->sp.sensor_vrays);
  const uint32_t np = static_cast<uint32_t>(n_poses);
  vmm::Workspace& w = h->match;
  VCHK(match_bits(h, threshold));
  VCHK(match_live_list(h, w, s, tfs, n_poses));
  VCHK(match_score(h, "k_match_score", vmm::LookBits{reinterpret_cast<const uint32_t*>(w.d_bits.p)}, n_poses));
  const uint32_t skipped = n - w.h_out[0];
  uint32_t best_occ = 0;
  int32_t best_k = 0;
  for (uint32_t k = 0; k < np; k++)
  {
    const uint32_t* c = w.h_out.data() + vmm::MM_HEAD + 4 * static_cast<size_t>(k);
    counts[4 * static_cast<size_t>(k)] = skipped;  // VOFOD_MATCH_SKIPPED: the same for every candidate
    for (int a = 1; a < 4; a++)
      counts[4 * static_cast<size_t>(k) + a] = c[a];
    if (c[3] > best_occ)
      best_occ = c[3], best_k = static_cast<int32_t>(k);
  }
  if (best)
    *best = best_k;
  return VOFOD_OK;
}

}  // extern "C"
