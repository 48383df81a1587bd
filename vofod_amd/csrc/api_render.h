// vofod_map_render and vofod_map_render_scans (included by vofod_hip.hip after api_maps.h): the voxel map rendered through the
// handle's LUT from a list of poses, or from a list of scans - a pose per column where a scan carries one - with the verdict of every
// measured return.  Contracts: include/vofod.h, MAP RENDER and SCANS AGAINST THE MAP; kernel and the account of its bursts: map_render.h.
#pragma once

#include "api_query.h"

namespace
{

// The four render outputs as the kernel writes them: the caller's own device arrays, or - for host outputs - the workspace's
// staging, which render_outputs_to_host copies out behind the launch.  Shared by the two entries.
inline int render_outputs(vofod_handle* h, vmr::Workspace& w, bool on_device, size_t total, uint32_t* range, uint32_t* voxel, uint8_t* what, float* t_in_out, vmr::RenderOut& out)
{
  out = vmr::RenderOut{range, voxel, what, reinterpret_cast<float2*>(t_in_out)};
  if (on_device)
    return VOFOD_OK;
  // host outputs: the kernel writes the workspace, the copies follow it on the stream
  if (range)
    HIPCHK(w.d_range.reserve(total));
  if (voxel)
    HIPCHK(w.d_voxel.reserve(total));
  if (what)
    HIPCHK(w.d_what.reserve(total));
  if (t_in_out)
    HIPCHK(w.d_tio.reserve(total));
  out = vmr::RenderOut{range ? w.d_range.p : nullptr, voxel ? w.d_voxel.p : nullptr, what ? w.d_what.p : nullptr, t_in_out ? w.d_tio.p : nullptr};
  return VOFOD_OK;
}

inline int render_outputs_to_host(vofod_handle* h, vmr::Workspace& w, size_t total, uint32_t* range, uint32_t* voxel, uint8_t* what, float* t_in_out)
{
  if (range)
    HIPCHK(hipMemcpyAsync(range, w.d_range, total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if (voxel)
    HIPCHK(hipMemcpyAsync(voxel, w.d_voxel, total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if (what)
    HIPCHK(hipMemcpyAsync(what, w.d_what, total, hipMemcpyDeviceToHost, h->stream));
  if (t_in_out)
    HIPCHK(hipMemcpyAsync(t_in_out, w.d_tio, total * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
  return VOFOD_OK;
}

// the rule vofod_raycast_begin applies to its one tf, for every view, before anything is queued
inline int render_origins_inside(vofod_handle* h, const float* tfs, size_t n_views, const char* who)
{
  for (size_t v = 0; v < n_views; v++)
  {
    const float origin[3] = {tfs[12 * v + 3], tfs[12 * v + 7], tfs[12 * v + 11]};
    int o[3];
    h->hg.coordToIdx(origin, o);
    if (!h->hg.inLimits(o))
    {
      h->err = std::string(who) + ": the origin of view " + std::to_string(v) + " lies outside the map";
      return VOFOD_ERR_SENSOR_OUTSIDE_MAP;
    }
  }
  return VOFOD_OK;
}

}  // namespace

extern "C" {

int vofod_map_render(vofod_handle* h, const float* tfs, size_t n_views, float threshold, float max_distance, uint32_t* range, uint32_t* voxel, uint8_t* what, float* t_in_out,
                     int32_t out_memspace)
{
  if (!h || !tfs || n_views == 0 || n_views > vmr::MR_MAX_VIEWS || (!range && !voxel && !what && !t_in_out) || !(max_distance > 0.0f) || std::isnan(threshold) ||
      (out_memspace != VOFOD_MEM_HOST && out_memspace != VOFOD_MEM_DEVICE))
    return VOFOD_ERR_INVALID_ARG;
  const bool on_device = out_memspace == VOFOD_MEM_DEVICE;
  if (on_device && (((reinterpret_cast<uintptr_t>(range) | reinterpret_cast<uintptr_t>(voxel)) & 3) || (reinterpret_cast<uintptr_t>(t_in_out) & 7)))
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  // reads the voxel map only, in a workspace of its own: admitted with tickets in flight and with a raycast or sepclusters pass pending
  VCHK(admit(h, NEEDS_NOTHING));
  VCHK(render_origins_inside(h, tfs, n_views, "map render"));
  const uint32_t n = static_cast<uint32_t>(h->sp.sensor_hrays) * static_cast<uint32_t>(h->sp.sensor_vrays);
  const size_t total = n_views * static_cast<size_t>(n);
  vmr::Workspace& w = h->render;
  HIPCHK(w.d_poses.reserve(n_views * 12));
  vmr::RenderOut out{};
  VCHK(render_outputs(h, w, on_device, total, range, voxel, what, t_in_out, out));
  HIPCHK(hipMemcpyAsync(w.d_poses, tfs, n_views * 12 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  const vmr::RenderParams rp{threshold, max_distance, n};
  const dim3 grid((n + vmr::MR_THREADS - 1) / vmr::MR_THREADS, static_cast<uint32_t>(n_views)), block(vmr::MR_THREADS);
  with_burst<vmr::MR_BURST>(env_int("VOFOD_RENDER_BURST", vmr::MR_BURST), [&](auto K) {
    auto kern = vmr::k_map_render<decltype(K)::value>;
    KLAUNCH_AS(h, "k_map_render", kern, grid, block, rp, h->mg, static_cast<const float*>(h->d_map.p), static_cast<const float*>(h->d_lut_dirs.p),
               static_cast<const float*>(h->d_lut_offs.p), static_cast<const float*>(w.d_poses.p), out);
  });
  HIPCHK(hipGetLastError());
  if (!on_device)
    VCHK(render_outputs_to_host(h, w, total, range, voxel, what, t_in_out));
  HIPCHK(hipStreamSynchronize(h->stream));  // (the call's only one: host outputs arrive with it)
  return VOFOD_OK;
}

int vofod_map_render_scans(vofod_handle* h, const vofod_scan* scans, const float* tfs, size_t n_scans, float threshold, float max_distance, float tolerance, uint32_t* range,
                           uint32_t* voxel, uint8_t* what, float* t_in_out, uint8_t* verdict, uint32_t* counts, int32_t out_memspace)
{
  if (!h || !scans || !tfs || n_scans == 0 || n_scans > vmr::MR_MAX_VIEWS || (!range && !voxel && !what && !t_in_out && !verdict && !counts) || !(max_distance > 0.0f) ||
      std::isnan(threshold) || !(tolerance >= 0.0f) || (out_memspace != VOFOD_MEM_HOST && out_memspace != VOFOD_MEM_DEVICE))
    return VOFOD_ERR_INVALID_ARG;
  const bool on_device = out_memspace == VOFOD_MEM_DEVICE;
  if (on_device && (((reinterpret_cast<uintptr_t>(range) | reinterpret_cast<uintptr_t>(voxel)) & 3) || (reinterpret_cast<uintptr_t>(t_in_out) & 7)))
    return VOFOD_ERR_INVALID_ARG;
  const bool compare = verdict || counts;  // the scans' ranges are read
  for (size_t v = 0; v < n_scans; v++)
  {
    const vofod_scan& s = scans[v];
    if (s.memspace != VOFOD_MEM_HOST && s.memspace != VOFOD_MEM_DEVICE)
      return VOFOD_ERR_INVALID_ARG;
    const bool dev = s.memspace == VOFOD_MEM_DEVICE;
    if (compare && !s.range)
      return VOFOD_ERR_INVALID_ARG;
    if (compare && dev && ((reinterpret_cast<uintptr_t>(s.range) | s.stride_bytes) & 3))
      return VOFOD_ERR_INVALID_ARG;
    if (dev && (reinterpret_cast<uintptr_t>(s.col_tfs) & 3))
      return VOFOD_ERR_INVALID_ARG;
  }
  for (size_t v = 0; v < n_scans; v++)
    if (scans[v].height != h->sp.sensor_vrays || scans[v].width != h->sp.sensor_hrays)
      return VOFOD_ERR_SIZE_MISMATCH;
  ApiLock lock(h);
  // as vofod_map_render: the voxel map is read, nothing is written but this call's own workspace (host tables and ranges are staged
  // THERE, not in a ticket's workspace), so it is admitted with tickets in flight and with a raycast or sepclusters pass pending
  VCHK(admit(h, NEEDS_NOTHING));
  VCHK(render_origins_inside(h, tfs, n_scans, "map render scans"));
  const uint32_t width = static_cast<uint32_t>(h->sp.sensor_hrays);
  const uint32_t n = width * static_cast<uint32_t>(h->sp.sensor_vrays);
  const size_t total = n_scans * static_cast<size_t>(n);
  vmr::Workspace& w = h->render;
  vmr::RenderOut out{};
  VCHK(render_outputs(h, w, on_device, total, range, voxel, what, t_in_out, out));
  HIPCHK(w.d_views.reserve(n_scans));
  uint8_t* d_verdict = verdict;
  if (verdict && !on_device)
  {
    HIPCHK(w.d_verdict.reserve(total));
    d_verdict = w.d_verdict.p;
  }
  if (counts)
    HIPCHK(w.d_counts.reserve(n_scans * 8));
  // the host scans' tables and, where they are compared, their range columns; then the view table
  VCHK(stage_scans(h, scans, n_scans, vss::WANT_TABLES | (compare ? vss::WANT_RANGE : 0u)));
  w.h_views.resize(n_scans);
  for (size_t v = 0; v < n_scans; v++)
  {
    const vss::Staged& e = h->qstage.at[v];
    w.h_views[v] = vmr::ViewEntry{{}, e.poses, e.range, e.range ? e.stride : 4};  // (no range to compare: the stride is not read, and is 4 as it was)
    std::memcpy(w.h_views[v].tf, tfs + 12 * v, sizeof(w.h_views[v].tf));
  }
  HIPCHK(hipMemcpyAsync(w.d_views, w.h_views.data(), n_scans * sizeof(vmr::ViewEntry), hipMemcpyHostToDevice, h->stream));
  if (counts)
    HIPCHK(hipMemsetAsync(w.d_counts, 0, n_scans * 8 * sizeof(uint32_t), h->stream));
  const vmr::RenderParams rp{threshold, max_distance, n};
  const vmr::ScanViews views{w.d_views.p, h->d_col_shift.p, h->d_mask.p, width, tolerance, d_verdict, counts ? w.d_counts.p : nullptr};
  const dim3 grid((n + vmr::MR_THREADS - 1) / vmr::MR_THREADS, static_cast<uint32_t>(n_scans)), block(vmr::MR_THREADS);
  with_burst<vmr::MR_BURST>(env_int("VOFOD_RENDER_BURST", vmr::MR_BURST), [&](auto K) {
    auto kern = vmr::k_map_render<decltype(K)::value, vmr::ScanViews>;
    KLAUNCH_AS(h, "k_map_render_scans", kern, grid, block, rp, h->mg, static_cast<const float*>(h->d_map.p), static_cast<const float*>(h->d_lut_dirs.p),
               static_cast<const float*>(h->d_lut_offs.p), views, out);
  });
  HIPCHK(hipGetLastError());
  if (!on_device)
    VCHK(render_outputs_to_host(h, w, total, range, voxel, what, t_in_out));
  if (verdict && !on_device)
    HIPCHK(hipMemcpyAsync(verdict, w.d_verdict, total, hipMemcpyDeviceToHost, h->stream));
  if (counts)
    HIPCHK(hipMemcpyAsync(counts, w.d_counts, n_scans * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // (the call's only one: host outputs arrive with it, and the staged inputs are free)
  return VOFOD_OK;
}

}  // extern "C"
