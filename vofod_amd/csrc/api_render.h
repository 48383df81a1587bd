// vofod_map_render (included by vofod_hip.hip after api_maps.h): the voxel map rendered through the handle's LUT from a list of
// poses.  Contract: include/vofod.h, MAP RENDER; kernel and the account of its bursts: map_render.h.
#pragma once

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
  // the rule vofod_raycast_begin applies to its one tf, for every view, before anything is queued
  for (size_t v = 0; v < n_views; v++)
  {
    const float origin[3] = {tfs[12 * v + 3], tfs[12 * v + 7], tfs[12 * v + 11]};
    int o[3];
    h->hg.coordToIdx(origin, o);
    if (!h->hg.inLimits(o))
    {
      h->err = "map render: the origin of view " + std::to_string(v) + " lies outside the map";
      return VOFOD_ERR_SENSOR_OUTSIDE_MAP;
    }
  }
  const uint32_t n = static_cast<uint32_t>(h->sp.sensor_hrays) * static_cast<uint32_t>(h->sp.sensor_vrays);
  const size_t total = n_views * static_cast<size_t>(n);
  vmr::Workspace& w = h->render;
  HIPCHK(w.d_poses.reserve(n_views * 12));
  vmr::RenderOut out{range, voxel, what, reinterpret_cast<float2*>(t_in_out)};
  if (!on_device)
  {
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
  }
  HIPCHK(hipMemcpyAsync(w.d_poses, tfs, n_views * 12 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  const vmr::RenderParams rp{threshold, max_distance, n};
  const dim3 grid((n + vmr::MR_THREADS - 1) / vmr::MR_THREADS, static_cast<uint32_t>(n_views)), block(vmr::MR_THREADS);
  // VOFOD_RENDER_BURST (diagnostics, tools/map_render_bench.py): the burst lengths measured beside the one kept
  int burst = vmr::MR_BURST;
  if (const char* e = std::getenv("VOFOD_RENDER_BURST"))
    burst = std::atoi(e);
  auto kern = burst == 1 ? vmr::k_map_render<1> : burst == 2 ? vmr::k_map_render<2> : burst == 8 ? vmr::k_map_render<8> : burst == 4 ? vmr::k_map_render<4> : vmr::k_map_render<vmr::MR_BURST>;
  KLAUNCH_AS(h, "k_map_render", kern, grid, block, rp, h->mg, static_cast<const float*>(h->d_map.p), static_cast<const float*>(h->d_lut_dirs.p), static_cast<const float*>(h->d_lut_offs.p),
             static_cast<const float*>(w.d_poses.p), out);
  HIPCHK(hipGetLastError());
  if (!on_device)
  {
    if (range)
      HIPCHK(hipMemcpyAsync(range, w.d_range, total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (voxel)
      HIPCHK(hipMemcpyAsync(voxel, w.d_voxel, total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (what)
      HIPCHK(hipMemcpyAsync(what, w.d_what, total, hipMemcpyDeviceToHost, h->stream));
    if (t_in_out)
      HIPCHK(hipMemcpyAsync(t_in_out, w.d_tio, total * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));  // (the call's only one: host outputs arrive with it)
  return VOFOD_OK;
}

}  // extern "C"
