// The other roles of the driver (included by vofod_hip.hip behind api_gate.h): the implementations of raycast, sepclusters and the
// stateless L4 helpers, and their part of the extern "C" surface of include/vofod.h - create, destroy, reset, status and
// parameters, the raycast, sepclusters, voxel-grid and cluster entries, the profiler.  The entries of the maps are in api_maps.h,
// those of scans and batches in api_frames.h, those that need no handle in api_host.h.
#pragma once

namespace
{

int gscan(vofod_handle* h, const uint32_t* d_in, uint32_t n, uint32_t* d_out, uint32_t* d_bsum, uint32_t* d_total)
{
  const uint32_t nblk = (n + vr::GS_EPB - 1) / vr::GS_EPB;
  if (n == 0)
  {
    HIPCHK(hipMemsetAsync(d_out, 0, sizeof(uint32_t), h->stream));
    if (d_total)
      HIPCHK(hipMemsetAsync(d_total, 0, sizeof(uint32_t), h->stream));
    return VOFOD_OK;
  }
  KLAUNCH(h, vr::k_gscan_a, dim3(nblk), dim3(256), d_in, n, d_bsum);
  KLAUNCH(h, vr::k_gscan_b, dim3(1), dim3(1024), d_bsum, nblk, d_total);
  KLAUNCH(h, vr::k_gscan_c, dim3(nblk), dim3(256), d_in, n, d_bsum, d_out);
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

int sep_ensure_words(vofod_handle* h, size_t n_words)
{
  vr::SepState& s = h->sep;
  auto& o = h->sep_own;
  if (!o.d_offsets)  // (the last of the three: it stands for all of them)
  {
    HIPCHK(alloc_view(o.d_small, s.d_small, 16));
    HIPCHK(o.h_small.alloc(16));
    s.h_small = o.h_small;
    HIPCHK(alloc_view(o.d_offsets, s.d_offsets, 3 * (2 * MAX_R + 1) * (2 * MAX_R + 1) * (2 * MAX_R + 1)));
  }
  if (n_words + 2 <= o.d_tprefix.n)  // (the last of the three again)
    return VOFOD_OK;
  o.d_tprefix.reset();
  HIPCHK(alloc_view(o.d_tbits, s.d_tbits, n_words + 2));
  HIPCHK(alloc_view(o.d_tpop, s.d_tpop, n_words + 2));
  HIPCHK(alloc_view(o.d_tprefix, s.d_tprefix, n_words + 2));
  return VOFOD_OK;
}

int sep_ensure_pts(vofod_handle* h, size_t n)
{
  vr::SepState& s = h->sep;
  auto& o = h->sep_own;
  if (o.d_bsum && n <= o.d_nsure.n)  // (d_bsum is the last of the ten: while it is there, all of them are)
    return VOFOD_OK;
  const size_t cap = n + n / 4 + 1024;
  o.d_bsum.reset();
  HIPCHK(alloc_view(o.d_px, s.d_px, cap));
  HIPCHK(alloc_view(o.d_py, s.d_py, cap));
  HIPCHK(alloc_view(o.d_pz, s.d_pz, cap));
  HIPCHK(alloc_view(o.d_pi, s.d_pi, cap));
  HIPCHK(alloc_view(o.d_sure, s.d_sure, cap));
  HIPCHK(alloc_view(o.d_sure_pre, s.d_sure_pre, cap + 1));
  HIPCHK(alloc_view(o.d_vcnt, s.d_vcnt, cap));
  HIPCHK(alloc_view(o.d_first, s.d_first, cap + 1));
  HIPCHK(alloc_view(o.d_nsure, s.d_nsure, cap));
  HIPCHK(alloc_view(o.d_bsum, s.d_bsum, cap / vr::GS_EPB + 1024));
  return VOFOD_OK;
}

// ------------------------------------------------------------------ raycast_cloud :1397-1605

// d_staged_poses: the device copy of the scan's pose table where the caller has staged it already (VOFOD_SCAN_AUTO_RAYCAST: the decode
// of this very scan read it), nullptr otherwise
int raycast_begin_locked(vofod_handle* h, const vofod_scan* scan, const float tf[12], const float* d_staged_poses)
{
  const vofod_dyn_params& dp = h->dp;
  if (h->raycast_pending)
    return VOFOD_ERR_INVALID_ARG;
  if (dp.raycast__pause)
    return VOFOD_ERR_PAUSED;
  if (!scan || !scan->intensity || !scan->range)
    return VOFOD_ERR_INVALID_ARG;
  if (scan->height != h->sp.sensor_vrays || scan->width != h->sp.sensor_hrays)
    return VOFOD_ERR_SIZE_MISMATCH;
  // vofod_set_raycast_motion: a scan with a pose per column casts each ray from its own pose (k_raycast_motion); a point scan may
  // carry the table here (the role reads range and intensity only)
  const bool motion = h->raycast_motion && scan->col_tfs;
  if (motion && scan->memspace == VOFOD_MEM_DEVICE && reinterpret_cast<uintptr_t>(scan->col_tfs) % 4 != 0)
  {
    h->err = "device-resident col_tfs: the table must be 4-byte aligned";
    return VOFOD_ERR_INVALID_ARG;
  }
  h->raycast_start_its = h->detection_its;
  h->raycast_pending = true;
  const bool exact = h->raycast_exact;  // vofod_set_raycast_exact
  const vr::ExactScale xs{exact ? std::ldexp(1.0f, h->ray_log2_units) : 0.0f, h->ray_qmax};
  const uint32_t n = static_cast<uint32_t>(scan->width) * scan->height;
  // stage intensity/range if they live on the host
  const char *d_int, *d_rng;
  uint64_t stride;
  if (scan->memspace == VOFOD_MEM_DEVICE)
  {
    d_int = static_cast<const char*>(scan->intensity);
    d_rng = static_cast<const char*>(scan->range);
    stride = scan->stride_bytes;
  }
  else if (is_range_image(*scan))
  {
    // a range image: only the two columns the raycast reads go to frame slot 0.  Columns 0-2 and the frame's arguments stay as
    // they are: under VOFOD_SCAN_AUTO_RAYCAST they hold this very scan's decoded points.
    float* base = h->ws.d_stage;
    VCHK(stage_host_column(h, base + 3 * static_cast<size_t>(h->ws.pt_cap), scan->intensity, scan->stride_bytes, n));
    VCHK(stage_host_column(h, base + 4 * static_cast<size_t>(h->ws.pt_cap), scan->range, scan->stride_bytes, n));
    d_int = reinterpret_cast<const char*>(base + 3 * static_cast<size_t>(h->ws.pt_cap));
    d_rng = reinterpret_cast<const char*>(base + 4 * static_cast<size_t>(h->ws.pt_cap));
    stride = 4;
  }
  else
  {
    // (only the two columns the raycast reads are staged: columns 0-2 of the slot stay what the last launch left there, which
    // vofod_detection_pixels may still be asked about - under VOFOD_SCAN_AUTO_RAYCAST they hold this very scan's points)
    const int r = stage_cloud(h, h->ws, 0, nullptr, nullptr, nullptr, scan->intensity, scan->range, scan->stride_bytes, n, VOFOD_MEM_HOST, 0, nullptr);
    if (r != VOFOD_OK)
      return r;
    float* base = h->ws.d_stage;
    d_int = reinterpret_cast<const char*>(base + 3 * static_cast<size_t>(h->ws.pt_cap));
    d_rng = reinterpret_cast<const char*>(base + 4 * static_cast<size_t>(h->ws.pt_cap));
    stride = 4;
  }
  // m_voxel_raycast.clear() :1430 — the sweep leaves it zeroed; clear only if an earlier pass was abandoned
  if (h->ray_dirty)
  {
    VCHK(fill_map(h, h->d_ray, 0.0f));
  }
  h->ray_dirty = true;
  // The representation belongs to the pass: recorded here, behind the staging that can still fail and beside the clear - from here on
  // the accumulator holds what this pass lays (read by finish, vofod_read_map, vofod_raycast_units and the snapshots).  A begin that
  // failed above leaves a pending FLOAT pass over whatever floats the accumulator held, as it always did.
  h->ray_pass_exact = exact;
  HIPCHK(hipMemsetAsync(h->d_counter + 1, 0, sizeof(unsigned long long), h->stream));
  vr::RayParams rp{};
  // [3P] Affine3f::rotation() == the linear part up to rounding for rigid transforms
  for (int i = 0; i < 3; i++)
  {
    for (int j = 0; j < 3; j++)
      rp.R[3 * i + j] = tf[4 * i + j];
    rp.origin[i] = tf[4 * i + 3];
  }
  rp.max_dist = static_cast<float>(dp.raycast__max_distance);
  rp.min_intensity = static_cast<float>(dp.raycast__min_intensity);
  rp.voxel_size = h->sp.voxel_size;
  rp.n = n;
  int o[3];
  h->hg.coordToIdx(rp.origin, o);
  int ret = VOFOD_OK;
  if (!h->hg.inLimits(o))  // :1432
    ret = VOFOD_ERR_SENSOR_OUTSIDE_MAP;
  else
  {
    const float* d_tab = nullptr;  // (a rigid pass reads no table, shifts or width)
    const uint32_t* d_shift = nullptr;
    uint32_t width = 0;
    if (motion)
    {
      // the table on the device: a device table where it lies, a host table in slot 0 of the synchronous workspace's pose block
      // (copied on the stream, in front of the kernel; the call waits for both, so the caller's table is free when it returns)
      d_tab = scan->memspace == VOFOD_MEM_DEVICE ? scan->col_tfs : d_staged_poses;
      if (!d_tab)
      {
        float* slot = nullptr;
        VCHK(pose_slot(h, h->ws, 0, scan->col_tfs, h->stream, slot));
        d_tab = slot;
      }
      d_shift = h->d_col_shift.p;
      width = static_cast<uint32_t>(scan->width);
    }
    const bool aligned16 = reinterpret_cast<uintptr_t>(d_tab) % 16 == 0;
    // one kernel template (kernels_raycast.h), selected by (motion, aligned16, exact), under the profiler name of the pass
    auto cast = [&](const char* label, auto acc) {
      using Acc = decltype(acc);
      auto kern = !motion ? vr::k_raycast_t<false, true, Acc> : aligned16 ? vr::k_raycast_t<true, true, Acc> : vr::k_raycast_t<true, false, Acc>;
      KLAUNCH_AS(h, label, kern, dim3((n + 255) / 256), dim3(256), rp, h->mg, acc, d_int, d_rng, stride, h->d_lut_dirs.p, h->d_lut_offs.p, h->d_mask.p, d_tab, d_shift, width,
                 reinterpret_cast<typename Acc::T*>(h->d_ray.p), reinterpret_cast<uint32_t*>(h->d_counter + 1));
    };
    if (exact)
      cast("k_raycast_exact", vr::AccUnits{xs});
    else
      cast(motion ? "k_raycast_motion" : "k_raycast", vr::AccFloat{});
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return ret;
}

int raycast_finish_locked(vofod_handle* h)
{
  if (!h->raycast_pending)
    return VOFOD_ERR_NOT_PENDING;
  h->raycast_pending = false;
  const bool exact = h->ray_pass_exact;  // (what begin laid: units or floats)
  h->ray_pass_exact = false;
  const vofod_dyn_params& dp = h->dp;
  if (h->detection_its == h->raycast_start_its)  // :1531-1537
  {
    // an abandoned exact pass takes its units with it: outside a pending exact pass the raycast map never holds anything but floats
    // (vofod_read_map, vofod_voxels_as_pc and vofod_map_export read it as such)
    if (exact)
    {
      VCHK(fill_map(h, h->d_ray, 0.0f));
      HIPCHK(hipStreamSynchronize(h->stream));
      h->ray_dirty = false;
    }
    return VOFOD_ERR_RAYCAST_NO_DETECTION;
  }
  vr::SweepParams sp{};
  sp.its_diff = static_cast<float>(h->detection_its - h->raycast_start_its);
  sp.ray_score = static_cast<float>(dp.voxel_map__scores__ray);
  const float weight = static_cast<float>(dp.raycast__weight_coefficient);
  const float voxel_diag = static_cast<float>(std::sqrt(3) * h->sp.voxel_size);
  sp.weighting_factor = weight / voxel_diag;
  sp.weight = weight;
  sp.new_rule = dp.raycast__new_update_rule;
  // max_val :1542 — zero iff no ray added a positive length; the old rule needs the value itself
  HIPCHK(hipMemcpyAsync(h->h_counter + 1, h->d_counter + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (static_cast<uint32_t>(h->h_counter[1]) == 0)
    return VOFOD_ERR_RAYCAST_EMPTY;  // :1544-1548 (flags stay as they are)
  if (!sp.new_rule && exact)
  {
    // the integer max of U, converted by the rule of the float view: float(U) rounds to nearest even, the scaling is exact
    HIPCHK(hipMemsetAsync(h->d_counter + 2, 0, sizeof(unsigned long long), h->stream));
    KLAUNCH_AS(h, "k_max_units", vr::k_max_units, dim3(2048), dim3(256), reinterpret_cast<const uint32_t*>(h->d_ray.p), h->mg.n, reinterpret_cast<uint32_t*>(h->d_counter + 2));
    HIPCHK(hipMemcpyAsync(h->h_counter + 2, h->d_counter + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    sp.max_val = std::ldexp(static_cast<float>(static_cast<uint32_t>(h->h_counter[2])), -h->ray_log2_units);
  }
  else if (!sp.new_rule)
  {
    HIPCHK(hipMemsetAsync(h->d_counter + 2, 0, sizeof(unsigned long long), h->stream));
    KLAUNCH(h, vr::k_max_nonneg, dim3(2048), dim3(256), h->d_ray, h->mg.n, reinterpret_cast<uint32_t*>(h->d_counter + 2));
    HIPCHK(hipMemcpyAsync(h->h_counter + 2, h->d_counter + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const uint32_t bits = static_cast<uint32_t>(h->h_counter[2]);
    std::memcpy(&sp.max_val, &bits, 4);
  }
  auto sweep = [&](const char* label, auto acc, float inv_scale) {
    using Acc = decltype(acc);
    KLAUNCH_AS(h, label, vr::k_ray_sweep_t<Acc>, dim3(256 * 8), dim3(256), sp, inv_scale, h->mg.n, h->d_map.p, h->d_flags.p, reinterpret_cast<typename Acc::T*>(h->d_ray.p));
  };
  if (exact)
    sweep("k_ray_sweep_exact", vr::AccUnits{}, std::ldexp(1.0f, -h->ray_log2_units));
  else
    sweep("k_ray_sweep", vr::AccFloat{}, 0.0f);  // (the float pass reads no scale)
  HIPCHK(hipStreamSynchronize(h->stream));
  h->ray_dirty = false;
  h->mapbits_valid = false;
  return VOFOD_OK;
}

// ------------------------------------------------------------------ counted grid tail

// ws holds a finished weighted voxelisation of one frame; replace the weights by the positional counts.
int counted_tail(vofod_handle* h, Workspace& ws, uint32_t V, uint32_t P, const uint32_t* d_sure_flags)
{
  vr::SepState& s = h->sep;
  VCHK(gscan(h, d_sure_flags, P, s.d_sure_pre, s.d_bsum, nullptr));
  KLAUNCH(h, vr::k_voxel_counts, dim3((V + 255) / 256), dim3(256), ws.d_hdrs, ws.va.pts, s.d_vcnt);
  VCHK(gscan(h, s.d_vcnt, V, s.d_first, s.d_bsum, nullptr));
  KLAUNCH(h, vr::k_counted_range, dim3((V + 255) / 256), dim3(256), ws.d_hdrs, s.d_first, s.d_sure_pre, P, ws.va.pts);
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// grows a workspace (Workspace::ensure); a failed allocation becomes the handle's error text
int grow_workspace(vofod_handle* h, Workspace& ws, const char* what, uint32_t F, uint32_t pt_cap, uint32_t vox_cap, uint32_t words_cap, uint32_t bricks_cap = 0)
{
  if (hipError_t e = ws.ensure(F, pt_cap, vox_cap, words_cap, bricks_cap); e != hipSuccess)
  {
    h->err = std::string(what) + hipGetErrorString(e);
    return VOFOD_ERR_DEVICE;
  }
  return VOFOD_OK;
}

// voxelise one device/host cloud into `ws` (frame 0), growing the workspace to the lattice it needs
int voxelize_cloud(vofod_handle* h, Workspace& ws, const vofod_cloud_view* in, GridParams& g, const float leaf[3], bool align, const float* align_center, FrameHdr& hdr)
{
  const uint32_t n = static_cast<uint32_t>(in->n);
  // Growth with headroom: a workspace grows by releasing and allocating its three dozen arrays (2.6 ms), and the cloud of
  // updateSeparatedBGClusters - the map's background voxels - gains a few thousand points from one call to the next while the map
  // warms: sized to the point, EVERY call of the role paid that (VOFOD_TRACE: 2.7 of the role's 2.9 ms).
  const uint32_t want = n > std::min(ws.pt_cap, ws.vox_cap) ? n + n / 2 + 4096u : std::max(n, 1u);
  VCHK(grow_workspace(h, ws, "workspace allocation: ", 1, want, want, std::max(ws.words_cap, 1u << 16)));
  for (int attempt = 0; attempt < 2; attempt++)
  {
    VCHK(stage_cloud(h, ws, 0, in->x, in->y, in->z, in->intensity, nullptr, in->stride_bytes, n, in->memspace, 0, nullptr));
    const float zero[3] = {0, 0, 0};
    fill_grid_params(h, g, leaf, align, align ? align_center : zero, ws);
    VCHK(launch_lattice(h, ws, g, 1, n));  // (the lattice's size is inspected before the bitmap is touched)
    HIPCHK(hipMemcpyAsync(&ws.h_packed[0].hdr, ws.d_hdrs, sizeof(FrameHdr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    hdr = ws.h_packed[0].hdr;
    const uint32_t need_bricks =
        hdr.n_in ? static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>((hdr.div_b[0] + 3) / 4) * ((hdr.div_b[1] + 3) / 4) * ((hdr.div_b[2] + 3) / 4), 1u << 28)) : 0u;
    if ((hdr.status == VOFOD_ERR_CAPACITY || (hdr.status == VOFOD_OK && need_bricks > ws.bricks_cap)) && attempt == 0)
    {
      VCHK(grow_workspace(h, ws, "workspace allocation: ", 1, n, n, hdr.need_words + hdr.need_words / 4 + 64, need_bricks + need_bricks / 4));
      continue;
    }
    break;
  }
  if (hdr.status != VOFOD_OK)
    return hdr.status;
  if (hdr.n_in == 0)
  {
    hdr.V = 0;
    return VOFOD_OK;
  }
  VCHK(launch_bitmap_chain(h, ws, g, 1, n, true));
  HIPCHK(hipMemcpyAsync(&ws.h_packed[0].hdr, ws.d_hdrs, sizeof(FrameHdr), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  hdr = ws.h_packed[0].hdr;
  return hdr.status;
}

// ------------------------------------------------------------------ updateSeparatedBGClusters :1126-1277

int sepclusters_begin_locked(vofod_handle* h, int* sure_out)
{
  const vofod_dyn_params& dp = h->dp;
  if (sure_out)
    *sure_out = h->sure_background_sufficient;
  if (dp.sepclusters__pause)
    return VOFOD_ERR_PAUSED;
  h->sep_pending = false;
  h->sep_start_its = h->detection_its;
  vr::SepState& s = h->sep;
  static const bool trace = std::getenv("VOFOD_TRACE") != nullptr;
  const auto t0 = clk::now();
  double tr[5] = {0, 0, 0, 0, 0};
  const float thr_new = static_cast<float>(dp.voxel_map__thresholds__new_obstacles);
  const float thr_sure = static_cast<float>(dp.voxel_map__thresholds__sure_obstacles);
  const float max_dist_idx = static_cast<float>(dp.sepclusters__max_bg_distance / h->sp.voxel_size);
  const int max_voxel_dist = static_cast<int>(std::ceil(max_dist_idx));
  const float lsz = static_cast<float>(std::max(max_voxel_dist - 1, 0));
  if (!(lsz > 0.0f))
    return VOFOD_ERR_INVALID_ARG;

  // K16: thresholded voxels in x-outer / z-inner order (voxelsAsVoxelPC :1153)
  VCHK(ensure_mapbits(h, thr_new));
  const uint32_t ncol = static_cast<uint32_t>(h->mg.sx) * h->mg.sy;
  VCHK(sep_ensure_words(h, ncol + 2));
  VCHK(sep_ensure_pts(h, std::max<size_t>(1 << 16, ncol)));  // also sizes the scan's block sums
  KLAUNCH(h, vr::k_col_count, dim3((ncol + 255) / 256), dim3(256), h->mg, h->d_mapbits, s.d_tpop);
  VCHK(gscan(h, s.d_tpop, ncol, s.d_tprefix, s.d_bsum, s.d_small));
  HIPCHK(hipMemcpyAsync(s.h_small, s.d_small, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const uint32_t P = s.h_small[0];
  s.P = P;
  tr[0] = ms_since(t0);
  if (P == 0)
    return VOFOD_ERR_EMPTY;  // :1155-1159
  VCHK(sep_ensure_pts(h, P));
  KLAUNCH(h, vr::k_col_emit, dim3((ncol + 255) / 256), dim3(256), h->mg, h->d_map, h->d_mapbits, s.d_tprefix, thr_sure, s.d_px, s.d_py, s.d_pz, s.d_pi, s.d_sure);

  // K6': VoxelGridCounted with leaf lsz on the index cloud (:1162-1167)
  vofod_cloud_view view{};
  view.x = s.d_px;
  view.y = s.d_py;
  view.z = s.d_pz;
  view.intensity = s.d_pi;
  view.stride_bytes = 4;
  view.n = P;
  view.memspace = VOFOD_MEM_DEVICE;
  const float leaf[3] = {lsz, lsz, lsz};
  FrameHdr hdr;
  VCHK(voxelize_cloud(h, h->sepws, &view, s.g, leaf, false, nullptr, hdr));
  Workspace& ws = h->sepws;
  tr[1] = ms_since(t0);
  VCHK(counted_tail(h, ws, hdr.V, P, s.d_sure));
  tr[2] = ms_since(t0);

  // clusterCloud(vmap_pc_ds, max_voxel_dist) :1171
  const float cmax = static_cast<float>(std::max({h->mg.sx, h->mg.sy, h->mg.sz})) + 2 * lsz;
  vofod_handle::ClusterTables* ct = nullptr;
  VCHK(cluster_tables(h, s.g, static_cast<float>(max_voxel_dist), cmax, &ct));
  VCHK(launch_cluster(h, ws, plan_cluster_only(h, ws, ct), s.g, ct));
  tr[3] = ms_since(t0);
  // sure voxels per cluster :1175-1183 and the latch :1188-1206
  HIPCHK(hipMemsetAsync(s.d_nsure, 0, sizeof(uint32_t) * std::max(hdr.V, 1u), h->stream));
  HIPCHK(hipMemsetAsync(s.d_small + 1, 0, 2 * sizeof(uint32_t), h->stream));
  const uint32_t gv = (hdr.V + 255) / 256;
  KLAUNCH(h, vr::k_cluster_sure, dim3(gv), dim3(256), ws.d_hdrs, ws.va.pts, ws.d_labels, s.d_nsure);
  KLAUNCH(h, vr::k_any_sure, dim3(gv), dim3(256), ws.d_hdrs, ws.d_labels, s.d_nsure, static_cast<uint32_t>(dp.sepclusters__min_sure_points), s.d_small + 1);
  HIPCHK(hipMemcpyAsync(s.h_small, s.d_small, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (trace)
    std::fprintf(stderr, "[vofod trace] sepclusters_begin: thresholded cloud (P = %u) %.3f, counted grid (V = %u) %.3f, counts %.3f, clustering enqueued %.3f, end %.3f ms\n", P, tr[0], hdr.V, tr[1], tr[2],
                 tr[3], ms_since(t0));
  if (s.h_small[1] == 0)
  {
    h->sure_background_sufficient = false;  // :1195
    if (sure_out)
      *sure_out = 0;
    return VOFOD_OK;
  }
  h->sure_background_sufficient = true;  // :1205
  if (sure_out)
    *sure_out = 1;
  h->sep_pending = true;
  return VOFOD_OK;
}

int sepclusters_finish_locked(vofod_handle* h)
{
  if (!h->sep_pending)
    return VOFOD_ERR_NOT_PENDING;
  h->sep_pending = false;
  const vofod_dyn_params& dp = h->dp;
  vr::SepState& s = h->sep;
  const float max_dist_idx = static_cast<float>(dp.sepclusters__max_bg_distance / h->sp.voxel_size);
  const int mvd = static_cast<int>(std::ceil(max_dist_idx));
  const float its_diff = static_cast<float>(std::max(h->detection_its - h->sep_start_its, 1));  // :1212
  static const bool trace = std::getenv("VOFOD_TRACE") != nullptr;
  const auto t0 = clk::now();
  std::vector<int> offs;  // :1219-1237
  for (int x = -mvd; x <= mvd; x++)
    for (int y = -mvd; y <= mvd; y++)
      for (int z = -mvd; z <= mvd; z++)
      {
        const int norm = static_cast<int>(std::sqrt(static_cast<double>(x * x + y * y + z * z)));
        if (static_cast<float>(norm) <= max_dist_idx)
        {
          offs.push_back(x);
          offs.push_back(y);
          offs.push_back(z);
        }
      }
  if (mvd > MAX_R)
    return VOFOD_ERR_INVALID_ARG;
  HIPCHK(hipMemcpyAsync(s.d_offsets, offs.data(), offs.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  vr::EraseParams ep{};
  ep.update_val = static_cast<float>(dp.voxel_map__scores__ray);
  ep.w1 = std::clamp(std::pow(1.0f - 0.5f, its_diff), 0.0f, 1.0f);  // :1240-1241
  ep.w2 = 1.0f - ep.w1;
  ep.min_sure = static_cast<uint32_t>(dp.sepclusters__min_sure_points);
  ep.n_offsets = static_cast<int>(offs.size() / 3);
  Workspace& ws = h->sepws;
  const uint32_t gv = (ws.vox_cap + 255) / 256;
  const uint32_t oy = static_cast<uint32_t>(std::max(1, std::min(ep.n_offsets / 16, 256)));
  KLAUNCH(h, vr::k_sep_erase, dim3(gv, oy), dim3(256), ep, h->mg, ws.d_hdrs, ws.va.pts, ws.d_labels, s.d_nsure, s.d_offsets, h->d_map);
  HIPCHK(hipStreamSynchronize(h->stream));
  if (trace)
    std::fprintf(stderr, "[vofod trace] sepclusters_finish: %d stencil offsets, %.3f ms\n", ep.n_offsets, ms_since(t0));
  h->mapbits_valid = false;
  return VOFOD_OK;
}

int copy_grid_out(vofod_handle* h, Workspace& ws, const GridParams& g, const FrameHdr& hdr, vofod_point_xyzr* out, uint32_t* keys, size_t cap, size_t* n_out,
                  vofod_grid_desc* grid)
{
  if (grid)
    for (int a = 0; a < 3; a++)
    {
      grid->leaf[a] = g.leaf[a];
      grid->offset[a] = hdr.offset[a];
      grid->min_b[a] = hdr.min_b[a];
      grid->div_b[a] = hdr.div_b[a];
    }
  if (n_out)
    *n_out = hdr.V;
  if (hdr.V > cap)
    return VOFOD_ERR_CAPACITY;
  if (hdr.V && out)
    HIPCHK(hipMemcpy(out, ws.va.pts, sizeof(float4) * hdr.V, hipMemcpyDeviceToHost));
  if (hdr.V && keys)
    HIPCHK(hipMemcpy(keys, ws.va.key, sizeof(uint32_t) * hdr.V, hipMemcpyDeviceToHost));
  return VOFOD_OK;
}

// every copy of the geometry the handle keeps, from h->sp (vsh::area_geometry: vofod_create and vofod_map_shift)
void set_area_geometry(vofod_handle* h)
{
  vsh::AreaGeometry g;
  vsh::area_geometry(h->sp, g);
  for (int a = 0; a < 3; a++)
  {
    h->exclude_center[a] = g.exclude_center[a];
    h->oparea_center[a] = g.oparea_center[a];
    h->mg.off[a] = h->hg.off[a] = g.map_off[a];
    h->hg.s[a] = g.map_size[a];
  }
  h->background_min_sufficient_pts = g.background_min_sufficient_pts;
  h->mg.vs = h->hg.vs = h->sp.voxel_size;
  h->mg.vs_inv = h->hg.vs_inv = 1.0f / h->sp.voxel_size;
  h->mg.sx = g.map_size[0];
  h->mg.sy = g.map_size[1];
  h->mg.sz = g.map_size[2];
  h->mg.n = static_cast<uint64_t>(g.map_size[0]) * g.map_size[1] * g.map_size[2];
}

}  // namespace

extern "C" {

void vofod_destroy(vofod_handle* h)
{
  if (!h)
    return;
  (void)hipSetDevice(h->device);
  if (h->stream)
    (void)hipStreamSynchronize(h->stream);
  delete h;
}

int vofod_create(const vofod_static_params* sp, const vofod_dyn_params* dp, vofod_handle** out)
{
  if (!sp || !dp || !out || !(sp->voxel_size > 0) || sp->sensor_hrays < 2 || sp->sensor_vrays < 2)
    return VOFOD_ERR_INVALID_ARG;
  *out = nullptr;
  vofod_handle* h = new vofod_handle;
  h->sp = *sp;
  h->dp = *dp;
  h->device = sp->device;
  h->sp.lut_directions = nullptr;
  h->sp.lut_offsets = nullptr;
  h->sp.mask = nullptr;
  auto fail = [&](int code) {
    std::fprintf(stderr, "vofod_create: %s\n", h->err.c_str());
    vofod_destroy(h);
    return code;
  };
#define CREATE_CHK(expr)                                                        \
  do                                                                            \
  {                                                                             \
    const hipError_t e_ = (expr);                                               \
    if (e_ != hipSuccess)                                                       \
    {                                                                           \
      h->err = std::string(#expr) + ": " + hipGetErrorString(e_);               \
      return fail(VOFOD_ERR_DEVICE);                                            \
    }                                                                           \
  } while (0)
  CREATE_CHK(hipSetDevice(h->device));
  CREATE_CHK(h->chain_stream[0].create(hipStreamCreateWithFlags, hipStreamNonBlocking));
  h->stream = h->chain_stream[0];
  {
    // the tail's one small kernel (k_explore) has the host waiting for it: highest priority, so that it is dispatched at the
    // next kernel boundary of the batches in flight instead of behind their queued kernels
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    int prio_tail = prio_hi;
    if (const char* e = std::getenv("VOFOD_TAIL_PRIO"))  // (diagnostics) hi | mid | lo
      prio_tail = e[0] == 'l' ? prio_lo : e[0] == 'm' ? (prio_lo + prio_hi) / 2 : prio_hi;
    CREATE_CHK(h->stream_tail.create(hipStreamCreateWithPriority, hipStreamNonBlocking, prio_tail));
    // staged pipeline of submitted batches (launch_frames): streaming kernels below the frame kernels
    CREATE_CHK(h->stream_key.create(hipStreamCreateWithPriority, hipStreamNonBlocking, prio_lo));
    // (VOFOD_FRAME_STREAMS: diagnostics - the number of frame streams, 1..8)
    h->n_frame_streams = 2;  // (more streams cost more than they bring: 811 k / 763 k / 656 k frames/s with 2 / 4 / 8 of them, 32-frame batches 435 k / 268 k / 216 k)
    if (const char* e = std::getenv("VOFOD_FRAME_STREAMS"))
      h->n_frame_streams = std::min(std::max(std::atoi(e), 1), static_cast<int>(vofod_handle::MAX_FRAME_STREAMS));
    for (int i = 0; i < h->n_frame_streams; i++)
      CREATE_CHK(h->stream_frames[i].create(hipStreamCreateWithPriority, hipStreamNonBlocking, (prio_lo + prio_hi) / 2));
    h->stream_frame = h->stream_frames[0];
  }
  // (tickets 1-3 have their streams from the start; tickets 4-7 - only small batches gain from more than four in flight - get
  // theirs when they are first taken: streams that merely exist are not free)
  for (int t = 1; t < 4; t++)
    CREATE_CHK(h->chain_stream[t].create(hipStreamCreateWithFlags, hipStreamNonBlocking));
  set_area_geometry(h);
  const int* sizes = h->hg.s;
  const size_t M = h->mg.n;
  const size_t M4 = std::max<size_t>(M, 4);  // (k_map_shift's clamped 16-byte load reads the first four voxels of any map)
  CREATE_CHK(h->d_map.alloc(M4));
  CREATE_CHK(h->d_flags.alloc(M4));
  CREATE_CHK(h->d_ray.alloc(M4));
  CREATE_CHK(h->d_mapbits.alloc((M + 63) / 64 + 2));
  CREATE_CHK(hipMemset(h->d_mapbits, 0, ((M + 63) / 64 + 2) * sizeof(unsigned long long)));
  CREATE_CHK(h->d_mapclose.alloc((M + 63) / 64 + 2));
  CREATE_CHK(h->d_counter.alloc(8));
  CREATE_CHK(h->h_counter.alloc(8));
  CREATE_CHK(h->d_bgcount.alloc(8 * MB_SLOTS));
  CREATE_CHK(h->h_bgcount.alloc(8 * MB_SLOTS));
  CREATE_CHK(h->d_rows.alloc(MAX_STENCIL_ROWS));
  CREATE_CHK(h->d_crows.alloc(MAX_STENCIL_ROWS));
  // sensor
  const size_t n = static_cast<size_t>(sp->sensor_hrays) * sp->sensor_vrays;
  std::vector<float> dirs(3 * n), offs(3 * n, 0.0f);
  if (sp->lut_directions)
    std::copy(sp->lut_directions, sp->lut_directions + 3 * n, dirs.begin());
  else
    vofod_sim_lut(sp->sensor_hrays, sp->sensor_vrays, sp->sensor_vfov, dirs.data());
  if (sp->lut_offsets)
    std::copy(sp->lut_offsets, sp->lut_offsets + 3 * n, offs.begin());
  std::vector<uint8_t> mask(n, 1);
  if (sp->mask)
    std::copy(sp->mask, sp->mask + n, mask.begin());
  CREATE_CHK(h->d_lut_dirs.alloc(3 * n));
  CREATE_CHK(h->d_lut_offs.alloc(3 * n));
  CREATE_CHK(h->d_mask.alloc(n));
  CREATE_CHK(hipMemcpy(h->d_lut_dirs, dirs.data(), 3 * n * sizeof(float), hipMemcpyHostToDevice));
  CREATE_CHK(hipMemcpy(h->d_lut_offs, offs.data(), 3 * n * sizeof(float), hipMemcpyHostToDevice));
  CREATE_CHK(hipMemcpy(h->d_mask, mask.data(), n, hipMemcpyHostToDevice));
  if (!vr::ray_exact_scale(sp->voxel_size, sp->sensor_hrays, sp->sensor_vrays, h->ray_log2_units, h->ray_qmax))
    h->ray_log2_units = -1;
  CREATE_CHK(h->d_col_shift.alloc(static_cast<size_t>(sp->sensor_vrays)));
  CREATE_CHK(hipMemset(h->d_col_shift, 0, sizeof(uint32_t) * std::max(sp->sensor_vrays, 1)));
  // per-frame workspace: the crops bound the voxel-grid lattice by the map lattice plus one cell per side
  const uint64_t cells = static_cast<uint64_t>(sizes[0] + 2) * (sizes[1] + 2) * (sizes[2] + 2);
  if (cells > 0x7fffffffull)
  {
    h->err = "voxel map too fine for 32-bit voxel keys";
    return fail(VOFOD_ERR_INDEX_OVERFLOW);
  }
  const uint32_t F = static_cast<uint32_t>(std::max(sp->max_batch_frames, 1));
  const uint32_t nbricks = static_cast<uint32_t>(((sizes[0] + 2 + 3) / 4) * ((sizes[1] + 2 + 3) / 4) * static_cast<uint64_t>((sizes[2] + 2 + 3) / 4));
  CREATE_CHK(h->ws.ensure(F, static_cast<uint32_t>(n), static_cast<uint32_t>(n), static_cast<uint32_t>((cells + 63) / 64), nbricks));
#undef CREATE_CHK
  {
    // host workers for the per-frame tail of a batch (frames are independent); VOFOD_THREADS overrides
    unsigned nt = std::min(8u, std::max(1u, std::thread::hardware_concurrency() / 2));
    if (const char* e = std::getenv("VOFOD_THREADS"))
      nt = std::max(1, std::atoi(e));
    if (F == 1)
      nt = 1;
    h->pool.reset(new vt::Pool(nt));
  }
  if (do_reset(h) != VOFOD_OK)
    return fail(VOFOD_ERR_DEVICE);
  h->sure_background_sufficient = false;  // :283-284
  h->background_pts_sufficient = false;
  h->last_detection_id = 0;  // :296
  (void)hipDeviceSynchronize();  // null-stream memsets of the set-up are complete before any non-blocking stream runs
  *out = h;
  return VOFOD_OK;
}

static int world_clear(vofod_handle* h);  // (api_maps.h, with the other host helpers of the world store)

int vofod_reset(vofod_handle* h)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE | MAP_UNREAD));
  if (h->world.enabled)
    VCHK(world_clear(h));  // W is init everywhere: K, the box and the switch stay (do_reset synchronises)
  h->wsync.end_chains();  // (world snapshots: the slots are handed out again, and a follower's store is no longer what it applied)
  const int r = do_reset(h);
  h->sure_background_sufficient = false;
  h->background_pts_sufficient = false;
  h->last_detection_id = 0;
  h->cf_off = false;
  forget_detections(h);  // (the ids start again, nothing collected before answers any more)
  return r;
}

int vofod_set_dynamic_params(vofod_handle* h, const vofod_dyn_params* dp)
{
  if (!h || !dp)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h, ApiLock::LOCK_ONLY);
  VCHK(admit(h, NEEDS_NOTHING));
  h->dp = *dp;
  return VOFOD_OK;
}

const char* vofod_last_error_string(vofod_handle* h) { return h ? h->err.c_str() : "null handle"; }

int vofod_get_status(vofod_handle* h, vofod_status_info* out)
{
  if (!h || !out)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h, ApiLock::LOCK_ONLY);
  VCHK(admit(h, NEEDS_NOTHING));
  out->detection_its = h->detection_its;
  out->last_detection_id = h->last_detection_id;
  out->background_pts_sufficient = h->background_pts_sufficient;
  out->sure_background_sufficient = h->sure_background_sufficient;
  out->raycast_pending = h->raycast_pending;
  out->map_size[0] = h->mg.sx;
  out->map_size[1] = h->mg.sy;
  out->map_size[2] = h->mg.sz;
  for (int a = 0; a < 3; a++)
    out->map_offset[a] = h->mg.off[a];
  return VOFOD_OK;
}

int vofod_raycast_begin(vofod_handle* h, const vofod_scan* scan, const float tf[12])
{
  if (!h || !tf)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE));
  return raycast_begin_locked(h, scan, tf, nullptr);
}

// A handle property, as the column shifts: off after vofod_create, kept across vofod_reset, vofod_map_apply and vofod_map_shift.
int vofod_set_raycast_motion(vofod_handle* h, int on)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h, ApiLock::LOCK_ONLY);
  VCHK(admit(h, WS0_FREE | MAP_UNREAD | NO_RAYCAST_PASS));
  h->raycast_motion = on != 0;
  return VOFOD_OK;
}

// A handle property with the rules of vofod_set_raycast_motion.  The switch chooses the representation of the NEXT pass; a pending
// pass keeps its own (raycast_begin_locked records it), which is why the switch is refused while one is pending.
int vofod_set_raycast_exact(vofod_handle* h, int on)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h, ApiLock::LOCK_ONLY);
  VCHK(admit(h, WS0_FREE | MAP_UNREAD | NO_RAYCAST_PASS));
  if (on && h->ray_log2_units < 0)
  {
    h->err = "exact raycast accumulation: sensor_hrays * sensor_vrays * (2 * voxel_size + 1) does not fit in 32 bits";
    return VOFOD_ERR_INDEX_OVERFLOW;
  }
  h->raycast_exact = on != 0;
  return VOFOD_OK;
}

int vofod_raycast_units(vofod_handle* h, uint32_t* units, size_t n, int32_t* log2_units_per_m)
{
  if (!h || !units || !log2_units_per_m)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));
  if (!h->raycast_pending || !h->ray_pass_exact)
    return VOFOD_ERR_NOT_PENDING;
  if (n != h->mg.n)
    return VOFOD_ERR_SIZE_MISMATCH;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(units, h->d_ray.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  *log2_units_per_m = h->ray_log2_units;
  return VOFOD_OK;
}

int vofod_raycast_finish(vofod_handle* h)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, MAP_UNREAD));
  return raycast_finish_locked(h);
}

int vofod_sepclusters_begin(vofod_handle* h, int* sure)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE));
  return sepclusters_begin_locked(h, sure);
}

int vofod_sepclusters_finish(vofod_handle* h)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE | MAP_UNREAD));
  return sepclusters_finish_locked(h);
}

int vofod_voxel_grid_weighted(vofod_handle* h, const vofod_cloud_view* in, float leaf, int align, const float align_center[3], vofod_point_xyzr* out, uint32_t* keys,
                              size_t cap, size_t* n_out, vofod_grid_desc* grid)
{
  if (!h || !in || !(leaf > 0) || (align && !align_center) || in->n > 0x7fffffffu)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE));
  GridParams g;
  FrameHdr hdr{};
  const float l[3] = {leaf, leaf, leaf};
  if (in->n == 0)
  {
    if (n_out)
      *n_out = 0;
    if (grid)
      *grid = vofod_grid_desc{{leaf, leaf, leaf}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    return VOFOD_OK;
  }
  const int r = voxelize_cloud(h, h->aux, in, g, l, align != 0, align_center, hdr);
  if (r != VOFOD_OK)
  {
    if (n_out)
      *n_out = 0;
    return r;
  }
  return copy_grid_out(h, h->aux, g, hdr, out, keys, cap, n_out, grid);
}

int vofod_voxel_grid_counted(vofod_handle* h, const vofod_cloud_view* in, float leaf, float threshold, vofod_point_xyzr* out, uint32_t* keys, size_t cap, size_t* n_out,
                             vofod_grid_desc* grid)
{
  if (!h || !in || !(leaf > 0) || !in->intensity || in->n > 0x7fffffffu)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE));
  GridParams g;
  FrameHdr hdr{};
  const float l[3] = {leaf, leaf, leaf};
  if (in->n == 0)
  {
    if (n_out)
      *n_out = 0;
    return VOFOD_OK;
  }
  int r = voxelize_cloud(h, h->aux, in, g, l, false, nullptr, hdr);
  if (r != VOFOD_OK)
  {
    if (n_out)
      *n_out = 0;
    return r;
  }
  const uint32_t P = static_cast<uint32_t>(in->n);
  VCHK(sep_ensure_words(h, 1));
  VCHK(sep_ensure_pts(h, P));
  const FrameArgs& a = h->aux.h_args[0];
  KLAUNCH(h, vr::k_flag_over, dim3((P + 255) / 256), dim3(256), a.intensity, a.stride, P, threshold, h->sep.d_sure);
  VCHK(counted_tail(h, h->aux, hdr.V, P, h->sep.d_sure));
  HIPCHK(hipStreamSynchronize(h->stream));
  return copy_grid_out(h, h->aux, g, hdr, out, keys, cap, n_out, grid);
}

int vofod_cluster(vofod_handle* h, const vofod_point_xyzr* pts, const uint32_t* keys, const vofod_grid_desc* grid, size_t n, float tolerance, uint32_t* labels,
                  size_t* n_clusters)
{
  if (!h || (!pts && n) || !labels || !keys || !grid || !(tolerance > 0) || n > 0x7fffffffu)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE));
  if (n_clusters)
    *n_clusters = 0;
  if (n == 0)
    return VOFOD_OK;
  const uint64_t cells = static_cast<uint64_t>(grid->div_b[0]) * grid->div_b[1] * grid->div_b[2];
  if (grid->div_b[0] <= 0 || grid->div_b[1] <= 0 || grid->div_b[2] <= 0 || cells > 0x7fffffffull)
    return VOFOD_ERR_INVALID_ARG;
  for (size_t i = 0; i < n; i++)
    if (keys[i] >= cells || (i && keys[i] <= keys[i - 1]))
    {
      h->err = "vofod_cluster: keys must be strictly ascending lattice keys";
      return VOFOD_ERR_INVALID_ARG;
    }
  Workspace& ws = h->aux;
  const uint32_t words = static_cast<uint32_t>((cells + 63) / 64);
  const uint32_t need_bricks = static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>((grid->div_b[0] + 3) / 4) * ((grid->div_b[1] + 3) / 4) * ((grid->div_b[2] + 3) / 4), 1u << 28));
  VCHK(grow_workspace(h, ws, "workspace allocation: ", 1, static_cast<uint32_t>(n), static_cast<uint32_t>(n), words + 64, need_bricks));
  // rebuild the frame state the clustering kernels consume: header, bitmap, word prefix, voxel arrays
  GridParams g;
  const float zero[3] = {0, 0, 0};
  fill_grid_params(h, g, grid->leaf, false, zero, ws);
  FrameHdr hdr{};
  hdr.n_in = static_cast<uint32_t>(n);
  hdr.status = VOFOD_OK;
  for (int a = 0; a < 3; a++)
  {
    hdr.offset[a] = grid->offset[a];
    hdr.min_b[a] = grid->min_b[a];
    hdr.div_b[a] = grid->div_b[a];
  }
  hdr.n_cells = static_cast<uint32_t>(cells);
  hdr.n_words = words;
  hdr.V = static_cast<uint32_t>(n);
  std::vector<unsigned long long> bm(words + 2, 0ull);
  for (size_t i = 0; i < n; i++)
    bm[keys[i] >> 6] |= 1ull << (keys[i] & 63);
  std::vector<uint32_t> prefix(words + 2, 0u), ident(n);
  uint32_t run = 0;
  for (uint32_t w = 0; w < words; w++)
  {
    prefix[w] = run;
    run += __builtin_popcountll(bm[w]);
  }
  for (size_t i = 0; i < n; i++)
    ident[i] = static_cast<uint32_t>(i);
  std::vector<int32_t> cbox(6 * n);
  for (size_t i = 0; i < n; i++)
    for (int c = 0; c < 3; c++)
    {
      cbox[6 * i + c] = 0x7fffffff;
      cbox[6 * i + 3 + c] = static_cast<int32_t>(0x80000000u);
    }
  HIPCHK(hipMemcpyAsync(ws.d_hdrs, &hdr, sizeof(hdr), hipMemcpyHostToDevice, h->stream));
  ws.bitmap_clean = false;
  HIPCHK(hipMemcpyAsync(ws.d_bitmaps, bm.data(), sizeof(unsigned long long) * (words + 2), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(ws.d_wprefix, prefix.data(), sizeof(uint32_t) * (words + 2), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(ws.va.pts, pts, sizeof(float4) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(ws.va.key, keys, sizeof(uint32_t) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(ws.va.parent, ident.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(ws.va.csize, 0, sizeof(uint32_t) * n, h->stream));
  HIPCHK(hipMemsetAsync(ws.va.cclose, 0, sizeof(uint32_t) * n, h->stream));
  HIPCHK(hipMemcpyAsync(ws.va.cbox, cbox.data(), sizeof(int32_t) * 6 * n, hipMemcpyHostToDevice, h->stream));
  float cmax = 0;
  for (int a = 0; a < 3; a++)
    cmax = std::max({cmax, std::fabs(grid->offset[a]), std::fabs(grid->offset[a] + grid->leaf[a] * (grid->div_b[a] + 1))});
  vofod_handle::ClusterTables* ct = nullptr;
  VCHK(cluster_tables(h, g, tolerance, cmax, &ct));
  VCHK(launch_cluster(h, ws, plan_cluster_only(h, ws, ct), g, ct));
  HIPCHK(hipMemcpyAsync(labels, ws.d_labels, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (n_clusters)
  {
    size_t c = 0;
    for (size_t i = 0; i < n; i++)
      c += labels[i] == i;
    *n_clusters = c;
  }
  return VOFOD_OK;
}

int vofod_profile_enable(vofod_handle* h, int on)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));
  (void)hipStreamSynchronize(h->stream);
  for (auto& r : h->prof.recs)
  {
    h->prof.pool.push_back(r.a);
    h->prof.pool.push_back(r.b);
  }
  h->prof.recs.clear();
  h->prof.on = on != 0;
  return VOFOD_OK;
}

size_t vofod_profile_read(vofod_handle* h, char* names, double* ms, uint64_t* calls, size_t cap)
{
  if (!h || !names || !ms || !calls)
    return 0;
  ApiLock lock(h);
  if (admit(h, NEEDS_NOTHING) != VOFOD_OK)
    return 0;
  (void)hipStreamSynchronize(h->stream);
  std::vector<std::string> order;
  std::map<std::string, std::pair<double, uint64_t>> acc;
  for (auto& r : h->prof.recs)
  {
    float t = 0;
    (void)hipEventElapsedTime(&t, r.a, r.b);
    std::string nm = r.name;
    const size_t c = nm.rfind(':');
    if (c != std::string::npos)
      nm = nm.substr(c + 1);
    if (!acc.count(nm))
      order.push_back(nm);
    acc[nm].first += t;
    acc[nm].second += 1;
    h->prof.pool.push_back(r.a);
    h->prof.pool.push_back(r.b);
  }
  h->prof.recs.clear();
  size_t n = 0;
  for (const auto& nm : order)
  {
    if (n >= cap)
      break;
    std::memset(names + 64 * n, 0, 64);
    std::strncpy(names + 64 * n, nm.c_str(), 63);
    ms[n] = acc[nm].first;
    calls[n] = acc[nm].second;
    n++;
  }
  return n;
}

}  // extern "C"
