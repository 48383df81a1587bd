// The frame entry points of include/vofod.h (included by vofod_hip.hip after driver_aux.h): scans and batches through
// frames_launch.h / frames_collect.h, the one-scan views of the batch path's input steps, and the detections' member voxels.
#pragma once

extern "C" {

int vofod_process_scan(vofod_handle* h, const vofod_scan* scan, const float tf[12], int flags, vofod_detection* out, size_t cap, size_t* n_out, vofod_scan_debug* dbg)
{
  if (!h || !scan || !tf || !n_out)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE | (flags & VOFOD_SCAN_NO_MAP_UPDATE ? NEEDS_NOTHING : MAP_UNREAD)));
  *n_out = 0;
  // (a cold map: more far voxels than the close-first path of a single scan takes - nothing of the scan was applied; it runs once
  // more, through the full clustering)
  return process_frames(h, scan, tf, 1, flags, out, cap, nullptr, n_out, dbg);
}

int vofod_process_batch(vofod_handle* h, const vofod_scan* scans, const float* tfs, size_t n, vofod_detection* out, size_t cap, uint32_t* n_out_per_frame, size_t* n_out,
                        vofod_scan_debug* dbg)
{
  if (!h || !scans || !tfs || !n_out)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE));
  *n_out = 0;
  int ret = VOFOD_OK;
  size_t total = 0;
  for (size_t base = 0; base < n; base += h->ws.F)  // larger batches run as successive launch groups
  {
    const uint32_t m = static_cast<uint32_t>(std::min<size_t>(h->ws.F, n - base));
    size_t got = 0;
    const int r = process_frames(h, scans + base, tfs + 12 * base, m, VOFOD_SCAN_NO_MAP_UPDATE, out ? out + total : nullptr, total < cap ? cap - total : 0,
                                 n_out_per_frame ? n_out_per_frame + base : nullptr, &got, dbg ? dbg + base : nullptr);
    for (size_t i = total; i < std::min(total + got, cap); i++)
      out[i].frame += static_cast<uint32_t>(base);
    total += got;
    if (r != VOFOD_OK)
      ret = r;
  }
  if (n > h->ws.F)
    h->ws.det_valid = false;  // (successive launch groups overwrite each other's lists: vofod_detection_points has nothing to answer from)
  *n_out = total;
  return ret;
}

int vofod_batch_submit(vofod_handle* h, const vofod_scan* scans, const float* tfs, size_t n, int* ticket)
{
  if (!h || !scans || !tfs || !ticket)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));  // (a ticket is taken beside the batches in flight; eight of them are a matter of capacity)
  if (n > h->ws.F)
  {
    h->err = "batch larger than max_batch_frames";
    return VOFOD_ERR_CAPACITY;
  }
  int t = -1;
  for (int i = 0; i < vofod_handle::MAX_INFLIGHT && t < 0; i++)
    if (!h->slot(i)->pending)
      t = i;
  if (t < 0)
  {
    h->err = "eight batches already in flight: collect one first";
    return VOFOD_ERR_CAPACITY;
  }
  if (t >= 4)
  {
    // more than four chains in flight: they only run side by side when the runtime may use more than its default of four
    // hardware queues (a process-wide setting read when the runtime initialises: INTEGRATION.md) - say so once
    static std::once_flag warned;
    const char* q = std::getenv("GPU_MAX_HW_QUEUES");
    if (!q || std::atoi(q) < 8)
      std::call_once(warned, [] {
        std::fprintf(stderr, "[vofod] more than four batches in flight but GPU_MAX_HW_QUEUES is %s: their streams share four hardware queues and take turns "
                             "(32-frame batches: ~140 k instead of ~230 k frames/s); export GPU_MAX_HW_QUEUES=16 before the process starts\n",
                     std::getenv("GPU_MAX_HW_QUEUES") ? std::getenv("GPU_MAX_HW_QUEUES") : "unset");
      });
  }
  Workspace* w = h->slot(t);
  if (w->F == 0)
    VCHK(grow_workspace(h, *w, "extra workspace: ", h->ws.F, h->ws.pt_cap, h->ws.vox_cap, h->ws.words_cap, h->ws.bricks_cap));
  FrameCall call{true, scans, tfs, static_cast<uint32_t>(n), VOFOD_SCAN_NO_MAP_UPDATE, nullptr};
  const int r = launch_frames(h, *w, call);
  if (r == VOFOD_OK)
    *ticket = t;
  return r;
}

int vofod_reserve(vofod_handle* h, int tickets)
{
  if (!h || tickets < 1 || tickets > vofod_handle::MAX_INFLIGHT)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));
  for (int t = 0; t < tickets; t++)
  {
    Workspace* w = h->slot(t);
    if (w->F == 0)
      VCHK(grow_workspace(h, *w, "extra workspace: ", h->ws.F, h->ws.pt_cap, h->ws.vox_cap, h->ws.words_cap, h->ws.bricks_cap));
    VCHK(ensure_chain_stream(h, t));
  }
  // the device tail's flood-fill buffers: shared by the batches of 128 frames and more (their tails take turns on the tail
  // stream), per ticket for smaller batches (launch_device_tail sizes those by the batch; reserved here for full workspaces)
  VCHK(ensure_explore(h, h->explore, h->ws.F, static_cast<size_t>(h->ws.F) * vtd::TP_MAXC, static_cast<size_t>(h->ws.F) * vtd::TP_MAXM));
  if (h->ws.F < 128u)
    for (int t = 0; t < tickets; t++)
      VCHK(ensure_explore(h, h->explore_slot[t], h->ws.F, static_cast<size_t>(h->ws.F) * vtd::TP_MAXC, static_cast<size_t>(h->ws.F) * vtd::TP_MAXM));
  return VOFOD_OK;
}

int vofod_batch_collect(vofod_handle* h, int ticket, vofod_detection* out, size_t cap, uint32_t* n_out_per_frame, size_t* n_out)
{
  if (!h || !n_out || ticket < 0 || ticket >= vofod_handle::MAX_INFLIGHT)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));
  Workspace& w = *h->slot(ticket);
  if (!w.pending)
    return VOFOD_ERR_NOT_PENDING;
  *n_out = 0;
  auto collect = [&] {  // (the inputs as the launch half left them in the workspace)
    FrameCall call{true, nullptr, w.job_tfs.data(), w.job_n, VOFOD_SCAN_NO_MAP_UPDATE, nullptr, &w.job_dp, w.job_g};
    return collect_frames(h, w, call, out, cap, n_out_per_frame, n_out);
  };
  // (a batch that has to run again is enqueued from the submitted descriptors)
  auto again = [&] {
    FrameCall call{true, w.job_scans.data(), w.job_tfs.data(), w.job_n, VOFOD_SCAN_NO_MAP_UPDATE, nullptr};
    const int r = launch_frames(h, w, call);
    return r != VOFOD_OK ? r : collect();
  };
  return with_reruns(collect, again);
}

// One scan through one input step of the batch path: staged into frame slot 0 of the synchronous workspace (stage_inputs refuses
// device columns whose base or stride is no multiple of 4), `step` (decode_ranges or deskew_points: one job of its kernel), the
// slot's three packed columns copied out, one synchronisation.
static int one_scan_step(vofod_handle* h, const vofod_scan* scan, int (*step)(vofod_handle*, Workspace&, size_t), float* x, float* y, float* z, int32_t out_memspace)
{
  Workspace& ws = h->ws;
  const size_t npts = static_cast<size_t>(scan->width) * scan->height;
  const float tf[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  bool host_copies = false;
  VCHK(stage_inputs(h, ws, scan, tf, 1, npts, host_copies));
  VCHK(step(h, ws, npts));
  float* out[3] = {x, y, z};
  for (int c = 0; c < 3; c++)
    HIPCHK(hipMemcpyAsync(out[c], ws.d_stage + static_cast<size_t>(c) * ws.pt_cap, npts * sizeof(float), out_memspace == VOFOD_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                          h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VOFOD_OK;
}

int vofod_range_to_points(vofod_handle* h, const vofod_scan* scan, float* x, float* y, float* z, int32_t out_memspace)
{
  if (!h || !scan || !x || !y || !z || !is_range_image(*scan) || (out_memspace != VOFOD_MEM_HOST && out_memspace != VOFOD_MEM_DEVICE) ||
      (scan->memspace != VOFOD_MEM_HOST && scan->memspace != VOFOD_MEM_DEVICE))
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  if (scan->height != h->sp.sensor_vrays || scan->width != h->sp.sensor_hrays)
    return VOFOD_ERR_SIZE_MISMATCH;
  VCHK(check_col_tfs(h, *scan));
  VCHK(admit(h, WS0_FREE));
  // (range_decode.h: one job, launched as k_range_decode, or as k_range_decode_motion for a scan with col_tfs)
  return one_scan_step(h, scan, decode_ranges, x, y, z, out_memspace);
}

// The compensated cloud of ONE point scan with col_tfs, by the route the batch takes: staged into frame slot 0 of the synchronous
// workspace, one job of k_point_deskew, the slot's packed columns copied out.  Needs no switch (vofod_set_point_motion admits such
// scans to the per-scan entry points; this call is what they would see).
int vofod_deskew_points(vofod_handle* h, const vofod_scan* scan, float* x, float* y, float* z, int32_t out_memspace)
{
  if (!h || !scan || !x || !y || !z || !scan->x || !scan->y || !scan->z || !scan->col_tfs || (out_memspace != VOFOD_MEM_HOST && out_memspace != VOFOD_MEM_DEVICE) ||
      (scan->memspace != VOFOD_MEM_HOST && scan->memspace != VOFOD_MEM_DEVICE))
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  if (scan->height != h->sp.sensor_vrays || scan->width != h->sp.sensor_hrays)
    return VOFOD_ERR_SIZE_MISMATCH;
  if (scan->memspace == VOFOD_MEM_DEVICE && reinterpret_cast<uintptr_t>(scan->col_tfs) % 4 != 0)
  {
    h->err = "device-resident col_tfs: the table must be 4-byte aligned";
    return VOFOD_ERR_INVALID_ARG;
  }
  VCHK(admit(h, WS0_FREE));
  return one_scan_step(h, scan, deskew_points, x, y, z, out_memspace);
}

// A handle property, as the column shifts: off after vofod_create, kept across vofod_reset, vofod_map_apply and vofod_map_shift.
int vofod_set_point_motion(vofod_handle* h, int on)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h, ApiLock::LOCK_ONLY);
  VCHK(admit(h, WS0_FREE | MAP_UNREAD));
  h->point_motion = on != 0;
  return VOFOD_OK;
}

// A sensor property: the measurement column of pixel (row, col) is (col + shift_by_row[row]) mod width.  The device table holds the
// shifts reduced to [0, width), so the kernel's mod is one compare.
int vofod_set_column_shift(vofod_handle* h, const int32_t* shift_by_row)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE | MAP_UNREAD));  // (a batch in flight may not have run its decode yet)
  const int64_t w = h->sp.sensor_hrays;
  std::vector<uint32_t> red(static_cast<size_t>(std::max(h->sp.sensor_vrays, 1)), 0u);
  if (shift_by_row && w > 0)
    for (int32_t r = 0; r < h->sp.sensor_vrays; r++)
      red[r] = static_cast<uint32_t>(((static_cast<int64_t>(shift_by_row[r]) % w) + w) % w);
  HIPCHK(hipMemcpyAsync(h->d_col_shift, red.data(), sizeof(uint32_t) * red.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VOFOD_OK;
}

int vofod_detection_points(vofod_handle* h, int source, vofod_detection_extent* ext, size_t ext_cap, size_t* n_ext, vofod_point_xyzr* points, uint32_t* index, size_t points_cap, size_t* n_points,
                           int32_t points_memspace)
{
  if (!h || !n_ext || !n_points || source < VOFOD_POINTS_SYNC || source >= vofod_handle::MAX_INFLIGHT || (points_memspace != VOFOD_MEM_HOST && points_memspace != VOFOD_MEM_DEVICE) ||
      (index && !points))
    return VOFOD_ERR_INVALID_ARG;
  if (points_memspace == VOFOD_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(index)) & 3))
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));
  const int t = source == VOFOD_POINTS_SYNC ? 0 : source;
  Workspace& ws = *h->slot(t);
  if (!ws.det_valid || ws.det_submitted != (source != VOFOD_POINTS_SYNC))
    return VOFOD_ERR_NOT_PENDING;
  // counts and offsets: known on the host from the collected detections
  const size_t n = ws.det_refs.size();
  std::vector<vdp::DetDesc> descs(n);
  size_t total = 0;
  for (size_t i = 0; i < n; i++)
  {
    const Workspace::DetRef& r = ws.det_refs[i];
    descs[i] = vdp::DetDesc{r.frame, r.root, static_cast<uint32_t>(total), r.n_points};
    total += r.n_points;
  }
  *n_ext = n;
  *n_points = total;
  if (!ext && !points)
    return VOFOD_OK;  // size query
  if ((ext && ext_cap < n) || (points && points_cap < total))
    return VOFOD_ERR_CAPACITY;
  if (n == 0)
    return VOFOD_OK;
  if (total > 0xffffffffull)
  {
    h->err = "detection points: more than 2^32 member voxels";
    return VOFOD_ERR_DEVICE;
  }
  // on the workspace's own chain stream (everything that wrote the workspace has been waited for by its collect half)
  VCHK(ensure_chain_stream(h, t));
  StreamScope scope(h, h->chain_stream[t]);
  HIPCHK(ws.d_detdesc.reserve(n));
  HIPCHK(ws.d_detbox.reserve(n));
  HIPCHK(ws.d_detpts.reserve(total));
  HIPCHK(ws.d_detidx.reserve(total));
  std::vector<vdp::DetBox> boxes(n);
  HIPCHK(hipMemcpyAsync(ws.d_detdesc, descs.data(), sizeof(vdp::DetDesc) * n, hipMemcpyHostToDevice, h->stream));
  KLAUNCH(h, vdp::k_det_points, dim3(static_cast<uint32_t>(n)), dim3(vdp::DP_THREADS), ws.d_hdrs, ws.d_cand, ws.va.pts, ws.det_vox_cap, ws.d_detdesc, ws.d_detpts, ws.d_detidx, ws.d_detbox);
  HIPCHK(hipMemcpyAsync(boxes.data(), ws.d_detbox, sizeof(vdp::DetBox) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < n; i++)
    if (boxes[i].found != descs[i].n_points)
    {
      h->err = "detection points: detection " + std::to_string(ws.det_refs[i].id) + " has " + std::to_string(descs[i].n_points) + " points, its cluster " + std::to_string(boxes[i].found) +
               " entries in the frame's member list";
      return VOFOD_ERR_DEVICE;
    }
  // (the staging buffers are 16-byte aligned for the kernel's stores; the caller's need not be)
  static_assert(sizeof(vofod_point_xyzr) == sizeof(float4), "a voxel record is a vofod_point_xyzr");
  const hipMemcpyKind kind = points_memspace == VOFOD_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (points && total)
    HIPCHK(hipMemcpyAsync(points, ws.d_detpts, sizeof(float4) * total, kind, h->stream));
  if (index && total)
    HIPCHK(hipMemcpyAsync(index, ws.d_detidx, sizeof(uint32_t) * total, kind, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t i = 0; ext && i < n; i++)
  {
    vofod_detection_extent& e = ext[i];
    e.id = ws.det_refs[i].id;
    e.frame = ws.det_refs[i].frame;
    e.first = descs[i].first;
    e.count = descs[i].n_points;
    for (int a = 0; a < 3; a++)
    {
      e.aabb_min[a] = boxes[i].aabb_min[a];
      e.aabb_max[a] = boxes[i].aabb_max[a];
    }
  }
  return VOFOD_OK;
}

int vofod_detection_pixels(vofod_handle* h, int source, vofod_detection_span* span, size_t span_cap, size_t* n_span, uint32_t* pixels, uint32_t* member, float* xyz, size_t pixels_cap,
                           size_t* n_pixels, int32_t memspace)
{
  if (!h || !n_span || !n_pixels || source < VOFOD_POINTS_SYNC || source >= vofod_handle::MAX_INFLIGHT || (memspace != VOFOD_MEM_HOST && memspace != VOFOD_MEM_DEVICE) ||
      ((member || xyz) && !pixels))
    return VOFOD_ERR_INVALID_ARG;
  if (memspace == VOFOD_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(pixels) | reinterpret_cast<uintptr_t>(member) | reinterpret_cast<uintptr_t>(xyz)) & 3))
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));
  const int t = source == VOFOD_POINTS_SYNC ? 0 : source;
  Workspace& ws = *h->slot(t);
  if (!ws.det_valid || ws.det_submitted != (source != VOFOD_POINTS_SYNC))
    return VOFOD_ERR_NOT_PENDING;
  const size_t n = ws.det_refs.size();
  *n_span = n;
  *n_pixels = 0;
  if (n == 0)
    return VOFOD_OK;  // (no detections: no launch, whatever was asked)
  // on the workspace's own chain stream (everything that wrote the workspace has been waited for by its collect half)
  VCHK(ensure_chain_stream(h, t));
  StreamScope scope(h, h->chain_stream[t]);
  std::vector<vpx::PixDesc> descs(n);
  size_t members = 0;
  for (size_t i = 0; i < n; i++)
  {
    const Workspace::DetRef& r = ws.det_refs[i];
    descs[i] = vpx::PixDesc{r.frame, r.root, r.n_points, static_cast<uint32_t>(members), 0u, 0u, {0u, 0u}};
    members += r.n_points;
  }
  if (members > 0xffffffffull)
  {
    h->err = "detection pixels: more than 2^32 member voxels";
    return VOFOD_ERR_DEVICE;
  }
  HIPCHK(ws.d_pxdesc.reserve(n));
  // ---- the counts: the sizing kernel, once per validity (the record builders clear what it found)
  if (ws.det_px_sizes.size() != n)
  {
    std::vector<vpx::PixSize> sizes(n);
    HIPCHK(ws.d_pxsize.reserve(n));
    HIPCHK(hipMemcpyAsync(ws.d_pxdesc, descs.data(), sizeof(vpx::PixDesc) * n, hipMemcpyHostToDevice, h->stream));
    KLAUNCH(h, vpx::k_det_pixel_sizes, dim3(static_cast<uint32_t>(n)), dim3(vpx::PX_THREADS), ws.d_hdrs, ws.d_cand, ws.va.pts, ws.det_vox_cap, ws.d_pxdesc, ws.d_pxsize);
    HIPCHK(hipMemcpyAsync(sizes.data(), ws.d_pxsize, sizeof(vpx::PixSize) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; i++)
      if (sizes[i].members != descs[i].n_points)
      {
        h->err = "detection pixels: detection " + std::to_string(ws.det_refs[i].id) + " has " + std::to_string(descs[i].n_points) + " points, its cluster " + std::to_string(sizes[i].members) +
                 " entries in the frame's member list";
        return VOFOD_ERR_DEVICE;
      }
    ws.det_px_sizes = std::move(sizes);
  }
  size_t total = 0;
  for (size_t i = 0; i < n; i++)
  {
    descs[i].first = static_cast<uint32_t>(total);
    descs[i].count = ws.det_px_sizes[i].count;
    total += descs[i].count;
  }
  *n_pixels = total;
  if (!span && !pixels)
    return VOFOD_OK;  // size query
  if ((span && span_cap < n) || (pixels && pixels_cap < total))
    return VOFOD_ERR_CAPACITY;
  if (total > 0xffffffffull)
  {
    h->err = "detection pixels: more than 2^32 returns";
    return VOFOD_ERR_DEVICE;
  }
  if (pixels)
  {
    // ---- the walk, into the workspace's staging buffers (16-byte aligned; the caller's need not be)
    HIPCHK(ws.d_pxfound.reserve(n));
    HIPCHK(ws.d_pxkey.reserve(members));
    HIPCHK(ws.d_pxrank.reserve(members));
    HIPCHK(ws.d_pxidx.reserve(total));
    HIPCHK(ws.d_pxmember.reserve(total));
    HIPCHK(ws.d_pxxyz.reserve(3 * total));
    std::vector<vpx::PixFound> found(n);
    HIPCHK(hipMemcpyAsync(ws.d_pxdesc, descs.data(), sizeof(vpx::PixDesc) * n, hipMemcpyHostToDevice, h->stream));
    KLAUNCH(h, vpx::k_det_pixels, dim3(static_cast<uint32_t>(n)), dim3(vpx::PX_THREADS), ws.d_args, ws.det_g, ws.d_hdrs, ws.d_cand, ws.va.pts, ws.det_vox_cap, ws.d_pxdesc, ws.d_pxkey, ws.d_pxrank,
            ws.d_pxidx, ws.d_pxmember, ws.d_pxxyz, ws.d_pxfound);
    HIPCHK(hipMemcpyAsync(found.data(), ws.d_pxfound, sizeof(vpx::PixFound) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; i++)
      if (found[i].members != descs[i].n_points || found[i].bad || found[i].pixels != descs[i].count)
      {
        const std::string who = "detection pixels: detection " + std::to_string(ws.det_refs[i].id) + " (frame " + std::to_string(ws.det_refs[i].frame) + ")";
        if (found[i].members != descs[i].n_points)
          h->err = who + " has " + std::to_string(descs[i].n_points) + " points, its cluster " + std::to_string(found[i].members) + " entries in the frame's member list";
        else if (found[i].bad)
          h->err = who + ": " + std::to_string(found[i].bad) + " member centres are no cell centres of the frame's lattice";
        else
          h->err = who + ": its member voxels weigh " + std::to_string(descs[i].count) + " returns, the frame's columns hold " + std::to_string(found[i].pixels) +
                   " (were device-resident columns changed since the scan ran?)";
        return VOFOD_ERR_DEVICE;
      }
    const hipMemcpyKind kind = memspace == VOFOD_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (total)
    {
      HIPCHK(hipMemcpyAsync(pixels, ws.d_pxidx, sizeof(uint32_t) * total, kind, h->stream));
      if (member)
        HIPCHK(hipMemcpyAsync(member, ws.d_pxmember, sizeof(uint32_t) * total, kind, h->stream));
      if (xyz)
        HIPCHK(hipMemcpyAsync(xyz, ws.d_pxxyz, sizeof(float) * 3 * total, kind, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
  }
  for (size_t i = 0; span && i < n; i++)
    span[i] = vofod_detection_span{ws.det_refs[i].id, ws.det_refs[i].frame, descs[i].first, descs[i].count};
  return VOFOD_OK;
}

}  // extern "C"
