// Launch half of the per-scan entry points (included by vofod_hip.hip): the body of processMsg (vofod_nodelet.cpp:926-965)
// for n frames up to the point where the host has to wait - inputs staged, kernel chain and read-back enqueued.
#pragma once

namespace
{

// One call of a per-scan entry point: its inputs, and what the launch half leaves for the collect half of the SAME call and
// nobody else needs.  Owned by the entry point, which fills the inputs; vofod_batch_collect fills one from the ticket.
struct FrameCall
{
  bool submitted;  // vofod_batch_submit / vofod_batch_collect: the two halves run in different API calls
  const vofod_scan* scans;
  const float* tfs;
  uint32_t n;
  int flags;
  vofod_scan_debug* dbg;
  // A submitted batch is classified with the dynamic parameters of its submission: vofod_set_dynamic_params may be called
  // between submit and collect (DetectionParams.cfg semantics: "between any two calls"), and the collect half (position sigma,
  // min_points, the host fall-back tail) as well as the re-run of an overflowed batch must not mix the two parameter sets.
  const vofod_dyn_params* dp = nullptr;
  GridParams g{};
  bool rc_done = false;     // ++its and the raycast role of VOFOD_SCAN_AUTO_RAYCAST have run ahead of the device tail
  hipStream_t tail_stream_used = nullptr;  // where the device tail's last operation was enqueued
  DevEvent ev[5];  // debug output: stage boundaries on the chain's stream
  clk::time_point t0 = clk::now();
  double tr_launch = 0, tr_sync1 = 0;  // VOFOD_TRACE
};

// Which streams a launch takes (route_submitted): what differs between a submitted and a synchronous launch.  Which kernels it runs is
// the plan's (chain_plan.h).
struct LaunchRoute
{
  bool staged = false;            // submitted, 128 frames and more: three-stage pipeline on the streaming / frame / tail streams
  hipStream_t chain = nullptr;    // submitted: the stream of the chain (the ticket's own, or the streaming stage's); nullptr: the handle's
  int own_tail = -1;              // submitted small batch: the ticket whose stream and flood-fill buffers the device tail takes
};

// h->stream names the stream every KLAUNCH goes to.  A scope that sends the launches elsewhere (or moves h->stream itself
// further down) puts it back on every return path.
struct StreamScope
{
  vofod_handle* h;
  hipStream_t saved;
  explicit StreamScope(vofod_handle* h_, hipStream_t st = nullptr) : h(h_), saved(h_->stream)
  {
    if (st)
      h->stream = st;
  }
  ~StreamScope() { h->stream = saved; }
};

// the chain streams of tickets 4-7 are created when the ticket is first taken (vofod_create has made those of tickets 0-3)
int ensure_chain_stream(vofod_handle* h, int t)
{
  if (!h->chain_stream[t])
    HIPCHK(h->chain_stream[t].create(hipStreamCreateWithFlags, hipStreamNonBlocking));
  return VOFOD_OK;
}

// which in-flight slot is `ws` (-1: not a ticket's workspace)
int slot_index(vofod_handle* h, const Workspace& ws)
{
  for (int t = 0; t < vofod_handle::MAX_INFLIGHT; t++)
    if (&ws == h->slot(t))
      return t;
  return -1;
}

inline bool trace_on()
{
  static const bool v = std::getenv("VOFOD_TRACE") != nullptr;
  return v;
}

// nVoxelsOver as findCloseFarClusters saw it (:715) and the background latch (:716-721).  (n_bg_voxels is the count of the map
// BEFORE this call's update; counters patched by this very call - bgcount_stale - belong to the next one and are not fetched here)
int latch_background(vofod_handle* h)
{
  if (h->bgcount_fresh)
  {
    if (h->ev_bgcount)
      HIPCHK(hipEventSynchronize(h->ev_bgcount));  // the copy may have been enqueued on another chain's stream
    uint64_t t = 0;
    for (int i = 0; i < MB_SLOTS; i++)
      t += h->h_bgcount[8 * i];
    h->n_bg_voxels = t;
    h->bgcount_fresh = false;
  }
  if (h->n_bg_voxels > h->background_min_sufficient_pts)
    h->background_pts_sufficient = true;
  return VOFOD_OK;
}

vc::ExploreParams explore_params(const vofod_dyn_params& dp, float thr_new, bool no_update)
{
  vc::ExploreParams ep{};
  ep.thr_unknown = static_cast<float>(dp.voxel_map__thresholds__frontiers);
  ep.thr_ground = thr_new;
  ep.frontier_value = static_cast<float>(dp.voxel_map__thresholds__frontiers);
  ep.ray_score = dp.voxel_map__scores__ray;
  ep.no_update = no_update ? 1 : 0;
  ep.stack_cap = vc::EX_CELLS;
  return ep;
}

// the gates' parameters (classify_cluster :1648-1696) as the device tail and the host tail take them
vt::TailParams tail_params(const vofod_handle* h, const vofod_dyn_params& dp)
{
  vt::TailParams tp{};
  tp.min_points = dp.classification__min_points;
  tp.max_distance = dp.classification__max_distance;
  tp.max_size = dp.classification__max_size;
  tp.max_explore = dp.classification__max_explore_distance;
  tp.voxel_size = h->sp.voxel_size;
  tp.latches = (h->background_pts_sufficient && h->sure_background_sufficient) ? 1 : 0;
  return tp;
}

// read-back of the full tables: header, speculative cluster records and candidate members of every frame
int read_back_full(vofod_handle* h, Workspace& ws, const GridParams& g, uint32_t n)
{
  KLAUNCH(h, k_pack, fgrid(g, (std::max(SPEC_C, SPEC_M) + 255) / 256), dim3(256), g, ws.d_hdrs, ws.d_table, ws.d_cand, ws.va, ws.d_packed);
  HIPCHK(hipMemcpyAsync(ws.h_packed, ws.d_packed, sizeof(PackedFrame) * n, hipMemcpyDeviceToHost, h->stream));
  return VOFOD_OK;
}

// ---- routing of a submitted launch: which stream its chain takes, where its tail goes
// In-flight batches on streams of their own overlap their kernel chains: a gain while a batch leaves CUs idle (32 / 64 /
// 128 frames: +31 / +56 / +16 %), a loss once one batch's kernels fill the chip (256 frames: -6 %, co-running chains only
// slow each other down).
// Round 2: the chains are staggered.  A batch's streaming kernels (bounding box, brick codes: HBM bound, a few waves per CU)
// start when the previous batch's have finished, i.e. while that batch's frame kernel (LDS bound, one workgroup per CU)
// runs: the two phases of consecutive batches share the chip instead of taking turns.
// (Rounds 2-3 kept VOFOD_TWO_CHAINS / VOFOD_STAGGER / VOFOD_PIPE / VOFOD_FRAME_STREAMS to switch these schemes off: lost
// experiments, removed in round 4 with their code paths - DESIGN 5.3 has the measurements.)
// Submitted batches run as a three-stage pipeline on three streams: the streaming kernels (bounding box + brick codes:
// vector-instruction bound, a few waves per CU) of every batch on a low-priority stream, the frame kernels (one 156 KB
// workgroup per CU, latency bound) on a second one, the classification tails on a third (high priority).  The streaming
// kernels of batch k+1 then fill the issue slots the frame kernel of batch k leaves idle, and when both are ready at the
// same moment the frame kernel's workgroups are placed first (a CU full of streaming waves has no room for one).
int route_submitted(vofod_handle* h, const Workspace& ws, uint32_t n, LaunchRoute& rt)
{
  // (a batch that leaves most CUs idle - fewer frames than half the CUs - gains more from whole chains running side by
  // side: its frame kernel shares the chip with the frame kernels of the other batches in flight)
  if (!h->stream_key || !h->stream_frame || n < 128u)
  {
    const int t = slot_index(h, ws);
    if (t >= 1)
    {
      VCHK(ensure_chain_stream(h, t));
      rt.chain = h->chain_stream[t];
    }
    // A small submitted batch (fewer frames than half the CUs: its whole chain runs on the ticket's stream) keeps flood-fill
    // buffers of its own and its tail on that stream: the tails of the batches in flight overlap.  On the shared tail stream
    // they took turns - k_tail_prep + k_explore + k_tail_finish last 250-280 us in the company of other batches' frame kernels
    // (120 us alone), and that turn WAS the pace of 32-frame batches (device timeline, tools/trace32.sh).
    if (n < 128u)
      rt.own_tail = t;
  }
  else
  {
    rt.chain = h->stream_key;
    rt.staged = true;
  }
  return VOFOD_OK;
}

// a range image (include/vofod.h): no point columns, only the sensor's range column
inline bool is_range_image(const vofod_scan& s) { return !s.x && !s.y && !s.z && s.range; }

// a pose per column (vofod_scan::col_tfs): range images, and point scans once vofod_set_point_motion has switched them on; a
// device-resident table is read in place with 4-byte loads at least
inline int check_col_tfs(vofod_handle* h, const vofod_scan& s)
{
  if (!s.col_tfs)
    return VOFOD_OK;
  if (!is_range_image(s) && !h->point_motion)
  {
    h->err = "col_tfs: only a range image (x == y == z == NULL) may carry a pose per column unless vofod_set_point_motion is on";
    return VOFOD_ERR_INVALID_ARG;
  }
  if (s.memspace == VOFOD_MEM_DEVICE && reinterpret_cast<uintptr_t>(s.col_tfs) % 4 != 0)
  {
    h->err = "device-resident col_tfs: the table must be 4-byte aligned";
    return VOFOD_ERR_INVALID_ARG;
  }
  return VOFOD_OK;
}

// Slot k of the workspace's pose block (F tables of width * 12 floats, allocated on the first use); a host table `src` is copied
// there on `st` (nullptr: the caller copies).
int pose_slot(vofod_handle* h, Workspace& ws, size_t k, const float* src, hipStream_t st, float*& slot)
{
  const size_t tab = static_cast<size_t>(h->sp.sensor_hrays) * 12;  // floats per table
  if (!ws.d_poses)
    HIPCHK(ws.d_poses.alloc(static_cast<size_t>(ws.F) * tab));
  slot = ws.d_poses + k * tab;
  if (src)
    HIPCHK(hipMemcpyAsync(slot, src, tab * sizeof(float), hipMemcpyHostToDevice, st));
  return VOFOD_OK;
}

// Pose tables of the batch's scans with col_tfs - the motion jobs of the range list (its first n_mjobs) and the point jobs, each list
// in frame order: device-resident tables are read where they lie, host-resident ones go to the workspace's pose block - the k-th host
// table of the batch into slot k, whichever list its job is in - with ONE 2-D copy when they lie at a constant pitch (one numpy block
// per batch), otherwise one copy each.  On the stream of the staging copies, in front of the event vofod_batch_submit waits for: the
// caller may overwrite its tables when submit returns.
int stage_pose_tables(vofod_handle* h, Workspace& ws, const vofod_scan* scans, uint32_t n)
{
  const size_t tab = static_cast<size_t>(h->sp.sensor_hrays) * 12;  // floats per table
  std::vector<const float*> host;                                     // the host tables, and the job entry each belongs to
  std::vector<const float**> entry_of;
  uint32_t jm = 0, jp = 0;
  for (uint32_t f = 0; f < n; f++)
  {
    if (!scans[f].col_tfs)
      continue;
    const float** entry = is_range_image(scans[f]) ? &ws.h_rjobs.p[jm++].poses : &ws.h_pjobs.p[jp++].poses;
    if (scans[f].memspace != VOFOD_MEM_DEVICE)
    {
      host.push_back(scans[f].col_tfs);
      entry_of.push_back(entry);
    }
  }
  if (host.empty())
    return VOFOD_OK;
  const ptrdiff_t pitch = host.size() >= 2 ? reinterpret_cast<const char*>(host[1]) - reinterpret_cast<const char*>(host[0]) : 0;
  bool constant = pitch >= static_cast<ptrdiff_t>(tab * sizeof(float));
  for (size_t k = 2; k < host.size() && constant; k++)
    constant = reinterpret_cast<const char*>(host[k]) == reinterpret_cast<const char*>(host[0]) + static_cast<ptrdiff_t>(k) * pitch;
  for (size_t k = 0; k < host.size(); k++)
  {
    float* slot = nullptr;
    VCHK(pose_slot(h, ws, k, constant ? nullptr : host[k], h->stream, slot));
    *entry_of[k] = slot;
  }
  if (constant)
    HIPCHK(hipMemcpy2DAsync(ws.d_poses, tab * sizeof(float), host[0], static_cast<size_t>(pitch), tab * sizeof(float), host.size(), hipMemcpyHostToDevice, h->stream));
  return VOFOD_OK;
}

// the device copy of the pose table of the call's FIRST scan as stage_inputs left it in the workspace (a range image's or a point
// scan's); nullptr when the scan has none.  A re-run keeps that of its first launch.
inline const float* staged_pose_table(const Workspace& ws, const vofod_scan& s) { return s.col_tfs ? ws.first_poses : nullptr; }

// ---- stage inputs (filterAndTransform :621-684 reads them)
// (the re-run of a batch that overflowed the LDS kernels keeps the frame arguments and the staged columns of its first
// launch: the caller's host buffers need not outlive vofod_batch_submit)
// Host-resident batches whose frames are packed x | y | z columns at a constant pitch (one pcl / numpy block per batch, or
// per-frame blocks of one arena) cross PCIe with ONE 2-D copy command instead of three per frame: at 256 frames the 768
// copy calls alone cost more host time than the whole device chain.  The copy is enqueued on the streaming stage's stream:
// it overlaps the frame kernel and the tail of the batches in front.  (Pinned memory makes it asynchronous; a pageable
// source is staged by the runtime and blocks the call.)
// host_copies: some column came from host memory.
int stage_inputs(vofod_handle* h, Workspace& ws, const vofod_scan* scans, const float* tfs, uint32_t n, size_t npts, bool& host_copies)
{
  bool staged_2d = false;
  ws.det_valid = false;  // (the workspace is taken: what vofod_detection_points answered from is about to be overwritten)
  ws.n_rjobs = ws.n_mjobs = ws.n_pjobs = 0;
  ws.first_poses = nullptr;
  // the range images of the batch, in frame order for now (a pose table: the caller's, for now)
  vrd::RangeJob* const jobs = ws.h_rjobs.p;
  uint32_t n_jobs = 0;
  // ... and its point scans with a pose per column, in frame order
  vpd::PointJob* const pjobs = ws.h_pjobs.p;
  uint32_t n_pjobs = 0;
  auto slot = [&](uint32_t f) { return ws.d_stage + static_cast<size_t>(f) * ws.pt_cap * 5; };
  // the frame's arguments point at the packed x | y | z columns of its staging slot (copied there, or decoded there by k_range_decode)
  auto slot_args = [&](uint32_t f) {
    float* base = slot(f);
    return stage_cloud(h, ws, f, base, base + ws.pt_cap, base + 2 * static_cast<size_t>(ws.pt_cap), nullptr, nullptr, 4, npts, VOFOD_MEM_DEVICE, FA_SCAN, tfs + 12 * f);
  };
  if (n >= 2 && scans[0].memspace == VOFOD_MEM_HOST && scans[0].x)
  {
    const char* x0 = static_cast<const char*>(scans[0].x);
    const ptrdiff_t pitch = static_cast<const char*>(scans[1].x) - x0;
    bool ok = pitch >= static_cast<ptrdiff_t>(npts * 12);
    for (uint32_t f = 0; f < n && ok; f++)
    {
      const vofod_scan& s = scans[f];
      const char* xf = x0 + static_cast<ptrdiff_t>(f) * pitch;
      ok = s.memspace == VOFOD_MEM_HOST && s.stride_bytes == 4 && static_cast<const char*>(s.x) == xf && static_cast<const char*>(s.y) == xf + npts * 4 &&
           static_cast<const char*>(s.z) == xf + npts * 8;
    }
    if (ok && ws.pt_cap == npts)
    {
      HIPCHK(hipMemcpy2DAsync(ws.d_stage, sizeof(float) * 5 * ws.pt_cap, x0, static_cast<size_t>(pitch), npts * 12, n, hipMemcpyHostToDevice, h->stream));
      for (uint32_t f = 0; f < n; f++)
      {
        VCHK(slot_args(f));
        if (scans[f].col_tfs)  // k_point_deskew works in place over the slot
          pjobs[n_pjobs++] = vpd::PointJob{ws.h_args[f].x, ws.h_args[f].y, ws.h_args[f].z, slot(f), 4, scans[f].col_tfs};
      }
      staged_2d = true;
    }
  }
  // Host-resident range images at a constant pitch (one uint32 column per frame, 4 B per point: a third of the x | y | z block)
  // cross the link the same way, with ONE 2-D copy into column 4 of the slots; k_range_decode rebuilds columns 0-2 from there.
  if (n >= 2 && scans[0].memspace == VOFOD_MEM_HOST && is_range_image(scans[0]))
  {
    const char* r0 = static_cast<const char*>(scans[0].range);
    const ptrdiff_t pitch = static_cast<const char*>(scans[1].range) - r0;
    bool ok = pitch >= static_cast<ptrdiff_t>(npts * 4);
    for (uint32_t f = 0; f < n && ok; f++)
    {
      const vofod_scan& s = scans[f];
      ok = s.memspace == VOFOD_MEM_HOST && is_range_image(s) && s.stride_bytes == 4 && static_cast<const char*>(s.range) == r0 + static_cast<ptrdiff_t>(f) * pitch;
    }
    if (ok)
    {
      HIPCHK(hipMemcpy2DAsync(ws.d_stage + 4 * static_cast<size_t>(ws.pt_cap), sizeof(float) * 5 * ws.pt_cap, r0, static_cast<size_t>(pitch), npts * 4, n, hipMemcpyHostToDevice, h->stream));
      for (uint32_t f = 0; f < n; f++)
      {
        VCHK(slot_args(f));
        jobs[n_jobs++] = vrd::RangeJob{reinterpret_cast<const char*>(slot(f) + 4 * static_cast<size_t>(ws.pt_cap)), slot(f), 4, scans[f].col_tfs};
      }
      staged_2d = true;
    }
  }
  host_copies = staged_2d;
  for (uint32_t f = 0; f < n && !staged_2d; f++)
  {
    const vofod_scan& s = scans[f];
    host_copies |= s.memspace != VOFOD_MEM_DEVICE;
    if (!is_range_image(s))
    {
      VCHK(stage_cloud(h, ws, f, s.x, s.y, s.z, nullptr, nullptr, s.stride_bytes, npts, s.memspace, FA_SCAN, tfs + 12 * f));
      if (!s.col_tfs)
        continue;
      // a point scan with poses: k_point_deskew reads the columns where stage_cloud has left them for the kernels - the caller's
      // device memory, the struct block of a host scan, the slot itself - and writes the packed columns of the slot, which the
      // frame's arguments point at from here on
      if (s.memspace == VOFOD_MEM_DEVICE &&
          (s.stride_bytes % 4 != 0 || (reinterpret_cast<uintptr_t>(s.x) | reinterpret_cast<uintptr_t>(s.y) | reinterpret_cast<uintptr_t>(s.z)) % 4 != 0))
      {
        h->err = "device-resident point scan with col_tfs: the columns' bases and stride must be multiples of 4 bytes";
        return VOFOD_ERR_INVALID_ARG;
      }
      const FrameArgs& a = ws.h_args[f];
      pjobs[n_pjobs++] = vpd::PointJob{a.x, a.y, a.z, slot(f), a.stride, s.col_tfs};
      VCHK(slot_args(f));
      continue;
    }
    // a range image: device-resident ranges are read where they lie, a host column goes to column 4 of the slot (gathered when strided)
    vrd::RangeJob job{static_cast<const char*>(s.range), slot(f), s.stride_bytes, s.col_tfs};
    if (s.memspace != VOFOD_MEM_DEVICE)
    {
      VCHK(stage_host_column(h, slot(f) + 4 * static_cast<size_t>(ws.pt_cap), s.range, s.stride_bytes, npts));
      job.src = reinterpret_cast<const char*>(slot(f) + 4 * static_cast<size_t>(ws.pt_cap));
      job.stride = 4;
    }
    else if (s.stride_bytes % 4 != 0 || reinterpret_cast<uintptr_t>(s.range) % 4 != 0)
    {
      h->err = "device-resident range column: base and stride must be multiples of 4 bytes";
      return VOFOD_ERR_INVALID_ARG;
    }
    VCHK(slot_args(f));
    jobs[n_jobs++] = job;
  }
  // the jobs with a pose per column first (k_range_decode_motion's span), those without behind them (k_range_decode's), each kind
  // still in frame order; the whole list goes up with one copy
  ws.n_mjobs = static_cast<uint32_t>(std::stable_partition(jobs, jobs + n_jobs, [](const vrd::RangeJob& job) { return job.poses != nullptr; }) - jobs);
  ws.n_rjobs = n_jobs - ws.n_mjobs;
  ws.n_pjobs = n_pjobs;
  if (ws.n_mjobs || n_pjobs)
    VCHK(stage_pose_tables(h, ws, scans, n));
  // (a first scan with a table owns job 0 of its list: the motion jobs lead the range list in frame order)
  ws.first_poses = !scans[0].col_tfs ? nullptr : is_range_image(scans[0]) ? jobs[0].poses : pjobs[0].poses;
  if (n_jobs)
    HIPCHK(hipMemcpyAsync(ws.d_rjobs, jobs, sizeof(vrd::RangeJob) * n_jobs, hipMemcpyHostToDevice, h->stream));
  if (n_pjobs)
    HIPCHK(hipMemcpyAsync(ws.d_pjobs, pjobs, sizeof(vpd::PointJob) * n_pjobs, hipMemcpyHostToDevice, h->stream));
  return VOFOD_OK;
}

// k_point_deskew over the job list stage_inputs left in the workspace: ONE launch per batch on the stream of the staging copies (no
// such frame: no launch), the instantiation chosen by what every job of the batch allows
int deskew_points(vofod_handle* h, Workspace& ws, size_t npts)
{
  if (!ws.n_pjobs || !npts)
    return VOFOD_OK;
  bool vec = npts % 4 == 0 && ws.pt_cap % 4 == 0, pose16 = true;
  for (uint32_t j = 0; j < ws.n_pjobs; j++)
  {
    const vpd::PointJob& job = ws.h_pjobs.p[j];
    vec = vec && job.stride == 4 &&
          (reinterpret_cast<uintptr_t>(job.x) | reinterpret_cast<uintptr_t>(job.y) | reinterpret_cast<uintptr_t>(job.z) | reinterpret_cast<uintptr_t>(job.dst)) % 16 == 0;
    pose16 = pose16 && reinterpret_cast<uintptr_t>(job.poses) % 16 == 0;
  }
  vrd::MotionArgs ma{};
  ma.shift = h->d_col_shift.p;
  ma.width = static_cast<uint32_t>(h->sp.sensor_hrays);
  exclude_box(h, ma.lo, ma.hi);
  const uint32_t n_px = static_cast<uint32_t>(npts), per_block = vpd::PD_THREADS * (vec ? 4u : 1u);
  const dim3 grid((n_px + per_block - 1) / per_block, ws.n_pjobs);
  auto pick = [&](auto v) {
    constexpr bool V = decltype(v)::value;
    return pose16 ? vpd::k_point_deskew_t<V, true> : vpd::k_point_deskew_t<V, false>;  // (aligned tables: fetched through LDS)
  };
  auto kern = vec ? pick(std::true_type{}) : pick(std::false_type{});
  KLAUNCH_AS(h, "k_point_deskew", kern, grid, dim3(vpd::PD_THREADS), ws.d_pjobs.p, n_px, ws.pt_cap, ma);
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// one launch of the decode template over jobs [first, first + n_jobs) of the list stage_inputs left in the workspace (none: no launch)
int decode_span(vofod_handle* h, Workspace& ws, size_t npts, bool motion, uint32_t first, uint32_t n_jobs)
{
  if (!n_jobs)
    return VOFOD_OK;
  bool vec = npts % 4 == 0 && ws.pt_cap % 4 == 0, pose16 = true;
  for (uint32_t j = first; j < first + n_jobs; j++)
  {
    const vrd::RangeJob& job = ws.h_rjobs.p[j];
    vec = vec && job.stride == 4 && reinterpret_cast<uintptr_t>(job.src) % 16 == 0;
    pose16 = pose16 && reinterpret_cast<uintptr_t>(job.poses) % 16 == 0;  // (a plain job has none: stays true, and is not used)
  }
  vrd::MotionArgs ma{};  // (a plain span reads none of it)
  if (motion)
  {
    ma.shift = h->d_col_shift.p;
    ma.width = static_cast<uint32_t>(h->sp.sensor_hrays);
    exclude_box(h, ma.lo, ma.hi);
  }
  // few frames: one per thread keeps every CU busy; many: up to RD_CHUNK_MAX per thread share one read of the LUT
  const uint32_t chunk = std::min(std::max(n_jobs / 16u, 1u), vrd::RD_CHUNK_MAX);
  const uint32_t n_px = static_cast<uint32_t>(npts), threads = vec ? n_px / 4u : n_px;
  const dim3 grid((threads + vrd::RD_THREADS - 1) / vrd::RD_THREADS, (n_jobs + chunk - 1) / chunk);
  // one kernel template (range_decode.h), selected by (vec, motion, pose16), under the profiler name of the span
  auto pick = [&](auto v) {
    constexpr bool V = decltype(v)::value;
    return !motion ? vrd::k_range_decode_t<V, false, true> : pose16 ? vrd::k_range_decode_t<V, true, true> : vrd::k_range_decode_t<V, true, false>;
  };
  auto kern = vec ? pick(std::true_type{}) : pick(std::false_type{});
  KLAUNCH_AS(h, motion ? "k_range_decode_motion" : "k_range_decode", kern, grid, dim3(vrd::RD_THREADS), ws.d_rjobs.p + first, n_jobs, chunk, n_px, ws.pt_cap, h->d_lut_dirs.p, h->d_lut_offs.p, ma);
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// the decode of the batch's range images, on the stream of the staging copies: one launch over the jobs with a pose per column, one
// over those without
int decode_ranges(vofod_handle* h, Workspace& ws, size_t npts)
{
  VCHK(decode_span(h, ws, npts, true, 0, ws.n_mjobs));
  return decode_span(h, ws, npts, false, ws.n_mjobs, ws.n_rjobs);
}

// an error return of the launch half must not leave copies from the caller's buffers in flight
struct H2DGuard
{
  hipEvent_t ev;
  bool armed;
  ~H2DGuard()
  {
    if (armed)
      (void)hipEventSynchronize(ev);
  }
};

// ---- tables and map images of K8/K9 (findCloseFarClusters :703-750): independent of the frames, prepared first
int prepare_map_images(vofod_handle* h, const vofod_dyn_params& dp, float thr_new, bool use_dilated, bool want_bgcount, CloseParams& cpar)
{
  VCHK(ensure_mapbits(h, thr_new));
  // (a sensor stream's patched nVoxelsOver counters - k_finalize_far of the PREVIOUS scan - are fetched here, before this scan's
  // own update is enqueued, and only while the count can still change something: the background latch, the debug output)
  if (want_bgcount)
    VCHK(refresh_bgcount(h));
  if (!h->closetab.valid || h->closetab.max_dist != static_cast<float>(dp.ground_points_max_distance))
  {
    std::vector<CloseRow> crows;
    if (const int r = build_close_rows(static_cast<float>(dp.ground_points_max_distance), h->mg.vs_inv, crows); r != VOFOD_OK)
    {
      h->err = "ground_points_max_distance / voxel_size exceeds the 63-bit window";
      return r;
    }
    HIPCHK(hipMemcpy(h->d_crows, crows.data(), sizeof(CloseRow) * crows.size(), hipMemcpyHostToDevice));
    h->closetab.valid = true;
    h->closetab.max_dist = static_cast<float>(dp.ground_points_max_distance);
    h->closetab.n_rows = static_cast<int>(crows.size());
  }
  cpar = CloseParams{h->closetab.n_rows, thr_new};
  if (use_dilated)
    return ensure_mapclose(h, cpar);
  return VOFOD_OK;
}

// staged pipeline: the chain moves from the streaming stage's stream to a frame stream
int enter_frame_stream(vofod_handle* h, Workspace& ws)
{
  HIPCHK(hipEventRecord(ws.ev_key, h->stream));
  // Consecutive frame kernels alternate between two streams: frame kernel k+1 waits neither for the LAST workgroup of frame
  // kernel k (its workgroups take the CUs as those of k retire: frames last 260-350 us) nor for the 14 us launch hand-off
  // behind it.  Measured +2..4 % (541 / 533 / 533 k against 519 / 510 / 534 k frames/s, alternating runs on one box).
  // (Measured in rounds 2-4, when a streaming kernel in front of the frame kernel set the pipeline's pace as a guest of the
  // frame kernels: one wave per SIMD beside a frame workgroup, ~440 us per batch.  The frame kernel reads the input itself now.)
  h->frame_toggle = (h->frame_toggle + 1) % std::max(h->n_frame_streams, 1);
  h->stream = h->stream_frames[h->frame_toggle];
  HIPCHK(hipStreamWaitEvent(h->stream, ws.ev_key, 0));
  return VOFOD_OK;
}

// A single map-updating scan without debug output (the reference's own mode) clusters close first on the general path
// (kernels_far.h): close bits from hasCloseTo's stencil with every voxel as its own cluster, then edges and unions around the
// far voxels only - instead of the six brick kernels over the whole frame.
int cluster_far_single(vofod_handle* h, Workspace& ws, const vplan::ChainPlan& plan, const GridParams& g, const vofod_handle::ClusterTables* ct, const CloseParams& cpar, const UpdateParams& up,
                       float thr_new)
{
  const uint32_t gv = (ws.vox_cap + 255u) / 256u;
  uint32_t* far_list = ws.d_labels;  // (labels are not written on this path)
  KLAUNCH(h, k_closefar, fgrid(g, gv), dim3(256), g, h->mg, cpar, h->d_crows, ws.d_hdrs, h->d_mapbits, ws.va, static_cast<const uint32_t*>(nullptr), static_cast<const unsigned long long*>(nullptr), ws.d_cand,
          ws.d_hdrs);
  KLAUNCH(h, k_closefar_sweep, fgrid(g, (ws.vox_cap * 16u + 255u) / 256u), dim3(256), g, h->mg, cpar, h->d_crows, ws.d_hdrs, h->d_mapbits, ws.va, ws.d_cand, far_list, ws.d_hdrs, ws.vox_cap);
  const uint32_t items = FAR_MAX * 2u * static_cast<uint32_t>(ct->n_rows);
  KLAUNCH(h, k_far_edges, dim3((items + 255u) / 256u), dim3(256), g, ct->cp, ct->d_rows, ws.d_hdrs, ws.d_bitmaps, ws.d_wprefix, ws.va, far_list);
  KLAUNCH(h, k_far_final, dim3(1), dim3(1024), g, ws.d_hdrs, ws.va, far_list, up, ws.d_table, ws.d_cand);
  // The occupancy image is patched where the update flips a bit (plan.mapbits_patched: valid while one voxel of the scan falls into
  // one map cell - the aligned lattice - and the flood fills' frontier value is no background value: their writes then flip nothing).
  KLAUNCH(h, k_finalize_far, dim3(gv), dim3(256), g, h->mg, up, ws.d_hdrs, ws.va, h->d_map, h->d_flags, ws.d_bitmaps, plan.mapbits_patched ? h->d_mapbits : nullptr, h->d_bgcount, thr_new);
  return VOFOD_OK;
}

// ---- K8/K9 findCloseFarClusters :703-750 (tables and images were prepared before the chain was enqueued) and
// ---- K10 updateVMaps :943-950 + cluster table + candidate members: whatever the clustering has not done already
int closefar_and_finalize(vofod_handle* h, Workspace& ws, const vplan::ChainPlan& plan, const GridParams& g, const CloseParams& cpar, const UpdateParams& up, vofod_scan_debug* dbg, const DevEvent* ev)
{
  const uint32_t gv = (ws.vox_cap + 255u) / 256u;
  if (plan.closefar != vplan::CloseFar::Fused)
  {
    // few frames: the undecided voxels go through a list to a sweep kernel with 16 lanes per voxel (ws.d_cand is free until
    // k_finalize); many frames: swept in place
    const bool split = plan.closefar == vplan::CloseFar::Split;
    KLAUNCH(h, k_closefar, fgrid(g, gv), dim3(256), g, h->mg, cpar, h->d_crows, ws.d_hdrs, h->d_mapbits, ws.va, ws.d_labels, plan.use_dilated ? h->d_mapclose : nullptr,
            split ? ws.d_cand : nullptr, ws.d_hdrs);
    if (split)
      KLAUNCH(h, k_closefar_sweep, fgrid(g, (ws.vox_cap * 16u + 255u) / 256u), dim3(256), g, h->mg, cpar, h->d_crows, ws.d_hdrs, h->d_mapbits, ws.va, ws.d_cand);
  }
  if (dbg)
    HIPCHK(hipEventRecord(ev[3], h->stream));
  if (plan.finalize == vplan::Finalize::Finalize)
    KLAUNCH(h, k_finalize, fgrid(g, gv), dim3(256), g, h->mg, up, ws.d_hdrs, ws.va, ws.d_labels, h->d_map, h->d_flags, ws.d_table, ws.d_cand, plan.keep_dirty ? nullptr : ws.d_bitmaps);
  return VOFOD_OK;
}

// VOFOD_SCAN_AUTO_RAYCAST applies the pending raycast update (or starts a pass) between ++its and the classification
// (:949-963), i.e. between the kernels enqueued so far and the device tail: the scan's status comes back first (a scan that has
// to run again, or failed, must not have moved the raycast state), then the raycast role, then the tail kernels.
int raycast_ahead_of_tail(vofod_handle* h, Workspace& ws, FrameCall& call)
{
  HIPCHK(hipMemcpyAsync(&ws.h_packed[0].hdr, ws.d_hdrs, sizeof(FrameHdr), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ws.h_packed[0].hdr.status == VOFOD_OK)
  {
    h->detection_its++;  // :949
    if (h->raycast_pending)
      raycast_finish_locked(h);
    else
      raycast_begin_locked(h, &call.scans[0], call.tfs, staged_pose_table(ws, call.scans[0]));
    call.rc_done = true;
  }
  return VOFOD_OK;
}

// Classification tail on the device (kernels_tail.h): boxes + gates, flood fills, detection records; nothing comes back
// but the records.
// (round 4: a single map-updating scan - the reference's own mode - takes the device tail too: no cluster table down, explore
// jobs up, results down between the kernels; the flood fills then write their frontiers to the map itself, vofod_nodelet.cpp:1712-1715)
int launch_device_tail(vofod_handle* h, Workspace& ws, const vplan::ChainPlan& plan, const LaunchRoute& rt, FrameCall& call)
{
  const uint32_t n = call.n;
  const GridParams& g = call.g;
  const vofod_dyn_params& dp = *call.dp;
  // the background latch (:716-721) is needed now, not at collect time
  VCHK(latch_background(h));
  ExploreBufs& eb = rt.own_tail >= 0 ? h->explore_slot[rt.own_tail] : h->explore;
  const uint32_t ebF = rt.own_tail >= 0 ? std::max<uint32_t>(eb.F(), (n + 31u) & ~31u) : h->ws.F;
  VCHK(ensure_explore(h, eb, ebF, static_cast<size_t>(ebF) * vtd::TP_MAXC, static_cast<size_t>(ebF) * vtd::TP_MAXM));
  // A submitted batch runs its tail on the handle's tail stream: one wave per frame does the flood
  // fills (latency bound, ~0.1 ms), which overlaps with the streaming kernels of the next batch instead of delaying them.
  // The tail stream also serialises the tails of the batches in flight on the shared flood-fill buffers.
  hipStream_t chain_stream = h->stream;
  StreamScope tail_scope(h);
  if (!h->ev_explore)
    HIPCHK(h->ev_explore.create(hipEventCreateWithFlags, hipEventDisableTiming));
  // (large batches: the tails take turns on the tail stream, underneath the frame kernel of the next batch)
  if (rt.own_tail >= 0)
    ;  // (own buffers, own stream: nothing to wait for)
  else if (call.submitted && h->stream_tail)
  {
    HIPCHK(hipEventRecord(ws.ev_packed, chain_stream));  // the cluster tables of this batch are complete
    h->stream = h->stream_tail;
    HIPCHK(hipStreamWaitEvent(h->stream, ws.ev_packed, 0));
  }
  else
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_explore, 0));  // (a synchronous call: wait for the tails of batches in flight)
  const vt::TailParams tp = tail_params(h, dp);
  const vc::ExploreParams ep = explore_params(dp, static_cast<float>(dp.voxel_map__thresholds__new_obstacles), plan.no_update);
  // the records (135 KB) go straight into the pinned host slots from the last tail kernel: no copy command on any stream (see k_tail_finish)
  static const bool diag_no_tail = std::getenv("VOFOD_DIAG_NO_TAIL") != nullptr;  // (diagnostics: timing of the pipeline without the tail kernel - results are wrong)
  if (diag_no_tail && n >= 128u)
    ;
  else if (plan.tail == vplan::Tail::Far)
    // close-first frames: ordered lists from the frame kernel (or k_far_final), the whole tail in one kernel of one wave per frame
    KLAUNCH(h, vtd::k_tail_far, dim3((n + vtd::TAIL_WPB - 1) / vtd::TAIL_WPB), dim3(64 * vtd::TAIL_WPB), g, ws.d_hdrs, ws.d_args, ws.d_table, ws.d_cand, ws.va, h->mg, tp, ep, eb.d_jobs, eb.d_members, h->d_map, eb.d_overlay, eb.d_stack, eb.d_explored, eb.d_touched,
            eb.d_ovl_list, eb.d_ovl_count, eb.d_results, eb.d_visited, ws.d_dets, ws.h_dets_dev, plan.far_single ? ws.d_tailc : static_cast<vtd::TailCluster*>(nullptr),
            (ws.prof_deferred && h->d_prof_ccl && !plan.far_single) ? h->d_prof_ccl + 32 * static_cast<size_t>(ws.prof_slot0) : static_cast<unsigned long long*>(nullptr));
  else
  {
    KLAUNCH(h, vtd::k_tail_prep, dim3(n), dim3(vtd::TP_THREADS), g, ws.d_hdrs, ws.d_args, ws.d_table, ws.d_cand, ws.va, h->mg, tp, eb.d_jobs, ws.d_job_be, ws.d_job_be + ws.F, eb.d_members, ws.d_tailc,
            ws.d_dets);
    KLAUNCH(h, vc::k_explore, dim3(n), dim3(64), ep, h->mg, eb.d_jobs, ws.d_job_be, ws.d_job_be + ws.F, eb.d_members, h->d_map, eb.d_overlay, eb.d_stack, eb.d_explored, eb.d_touched, eb.d_ovl_list,
            eb.d_ovl_count, eb.d_results, eb.d_visited);
    KLAUNCH(h, vtd::k_tail_finish, dim3(n), dim3(64), ws.d_tailc, eb.d_results, ws.d_dets, ws.h_dets_dev);
  }
  if (rt.own_tail < 0)
    HIPCHK(hipEventRecord(h->ev_explore, h->stream));  // the shared flood-fill buffers are free again
  call.tail_stream_used = h->stream;
  return VOFOD_OK;
}

// The launch half.  `call` is filled for the collect half of a synchronous call; a submitted batch leaves what its collect
// half needs in the workspace (pending, job_n, job_g, job_tfs, job_scans, job_dp, plan, ev_done).
// The kernel chain is decided once, by plan_chain (chain_plan.h), when everything it depends on is known - the staged inputs,
// the cluster tables, the latches - and before the first kernel of the chain is enqueued; the stages below execute the plan.
int launch_frames(vofod_handle* h, Workspace& ws, FrameCall& call)
{
  const vofod_static_params& sp = h->sp;
  const bool submitted = call.submitted;
  const uint32_t n = call.n;
  vofod_scan_debug* dbg = call.dbg;
  ws.det_valid = false;  // (as in stage_inputs: a re-run does not stage, an empty batch launches nothing)
  if (submitted && !ws.rerun)
    ws.job_dp = h->dp;
  call.dp = submitted ? &ws.job_dp : &h->dp;
  const vofod_dyn_params& dp = *call.dp;
  if (n == 0)
    return VOFOD_OK;
  if (n > ws.F)
  {
    h->err = "batch larger than max_batch_frames";
    return VOFOD_ERR_CAPACITY;
  }
  const size_t npts = static_cast<size_t>(sp.sensor_hrays) * sp.sensor_vrays;
  for (uint32_t f = 0; f < n; f++)
  {
    const vofod_scan& s = call.scans[f];
    if ((!s.x || !s.y || !s.z) && !is_range_image(s))  // (one or two of the three NULL, or no range column either)
      return VOFOD_ERR_INVALID_ARG;
    VCHK(check_col_tfs(h, s));
    if (static_cast<size_t>(s.width) * s.height != npts)  // :895-899
      return VOFOD_ERR_SIZE_MISMATCH;
  }
  // re-run of the batch that overflowed the LDS kernels: the flag is consumed here, whatever path this call takes (an early
  // error return must not leave it standing for a different batch), and only a launch of the very same job reuses its inputs
  const bool rerun = ws.rerun && ws.job_n == n;
  ws.rerun = false;
  DevEvent* ev = call.ev;
  if (dbg)
    for (int i = 0; i < 5; i++)
      HIPCHK(ev[i].create(hipEventCreate));
  const float thr_new = static_cast<float>(dp.voxel_map__thresholds__new_obstacles);

  // ---- the switches, read once per call; where the chain goes (the streams of a submitted launch)
  const vplan::Switches sw = vplan::read_switches();
  const bool no_update = call.flags & VOFOD_SCAN_NO_MAP_UPDATE;
  const bool use_dilated = vplan::wants_dilated(sw, no_update, n);  // (the one decision the map images need ahead of the plan)
  LaunchRoute rt;
  if (submitted)
    VCHK(route_submitted(h, ws, n, rt));
  StreamScope chain_scope(h, rt.chain);
  if (submitted && h->ev_stagger_set)
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_stagger, 0));  // the previous batch's streaming kernels are through
  if (submitted && !(h->mapbits_valid && h->mapbits_thr == thr_new))
  {
    // the occupancy image is shared by both chains: make sure it is complete before a second stream reads it
    VCHK(ensure_mapbits(h, thr_new));
    HIPCHK(hipStreamSynchronize(h->stream));
  }

  bool host_copies = false;
  if (!rerun)
    VCHK(stage_inputs(h, ws, call.scans, call.tfs, n, npts, host_copies));
  // include/vofod.h promises that the scans' host buffers need not outlive vofod_batch_submit.  A copy from page-locked memory
  // is truly asynchronous - and on the streaming stage's stream it is queued behind the previous batch's streaming kernels:
  // it may start long after the call has returned, when a caller that refills its arena has already overwritten it.
  // The event marks the end of the batch's copies; the submitting call returns behind it (below).
  if (host_copies && submitted && ws.ev_h2d)
    HIPCHK(hipEventRecord(ws.ev_h2d, h->stream));
  else
    host_copies = false;
  H2DGuard h2d_guard{ws.ev_h2d, host_copies};
  if (!rerun)
  {
    VCHK(decode_ranges(h, ws, npts));
    VCHK(deskew_points(h, ws, npts));
  }

  GridParams& g = call.g;
  const float leaf[3] = {sp.voxel_size, sp.voxel_size, sp.voxel_size};
  const int zero[3] = {0, 0, 0};
  float align_center[3];
  h->hg.idxToCoord(zero, align_center);  // :664
  fill_grid_params(h, g, leaf, true, align_center, ws);
  CloseParams cpar{};
  VCHK(prepare_map_images(h, dp, thr_new, use_dilated, !h->background_pts_sufficient || dbg, cpar));
  if (dbg)
    HIPCHK(hipEventRecord(ev[0], h->stream));

  // ---- the plan (chain_plan.h): its inputs, gathered; the two latches as they stand now
  vofod_handle::ClusterTables* ct = nullptr;
  VCHK(cluster_tables(h, g, static_cast<float>(dp.ground_points_max_distance), map_cmax(h), &ct));
  const bool rerun_off_lds = h->lds_ccl_off;
  h->lds_ccl_off = false;  // one-shot: only the re-run of the batch that overflowed stays off the LDS kernels
  // (the release bound is tested against the count of the map as it is NOW: a map image rebuilt for this call - vofod_write_map, a
  // scan through the full clustering - has its count still on the way, n_bg_voxels is the previous map's until it is fetched)
  if (h->cf_off)
    VCHK(latch_background(h));
  if (h->cf_off && (h->n_bg_voxels > h->cf_off_bg + h->cf_off_bg / 4 + 1000 || h->n_bg_voxels < h->cf_off_bg))
    h->cf_off = false;  // the map has changed a lot since: try the close-first kernel again
  vplan::PlanInputs in = plan_inputs(h, ws, ct, sw);
  in.lds_ccl_off = rerun_off_lds;
  in.n = n;
  in.no_update = no_update;
  in.submitted = submitted;
  in.dbg = dbg != nullptr;
  in.dbg_far_only = dbg && dbg[0].far_only;
  in.auto_raycast = call.flags & VOFOD_SCAN_AUTO_RAYCAST;
  const RefLattice ref_lattice = fill_ref_lattice(g);  // the frame kernel's bricks and cell codes refer to it
  in.ref_lattice_on = ref_lattice.on != 0;
  in.layout_packed = true;  // packed, 16-byte aligned float columns, a multiple of 4 points each: the frame kernel's input pass uses 16-byte loads
  for (uint32_t f = 0; f < n && in.layout_packed; f++)
  {
    const FrameArgs& a = ws.h_args[f];
    in.layout_packed = a.stride == 4 && (a.n & 3u) == 0 && a.n >= 4 && ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.y) | reinterpret_cast<uintptr_t>(a.z)) & 15u) == 0;
  }
  in.patchable = g.align && static_cast<float>(dp.voxel_map__thresholds__frontiers) <= thr_new;
  const vplan::ChainPlan& plan = ws.plan = vplan::plan_chain(in);
  if (trace_on())
    std::fprintf(stderr, "[vofod trace] n=%u plan: %s, %s, %s, %s, %s\n", n, name(plan.voxeliser), name(plan.clusterer), name(plan.closefar), name(plan.finalize), name(plan.tail));
  g.sparse_prefix = plan.bricks ? 1u : 0u;

  // ---- K1-K6 (filterAndTransform :621-684) - or only what the frame kernel, which reads the input itself, needs ahead of it
  VCHK(launch_voxelize(h, ws, plan, g, n, static_cast<uint32_t>(npts)));
  if (dbg)
    HIPCHK(hipEventRecord(ev[1], h->stream));
  if (rt.staged)
    VCHK(enter_frame_stream(h, ws));

  // ---- K7 clusterCloud :932.  Read-only batches cluster close first (k_frame_lds): only the far clusters are ever used
  // (vofod_nodelet.cpp:946-963).  The debug view of ALL clusters keeps the full clustering; dbg[0].far_only asks for the
  // production path's view instead.
  UpdateParams up{};
  up.score_point = static_cast<float>(dp.voxel_map__scores__point);
  up.score_unknown = static_cast<float>(dp.voxel_map__scores__unknown);
  up.min_points = dp.classification__min_points;
  up.cand_max_extent = static_cast<float>(dp.classification__max_size * (1.0 + 1e-4) + 1e-3 * sp.voxel_size);
  up.no_update = no_update;
  if (plan.far_single)
    VCHK(cluster_far_single(h, ws, plan, g, ct, cpar, up, thr_new));
  else if (plan.frame())
    VCHK(launch_frame_kernel(h, ws, plan, g, n, ct, ref_lattice, up));
  else
    VCHK(launch_cluster(h, ws, plan, g, ct));
  if (dbg)
    HIPCHK(hipEventRecord(ev[2], h->stream));
  VCHK(closefar_and_finalize(h, ws, plan, g, cpar, up, dbg, ev));
  ws.bitmap_clean = plan.bitmap_clean_after;

  // ---- the tail on the device, or the read-back of what the host tail needs
  call.tail_stream_used = h->stream;
  if (plan.raycast_ahead)
    VCHK(raycast_ahead_of_tail(h, ws, call));
  if (plan.dtail)
    VCHK(launch_device_tail(h, ws, plan, rt, call));
  else
    VCHK(read_back_full(h, ws, g, n));
  if (dbg)
    HIPCHK(hipEventRecord(ev[4], h->stream));
  call.tr_launch = ms_since(call.t0);
  if (!submitted)
    return VOFOD_OK;  // (the collect half follows in the same call)

  h2d_guard.armed = false;
  if (host_copies)
    HIPCHK(hipEventSynchronize(ws.ev_h2d));  // (the whole chain is enqueued by now: the device works while the host waits for the link)
  HIPCHK(hipEventRecord(ws.ev_done, plan.dtail ? call.tail_stream_used : h->stream));
  ws.pending = true;
  ws.job_n = n;
  ws.job_g = g;
  if (call.tfs != ws.job_tfs.data())
    ws.job_tfs.assign(call.tfs, call.tfs + 12 * static_cast<size_t>(n));
  if (call.scans != ws.job_scans.data())
    ws.job_scans.assign(call.scans, call.scans + n);
  return VOFOD_OK;
}

}  // namespace
