// Collect half of the per-scan entry points (included by vofod_hip.hip behind frames_launch.h): wait for the chain, then the host
// side of processMsg (vofod_nodelet.cpp:946-965) - map-image bookkeeping, the raycast role, the device tail's records or the host tail.
#pragma once

namespace
{

// The frames' status words, wherever they came back, into the packed slots.  A frame that held more bricks than the LDS
// clustering kernel takes: nothing of this batch was used (batches never update the map); the caller runs it again on the
// global-memory kernels.
int adopt_status(vofod_handle* h, Workspace& ws, uint32_t n)
{
  if (ws.plan.dtail)
    for (uint32_t f = 0; f < n; f++)
      ws.h_packed[f].hdr.status = ws.h_dets[f].status;
  for (uint32_t f = 0; f < n; f++)
    if (ws.h_packed[f].hdr.status == CCL_RETRY_STATUS)
    {
      h->lds_ccl_off = true;
      ws.rerun = true;
      ws.job_n = n;
      ws.bitmap_clean = false;
      return CCL_RETRY_STATUS;
    }
  return VOFOD_OK;
}

// a map-updating scan has changed the map under its occupancy image
void book_map_images(vofod_handle* h, Workspace& ws)
{
  // (the image was patched by k_finalize_far - unless the scan has to run again or left the map: then it is rebuilt)
  if (ws.plan.mapbits_patched && ws.h_packed[0].hdr.status == VOFOD_OK && h->mapbits_valid)
  {
    h->bgcount_stale = true;  // (the counters on the device are newer than the host's sum: fetched when somebody needs it)
    h->mapbits_gen++;         // (the dilated image of the batches is of an older state)
  }
  else
    h->mapbits_valid = false;
}

// A frame with more pure-far bricks than the close-first kernel takes: nothing of this batch was used; the caller runs
// it again (same descriptors, staged columns kept) with the full clustering.
int check_close_first_overflow(vofod_handle* h, Workspace& ws, uint32_t n)
{
  for (uint32_t f = 0; f < n; f++)
    if (ws.h_packed[f].hdr.status == CF_RETRY_STATUS)
    {
      h->cf_off = true;
      h->cf_off_bg = h->n_bg_voxels;
      ws.rerun = true;
      ws.job_n = n;
      return CCL_RETRY_STATUS;
    }
  return VOFOD_OK;
}

// What the three record builders below share: extractDetections' record (:848-877) for one detection after the other - ids,
// the references vofod_detection_points answers from, the caller's array up to its capacity - and the ending of the call.
struct RecordSink
{
  vofod_handle* h;
  Workspace& ws;
  const FrameCall& call;
  vofod_detection* out;
  size_t cap;
  uint32_t* n_out_per_frame;
  size_t total = 0, frame_begin = 0;
  RecordSink(vofod_handle* h_, Workspace& ws_, const FrameCall& call_, vofod_detection* out_, size_t cap_, uint32_t* n_out_per_frame_)
      : h(h_), ws(ws_), call(call_), out(out_), cap(cap_), n_out_per_frame(n_out_per_frame_)
  {
    ws.det_begin(call.submitted, call.g);
  }
  void add(uint32_t f, uint32_t root, const float center[3], uint32_t n_points, double conf_sum)
  {
    const vofod_detection det = vt::make_detection(h->last_detection_id++, call.tfs + 12 * f, center, n_points, conf_sum, f, h->sp, *call.dp);
    ws.det_refs.push_back({det.id, f, root, n_points});
    if (out && total < cap)
      out[total] = det;
    total++;
  }
  void frame_done(uint32_t f)
  {
    if (n_out_per_frame)
      n_out_per_frame[f] = static_cast<uint32_t>(total - frame_begin);
    frame_begin = total;
  }
  int close(int ret, size_t* n_out)
  {
    *n_out = total;
    if (total > cap)
      ret = VOFOD_ERR_CAPACITY;
    ws.det_valid = ret == VOFOD_OK;
    return ret;
  }
};

// ---- the tail ran on the device: the raw detections, frame by frame
int device_tail_records(vofod_handle* h, Workspace& ws, const FrameCall& call, vofod_detection* out, size_t cap, uint32_t* n_out_per_frame, size_t* n_out)
{
  const uint32_t n = call.n;
  int ret = VOFOD_OK;
  if (call.submitted && out)
  {
    // an output array too small for this batch: nothing is consumed - the ticket stays pending, ids are not handed
    // out, *n_out tells the size to come back with
    size_t need = 0;
    for (uint32_t f = 0; f < n; f++)
      need += ws.h_dets[f].n;
    if (need > cap)
    {
      ws.pending = true;
      *n_out = need;
      return VOFOD_ERR_CAPACITY;
    }
  }
  RecordSink sink(h, ws, call, out, cap, n_out_per_frame);
  for (uint32_t f = 0; f < n; f++)
  {
    const vtd::FrameDets& D = ws.h_dets[f];
    if (D.status != VOFOD_OK)
      ret = D.status;
    for (uint32_t i = 0; i < D.n; i++)
      sink.add(f, D.d[i].root, D.d[i].center, D.d[i].n_points, D.d[i].conf_sum);
    sink.frame_done(f);
  }
  if (trace_on())
    std::fprintf(stderr, "[vofod trace] n=%u device tail: sync %.3f end %.3f ms, %zu detections\n", n, call.tr_sync1, ms_since(call.t0), sink.total);
  return sink.close(ret, n_out);
}

// A map-updating scan whose flood fills have already written their frontiers to the map: the tail cannot be run again.
// More detections than the record slots hold (TP_MAXD per frame): everything needed is on the device - the clusters in
// canonical order (d_tailc) and their explore results.  (A work list overflow cannot happen for radii the device accepts.)
int device_tail_overflow_records(vofod_handle* h, Workspace& ws, const FrameCall& call, uint32_t fb, vofod_detection* out, size_t cap, uint32_t* n_out_per_frame, size_t* n_out)
{
  if (fb & vtd::TAIL_FB_EXPLORE)
  {
    h->err = "device tail: flood-fill work list overflow";
    return VOFOD_ERR_DEVICE;
  }
  std::vector<vtd::TailCluster> tc(vtd::TP_MAXC);
  std::vector<vc::ExploreResult> res(vtd::TP_MAXC);
  HIPCHK(hipMemcpy(tc.data(), ws.d_tailc, sizeof(vtd::TailCluster) * vtd::TP_MAXC, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(res.data(), h->explore.d_results, sizeof(vc::ExploreResult) * vtd::TP_MAXC, hipMemcpyDeviceToHost));  // (frame 0: result slots 0..TP_MAXC-1)
  RecordSink sink(h, ws, call, out, cap, n_out_per_frame);
  for (int c = 0; c < vtd::TP_MAXC; c++)
    if (tc[c].job >= 0 && tc[c].job < vtd::TP_MAXC && res[tc[c].job].floating)
      sink.add(0u, tc[c].root, tc[c].obb_center, tc[c].n_members, res[tc[c].job].conf_sum);
  sink.frame_done(0u);
  return sink.close(VOFOD_OK, n_out);
}

// ---- host tail: classifyClusters :961 + extractDetections :963.
// Host: canonical cluster order, OBB + gates of the few candidate clusters.  Device (k_explore): the flood
// fills and uncertainty sums, one wave per frame, jobs of a frame in the reference's order.
struct FrameTail
{
  std::vector<HostCluster> cl;
  vt::MemberIndex by_root;
  std::vector<int> job_of;  // per cluster: index into jobs or -1
  bool host_fallback = false;
  // tables that overflowed the speculative read-back (phase A)
  std::vector<ClusterRec> recs_big;
  std::vector<CandMemberX> members_big;
  bool big_recs = false, big_members = false;
  // the frame's explore jobs before the frames are concatenated (phase B)
  std::vector<vc::ExploreJob> jobs;
  std::vector<int> members;
};

struct ExploreWork
{
  std::vector<vc::ExploreJob> jobs;
  std::vector<uint32_t> job_begin;
  std::vector<int> job_members;
  std::vector<vc::ExploreResult> results;
};

// phase A (serial): frames whose tables overflowed the speculative read-back fetch the rest
int fetch_big_tables(vofod_handle* h, Workspace& ws, const GridParams& g, uint32_t n, std::vector<FrameTail>& tails, int& ret)
{
  for (uint32_t f = 0; f < n; f++)
  {
    FrameTail& T = tails[f];
    const FrameHdr& hdr = ws.h_packed[f].hdr;
    if (hdr.status != VOFOD_OK)
      ret = hdr.status;
    T.big_recs = hdr.C > SPEC_C;
    T.big_members = hdr.n_cand > SPEC_M;
    if (T.big_recs)
    {
      T.recs_big.resize(hdr.C);
      HIPCHK(hipMemcpy(T.recs_big.data(), ws.d_table + static_cast<size_t>(f) * ws.vox_cap, sizeof(ClusterRec) * hdr.C, hipMemcpyDeviceToHost));
    }
    if (T.big_members)
    {
      T.members_big.resize(hdr.n_cand);
      CandMemberX* d_tmp = static_cast<CandMemberX*>(ws.d_members_big);  // n_cand <= V <= vox_cap: sized with the workspace
      KLAUNCH(h, k_gather_members, dim3((hdr.n_cand + 255) / 256), dim3(256), g, f, hdr.n_cand, ws.d_cand, ws.va, d_tmp);
      HIPCHK(hipMemcpyAsync(T.members_big.data(), d_tmp, sizeof(CandMemberX) * hdr.n_cand, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
  }
  return VOFOD_OK;
}

// phase B (one frame, run in parallel over the frames): canonical order, member index, boxes and gates, the frame's explore jobs
void prep_frame_tail(const vofod_handle* h, const PackedFrame& pf, uint32_t f, const float* tf, const vt::TailParams& tp, FrameTail& T)
{
  const FrameHdr& hdr = pf.hdr;
  const ClusterRec* recs = T.big_recs ? T.recs_big.data() : pf.table;
  const CandMemberX* members = T.big_members ? T.members_big.data() : pf.members;
  // canonical order: size desc, smallest member asc
  T.cl.resize(hdr.C);
  for (uint32_t c = 0; c < hdr.C; c++)
    T.cl[c].rec = recs[c];
  std::sort(T.cl.begin(), T.cl.end(), [](const HostCluster& a, const HostCluster& b) {
    if (a.rec.size != b.rec.size)
      return a.rec.size > b.rec.size;
    return a.rec.root < b.rec.root;
  });
  {
    std::vector<std::pair<uint64_t, vt::Member>> tmp(hdr.n_cand);
    for (uint32_t i = 0; i < hdr.n_cand; i++)
    {
      const CandMemberX& m = members[i];
      tmp[i] = {(static_cast<uint64_t>(m.root) << 32) | m.v, vt::Member{m.v, {m.x, m.y, m.z}, m.count}};
    }
    T.by_root.build(tmp);
  }
  T.job_of.assign(hdr.C, -1);
  std::vector<vc::ExploreJob>& jl = T.jobs;
  std::vector<int>& ml = T.members;
  for (uint32_t ci = 0; ci < hdr.C; ci++)
  {
    HostCluster& c = T.cl[ci];
    if (c.rec.close)
      continue;
    c.cclass = VOFOD_CLASS_INVALID;
    if (!c.rec.cand)
      continue;  // fails min_points or cannot pass max_size (device-side gate)
    const vt::MemberSpan mem = T.by_root.of(c.rec.root);
    auto get = [&](size_t i, float p[3]) {
      for (int a = 0; a < 3; a++)
        p[a] = mem[i].p[a];
    };
    // classify_cluster :1648-1696: boxes, gates, the explore job's radius and box
    c.gates = vt::classify_gates(static_cast<uint32_t>(mem.size()), get, tf, tp, h->hg.off, h->hg.vs_inv, h->hg.s);
    if (c.gates.passed && !c.gates.explore)  // without the latches :1694, :1719-1722
      c.cclass = VOFOD_CLASS_UNKNOWN;
    if (!c.gates.explore)
      continue;
    vc::ExploreJob job{};
    job.frame = f;
    job.n_members = static_cast<uint32_t>(mem.size());
    job.member_off = static_cast<uint32_t>(ml.size() / 3);  // rebased when the frames are concatenated
    job.R = c.gates.R;
    for (int a = 0; a < 3; a++)
    {
      job.box_lo[a] = c.gates.box_lo[a];
      job.box_hi[a] = c.gates.box_hi[a];
    }
    for (const vt::Member& m : mem)
    {
      int o[3];
      h->hg.coordToIdx(m.p, o);
      ml.insert(ml.end(), o, o + 3);
    }
    if (job.R > vc::EX_MAX_R || job.R < 0)
      T.host_fallback = true;
    T.job_of[ci] = static_cast<int>(jl.size());  // rebased when the frames are concatenated
    jl.push_back(job);
  }
  if (jl.size() > vc::EX_MAX_JOBS)
    T.host_fallback = true;
}

// phase C (serial): concatenate the frames' job lists in frame order
void concat_jobs(std::vector<FrameTail>& tails, ExploreWork& w)
{
  const uint32_t n = static_cast<uint32_t>(tails.size());
  w.job_begin.assign(n + 1, 0);
  for (uint32_t f = 0; f < n; f++)
  {
    w.job_begin[f] = static_cast<uint32_t>(w.jobs.size());
    const uint32_t jbase = static_cast<uint32_t>(w.jobs.size()), mbase = static_cast<uint32_t>(w.job_members.size() / 3);
    for (vc::ExploreJob j : tails[f].jobs)
    {
      j.member_off += mbase;
      j.result_slot = static_cast<uint32_t>(w.jobs.size());
      w.jobs.push_back(j);
    }
    w.job_members.insert(w.job_members.end(), tails[f].members.begin(), tails[f].members.end());
    for (int& ji : tails[f].job_of)
      if (ji >= 0)
        ji += static_cast<int>(jbase);
  }
  w.job_begin[n] = static_cast<uint32_t>(w.jobs.size());
  w.results.resize(w.jobs.size());
}

// the flood fills and uncertainty sums of the host tail's jobs on the device (k_explore), results back
int explore_on_device(vofod_handle* h, const FrameCall& call, ExploreWork& w, float thr_new, bool no_update)
{
  const uint32_t n = call.n;
  VCHK(ensure_explore(h, h->explore, h->ws.F, w.jobs.size(), w.job_members.size() / 3));
  // a collected async batch runs its tail on a second stream so that it does not queue behind the next batch's chain
  StreamScope tail_scope(h, call.submitted ? h->stream_tail : nullptr);
  ExploreBufs& eb = h->explore;
  if (h->ev_explore)
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_explore, 0));  // a device tail in flight may still use the flood-fill buffers
  HIPCHK(hipMemcpyAsync(eb.d_jobs, w.jobs.data(), sizeof(vc::ExploreJob) * w.jobs.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(eb.d_job_begin, w.job_begin.data(), sizeof(uint32_t) * (n + 1), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(eb.d_members, w.job_members.data(), sizeof(int) * w.job_members.size(), hipMemcpyHostToDevice, h->stream));
  const vc::ExploreParams ep = explore_params(*call.dp, thr_new, no_update);
  KLAUNCH(h, vc::k_explore, dim3(n), dim3(64), ep, h->mg, eb.d_jobs, eb.d_job_begin, eb.d_job_begin + 1, eb.d_members, h->d_map, eb.d_overlay, eb.d_stack, eb.d_explored, eb.d_touched,
          eb.d_ovl_list, eb.d_ovl_count, eb.d_results, eb.d_visited);
  HIPCHK(hipMemcpyAsync(w.results.data(), eb.d_results, sizeof(vc::ExploreResult) * w.jobs.size(), hipMemcpyDeviceToHost, h->stream));
  if (h->ev_explore)
    HIPCHK(hipEventRecord(h->ev_explore, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!no_update)
    h->mapbits_valid = false;
  return VOFOD_OK;
}

// extractDetections :834-879 for one frame
void extract_detections(RecordSink& sink, const FrameTail& T, uint32_t f, const std::vector<vc::ExploreResult>& results)
{
  for (size_t ci = 0; ci < T.cl.size(); ci++)
  {
    const HostCluster& c = T.cl[ci];
    if (c.rec.close || c.cclass != VOFOD_CLASS_MAV)
      continue;
    sink.add(f, c.rec.root, c.gates.obb_center, static_cast<uint32_t>(T.by_root.of(c.rec.root).size()), results[T.job_of[ci]].conf_sum);
  }
  sink.frame_done(f);
}

// the debug view of one frame (vofod_scan_debug): counts, weighted cloud, labels, cluster list
int fill_debug_view(vofod_handle* h, Workspace& ws, const GridParams& g, uint32_t f, const FrameTail& T, bool far_view, vofod_scan_debug& d, int& ret)
{
  const FrameHdr& hdr = ws.h_packed[f].hdr;
  d.n_input_after_crop = hdr.n_in;
  d.n_bg_voxels = h->n_bg_voxels;
  d.background_pts_sufficient = h->background_pts_sufficient;
  d.sure_background_sufficient = h->sure_background_sufficient;
  // far-only view (dbg[0].far_only): what the production path of a read-only batch computes - the far clusters, and labels
  // for their voxels only.  A frame that went through the full clustering all the same (no dilated image, more pure-far
  // bricks than the close-first path takes, VOFOD_CLOSE_FIRST=0) is cut down to that view here.
  uint32_t n_shown = hdr.C;
  if (far_view && !hdr.far_only)
  {
    n_shown = 0;
    for (uint32_t c = 0; c < hdr.C; c++)
      n_shown += T.cl[c].rec.close ? 0u : 1u;
  }
  d.n_weighted = hdr.V;
  d.n_clusters = n_shown;
  if ((d.weighted || d.labels) && d.weighted_cap < hdr.V)
    ret = VOFOD_ERR_CAPACITY;
  else
  {
    if (d.weighted && hdr.V)
      HIPCHK(hipMemcpy(d.weighted, ws.va.pts + static_cast<size_t>(f) * ws.vox_cap, sizeof(float4) * hdr.V, hipMemcpyDeviceToHost));
    if (d.labels && hdr.V)
    {
      HIPCHK(hipMemcpy(d.labels, ws.d_labels + static_cast<size_t>(f) * ws.vox_cap, sizeof(uint32_t) * hdr.V, hipMemcpyDeviceToHost));
      if (far_view && !hdr.far_only)
      {
        std::vector<uint32_t> far_roots;
        for (uint32_t c = 0; c < hdr.C; c++)
          if (!T.cl[c].rec.close)
            far_roots.push_back(T.cl[c].rec.root);
        std::sort(far_roots.begin(), far_roots.end());
        for (uint32_t v = 0; v < hdr.V; v++)
          if (!std::binary_search(far_roots.begin(), far_roots.end(), d.labels[v]))
            d.labels[v] = CF_LABEL_NONE;
      }
    }
  }
  if (d.clusters)
  {
    if (d.clusters_cap < n_shown)
      ret = VOFOD_ERR_CAPACITY;
    else
      for (uint32_t c = 0, c_out = 0; c < hdr.C; c++)
      {
        const HostCluster& hc = T.cl[c];
        if (far_view && hc.rec.close)
          continue;
        vofod_cluster_info& ci = d.clusters[c_out++];
        ci.first_member = hc.rec.root;
        ci.n_points = hc.rec.size;
        ci.is_close = hc.rec.close;
        ci.cclass = hc.cclass;
        for (int a = 0; a < 3; a++)
        {
          ci.aabb_min[a] = (static_cast<float>(hc.rec.imin[a]) + 0.5f) * g.leaf[a] + hdr.offset[a];
          ci.aabb_max[a] = (static_cast<float>(hc.rec.imax[a]) + 0.5f) * g.leaf[a] + hdr.offset[a];
          ci.obb_center[a] = hc.gates.evaluated ? hc.gates.obb_center[a] : NAN;
        }
        ci.obb_size = hc.gates.obb_size;
      }
  }
  return VOFOD_OK;
}

// The host tail over the read-back tables of all frames.
int host_tail(vofod_handle* h, Workspace& ws, const FrameCall& call, const double dev_ms[4], vofod_detection* out, size_t cap, uint32_t* n_out_per_frame, size_t* n_out)
{
  const uint32_t n = call.n;
  const vofod_dyn_params& dp = *call.dp;
  vofod_scan_debug* dbg = call.dbg;
  const bool no_update = call.flags & VOFOD_SCAN_NO_MAP_UPDATE;
  const auto t_tail = clk::now();
  const float thr_new = static_cast<float>(dp.voxel_map__thresholds__new_obstacles);
  const float thr_frontiers = static_cast<float>(dp.voxel_map__thresholds__frontiers);
  const vt::TailParams tp = tail_params(h, dp);
  int ret = VOFOD_OK;
  std::vector<FrameTail> tails(n);
  ExploreWork w;
  VCHK(fetch_big_tables(h, ws, call.g, n, tails, ret));
  h->pool->parallel_for(n, [&](uint32_t f) { prep_frame_tail(h, ws.h_packed[f], f, call.tfs + 12 * f, tp, tails[f]); });
  concat_jobs(tails, w);
  const double tr_prep = ms_since(call.t0);

  bool any_host = std::getenv("VOFOD_EXPLORE") && std::strcmp(std::getenv("VOFOD_EXPLORE"), "host") == 0;  // tests exercise the fallback
  for (const FrameTail& T : tails)
    any_host |= T.host_fallback;
  if (!w.jobs.empty() && !any_host)
    VCHK(explore_on_device(h, call, w, thr_new, no_update));
  const double tr_explore = ms_since(call.t0);

  RecordSink sink(h, ws, call, out, cap, n_out_per_frame);
  for (uint32_t f = 0; f < n; f++)
  {
    FrameTail& T = tails[f];
    if (any_host && w.job_begin[f + 1] > w.job_begin[f])
    {
      // fallback (Manhattan radius or job count beyond the device kernel's limits): sequential host path over read-back boxes
      VCHK(host_explore_frame(h, T.cl, T.by_root, T.job_of, w.jobs, w.results, no_update, thr_frontiers, thr_new, dp));
    }
    for (size_t ci = 0; ci < T.cl.size(); ci++)
      if (const int ji = T.job_of[ci]; ji >= 0)
        T.cl[ci].cclass = w.results[ji].floating ? VOFOD_CLASS_MAV : VOFOD_CLASS_UNKNOWN;
    extract_detections(sink, T, f, w.results);
    if (dbg)
    {
      vofod_scan_debug& d = dbg[f];
      VCHK(fill_debug_view(h, ws, call.g, f, T, dbg[0].far_only != 0, d, ret));
      for (int i = 0; i < 4; i++)
        d.stage_ms[i] = dev_ms[i];
      d.stage_ms[4] = ms_since(t_tail);
      d.stage_ms[5] = ms_since(call.t0);
    }
  }
  if (trace_on())
  {
    size_t sumC = 0, sumCand = 0, sumEval = 0;
    for (uint32_t f = 0; f < n; f++)
    {
      sumC += ws.h_packed[f].hdr.C;
      sumCand += ws.h_packed[f].hdr.n_cand;
      for (const auto& c : tails[f].cl)
        sumEval += c.gates.evaluated;
    }
    std::fprintf(stderr, "[vofod trace] n=%u launch %.3f sync1 %.3f prep %.3f explore %.3f end %.3f ms jobs %zu C %zu cand_members %zu evaluated %zu\n", n, call.tr_launch, call.tr_sync1, tr_prep,
                 tr_explore, ms_since(call.t0), w.jobs.size(), sumC, sumCand, sumEval);
  }
  return sink.close(ret, n_out);
}

// The collect half: `call` comes from launch_frames of the same synchronous call, or from ticket_call.
int collect_frames(vofod_handle* h, Workspace& ws, FrameCall& call, vofod_detection* out, size_t cap, uint32_t* n_out_per_frame, size_t* n_out)
{
  const uint32_t n = call.n;
  if (n == 0)
  {
    GridParams g{};
    g.vox_cap = ws.vox_cap;
    ws.det_begin(call.submitted, g);
    ws.det_valid = true;  // (no frames, no detections: vofod_detection_points answers 0 / 0)
    return VOFOD_OK;      // (*n_out is zero already: the entry points clear it)
  }
  const bool no_update = call.flags & VOFOD_SCAN_NO_MAP_UPDATE;
  // ---- wait for the chain
  if (call.submitted)
  {
    HIPCHK(hipEventSynchronize(ws.ev_done));
    ws.pending = false;
  }
  else
    HIPCHK(hipStreamSynchronize(h->stream));
  VCHK(print_deferred_prof(h, ws, n));
  call.tr_sync1 = ms_since(call.t0);

  // ---- status of the frames, bookkeeping of the map images, the raycast role
  VCHK(adopt_status(h, ws, n));
  if (!no_update)
    book_map_images(h, ws);
  VCHK(latch_background(h));
  VCHK(check_close_first_overflow(h, ws, n));
  if (!no_update && !call.rc_done)
  {
    h->detection_its++;  // :949
    if (call.flags & VOFOD_SCAN_AUTO_RAYCAST)
    {
      if (h->raycast_pending)
        raycast_finish_locked(h);
      else
        raycast_begin_locked(h, &call.scans[0], call.tfs, staged_pose_table(ws, call.scans[0]));
    }
  }
  double dev_ms[4] = {0, 0, 0, 0};
  if (call.dbg)
    for (int i = 0; i < 4; i++)
    {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, call.ev[i], call.ev[i + 1]);
      dev_ms[i] = ms;
    }

  if (ws.plan.dtail)
  {
    uint32_t fb = 0;
    for (uint32_t f = 0; f < n; f++)
      fb |= ws.h_dets[f].fallback;
    if (!fb)
      return device_tail_records(h, ws, call, out, cap, n_out_per_frame, n_out);
    if (!no_update && (fb & (vtd::TAIL_FB_DETS | vtd::TAIL_FB_EXPLORE)))
      return device_tail_overflow_records(h, ws, call, fb, out, cap, n_out_per_frame, n_out);
    // a frame exceeded a capacity of the device tail: the host tail redoes the batch from the full tables
    // (capacities of k_tail_prep - members, clusters, radius: no flood fill has run yet, also on a map-updating scan)
    VCHK(read_back_full(h, ws, call.g, n));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return host_tail(h, ws, call, dev_ms, out, cap, n_out_per_frame, n_out);
}

// A frame beyond the capacities of the frame kernel makes a collect half return CCL_RETRY_STATUS: the batch runs once more - with
// the full clustering when the close-first kernel gave up (a cold map), on the global-memory kernels when the LDS image did;
// the two can follow each other, so twice at most.
template <class First, class Again>
int with_reruns(First&& first, Again&& again)
{
  int r = first();
  for (int attempt = 0; attempt < 2 && r == CCL_RETRY_STATUS; attempt++)
    r = again();
  return r;
}

// a synchronous call: one half after the other
int process_frames(vofod_handle* h, const vofod_scan* scans, const float* tfs, uint32_t n, int flags, vofod_detection* out, size_t cap, uint32_t* n_out_per_frame, size_t* n_out,
                   vofod_scan_debug* dbg)
{
  auto once = [&] {
    FrameCall call{false, scans, tfs, n, flags, dbg};
    const int r = launch_frames(h, h->ws, call);
    return r != VOFOD_OK ? r : collect_frames(h, h->ws, call, out, cap, n_out_per_frame, n_out);
  };
  return with_reruns(once, once);
}

}  // namespace
