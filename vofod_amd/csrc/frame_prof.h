// VOFOD_LDS_PROF (diagnostics; included by vofod_hip.hip): the 100 MHz wall clock stamps the frame kernel and k_slab_emit leave
// in the handle's stamp buffers, read back and printed.  The launch functions call in here with one line each; the formats are
// parsed by tools/phase_table.sh and tools/cu_gaps.py.
#pragma once

namespace
{

// mean / median / p90 / max of a list of durations (sorted in place), as a JSON member
struct Quantiles
{
  double mean = 0, median = 0, p90 = 0, max = 0;
  explicit Quantiles(std::vector<double>& v)
  {
    std::sort(v.begin(), v.end());
    for (double x : v)
      mean += x / v.size();
    median = v[v.size() / 2];
    p90 = v[v.size() * 9 / 10];
    max = v.back();
  }
  void json(FILE* fp, const char* name) const { std::fprintf(fp, "\"%s\": {\"mean\": %.2f, \"median\": %.2f, \"p90\": %.2f, \"max\": %.2f}", name, mean, median, p90, max); }
};

// k_slab_emit's stamp buffer (nullptr unless VOFOD_LDS_PROF is set): allocated on the first launch that wants it
int slab_emit_prof_buffer(vofod_handle* h, unsigned long long*& d_prof)
{
  if (!h->d_prof_slab && std::getenv("VOFOD_LDS_PROF"))
    HIPCHK(h->d_prof_slab.alloc(16 * 4096));
  d_prof = h->d_prof_slab;
  return VOFOD_OK;
}

// VOFOD_LDS_PROF: the phases of k_slab_emit's n workgroups, behind its launch (the stream is synchronised)
int print_slab_emit_prof(vofod_handle* h, uint32_t n)
{
  std::vector<unsigned long long> all(16 * n);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(all.data(), h->d_prof_slab, sizeof(unsigned long long) * 16 * n, hipMemcpyDeviceToHost));
  const unsigned long long* t = all.data();
  std::fprintf(stderr, "[k_slab_emit] keys %.1f | zero %.1f mark %.1f count+scan %.1f out+emit %.1f us (all slabs of frame 0)\n", t[0] * 0.01, t[1] * 0.01, t[2] * 0.01, t[3] * 0.01, t[4] * 0.01);
  unsigned long long t0 = ~0ull, t1 = 0;
  for (uint32_t f = 0; f < n; f++)
  {
    t0 = std::min(t0, all[16 * f + 5]);
    t1 = std::max(t1, all[16 * f + 6]);
  }
  double smax = 0;
  std::vector<double> dur;
  std::vector<std::pair<double, uint32_t>> byd;
  for (uint32_t f = 0; f < n; f++)
  {
    dur.push_back((all[16 * f + 6] - all[16 * f + 5]) * 0.01);
    byd.push_back({dur.back(), f});
    smax = std::max(smax, (all[16 * f + 5] - t0) * 0.01);
  }
  std::sort(byd.begin(), byd.end());
  for (size_t q : {size_t(0), byd.size() / 4, byd.size() / 2, 3 * byd.size() / 4, byd.size() - 1})
  {
    const uint32_t f = byd[q].second;
    std::fprintf(stderr, "[k_slab_emit]   frame %u: %.1f us, keys %llu, zero %.1f mark %.1f count %.1f emit %.1f\n", f, byd[q].first, all[16 * f + 7], all[16 * f + 1] * 0.01, all[16 * f + 2] * 0.01,
                 all[16 * f + 3] * 0.01, all[16 * f + 4] * 0.01);
  }
  const Quantiles q(dur);
  std::fprintf(stderr, "[k_slab_emit] %u workgroups: span %.1f us, per-workgroup min %.1f mean %.1f max %.1f us, latest start +%.1f us\n", n, (t1 - t0) * 0.01, dur.front(), q.mean, q.max, smax);
  return VOFOD_OK;
}

// The frame kernel's stamp slots for this launch (nullptr unless VOFOD_LDS_PROF is set).  =2: a submitted batch keeps the stamps in
// its ticket's slots and prints them when it is collected - the phases as they last with the other batches' kernels beside them
// (=1 synchronises behind every launch).
int frame_prof_slots(vofod_handle* h, Workspace& ws, unsigned long long*& d_prof)
{
  DevBuf<unsigned long long>& d_prof_all = h->d_prof_ccl;
  if (!d_prof_all && std::getenv("VOFOD_LDS_PROF"))
  {
    HIPCHK(d_prof_all.alloc(FR_PROF_WORDS));  // (the frames' slots, then the per-wave values of the input pass)
    HIPCHK(hipMemset(d_prof_all, 0, sizeof(unsigned long long) * FR_PROF_WORDS));
  }
  ws.prof_deferred = false;
  uint32_t prof_slot0 = 0;
  if (d_prof_all && std::atoi(std::getenv("VOFOD_LDS_PROF") ? std::getenv("VOFOD_LDS_PROF") : "0") == 2 && ws.F <= 256)
    for (int t = 0; t < vofod_handle::MAX_INFLIGHT; t++)
      if (&ws == h->slot(t))
      {
        ws.prof_deferred = true;
        prof_slot0 = 256u * static_cast<uint32_t>(t);
      }
  ws.prof_slot0 = prof_slot0;
  d_prof = d_prof_all ? d_prof_all + 32 * static_cast<size_t>(prof_slot0) : nullptr;
  return VOFOD_OK;
}

// Phase durations of the frame kernel's workgroups from the stamps in slots [s0, s0 + cnt) of the handle's stamp buffer.
// VOFOD_LDS_PROF=1: after every launch (the stream is synchronised: one batch at a time); =2: when the batch is collected (batches
// in flight keep their own slots: the phases as they last in the pipeline).
int print_frame_prof(vofod_handle* h, uint32_t s0, uint32_t cnt, bool sync)
{
  unsigned long long* d_prof = h->d_prof_ccl;
  std::vector<unsigned long long> t(32 * cnt);
  if (sync)
    HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(t.data(), d_prof + 32 * static_cast<size_t>(s0), sizeof(unsigned long long) * 32 * cnt, hipMemcpyDeviceToHost));
  // the input pass per wave: [frame][wave]{clock at which the wave left the loop, ticks it waited for its pieces}
  unsigned long long* d_wave = d_prof + 32 * static_cast<size_t>(FR_PROF_FRAMES) + 32 * static_cast<size_t>(s0);
  std::vector<unsigned long long> tw(32 * cnt);
  HIPCHK(hipMemcpy(tw.data(), d_wave, sizeof(unsigned long long) * 32 * cnt, hipMemcpyDeviceToHost));
  if (const char* rawf = std::getenv("VOFOD_LDS_PROF_RAW"))
  {
    // raw mode: nothing is formatted while the pipeline runs (the JSON table below costs the host ~100 us per launch: 840 k instead
    // of 950 k frames/s) - every frame's start, end and CU are kept and written to the named file when the process ends
    // (tools/cu_gaps.py lays the frames of every CU end to end)
    struct RawLog
    {
      std::vector<unsigned long long> v;  // launch, start, end, hw id per frame
      std::string path;
      uint64_t launch = 0;
      ~RawLog()
      {
        if (FILE* fp = std::fopen(path.c_str(), "w"))
        {
          for (size_t i = 0; i + 3 < v.size(); i += 4)
            std::fprintf(fp, "%llu %.2f %.2f %u %u %u %u\n", v[i], v[i + 1] * 0.01, v[i + 2] * 0.01, static_cast<unsigned>(v[i + 3] >> 32) & 15u, static_cast<unsigned>(v[i + 3] >> 13) & 7u,
                         static_cast<unsigned>(v[i + 3] >> 12) & 1u, static_cast<unsigned>(v[i + 3] >> 8) & 15u);
          std::fclose(fp);
        }
      }
    };
    static RawLog log;
    log.path = rawf;
    for (uint32_t f = 0; f < cnt; f++)
      if (t[32 * f + 13])
      {
        const unsigned long long rec[4] = {log.launch, t[32 * f], t[32 * f + 13], t[32 * f + 21]};
        log.v.insert(log.v.end(), rec, rec + 4);
      }
    log.launch++;
    HIPCHK(hipMemsetAsync(d_prof + 32 * static_cast<size_t>(s0), 0, sizeof(unsigned long long) * 32 * cnt, h->stream));
    HIPCHK(hipMemsetAsync(d_wave, 0, sizeof(unsigned long long) * 32 * cnt, h->stream));
    return VOFOD_OK;
  }
  static const char* names[13] = {"bits", "prefix", "words", "rank-a/b", "rank-c", "emit", "extras", "probe", "adjacent", "far", "exact", "minima+stats", "labels"};  // (rank-a/b includes the counting pass: stamp 14 splits them)
  std::vector<std::pair<double, uint32_t>> byd;
  unsigned long long t0 = ~0ull, t1 = 0;
  for (uint32_t f = 0; f < cnt; f++)
  {
    if (!t[32 * f + 13])
      continue;
    byd.push_back({(t[32 * f + 13] - t[32 * f]) * 0.01, f});
    t0 = std::min(t0, t[32 * f]);
    t1 = std::max(t1, t[32 * f + 13]);
  }
  std::sort(byd.begin(), byd.end());
  double mean = 0;
  for (auto& b : byd)
    mean += b.first / byd.size();
  for (size_t q : {size_t(0), byd.size() / 2, byd.size() - 1})
  {
    if (byd.empty())
      break;
    const uint32_t f = byd[q].second;
    if (t[32 * f + 31] == ~0ull)
    {
      // a close-first frame: its own phases behind the emission
      auto us = [&](int a, int b) { return (t[32 * f + b] - t[32 * f + a]) * 0.01; };
      // (stamps 3 -> 15 -> 14: closebits, then the counting pass)
      const double t_count = us(15, 14), t_closebits = us(3, 15);
      std::fprintf(stderr,
                   "[k_frame_lds_far] frame %u: %.1f us | keys %llu V %llu bricks %llu pure-far bricks %llu far clusters %llu candidate members %llu | input+fragile %.1f prefix %.1f words %.1f count %.1f closebits "
                   "%.1f rank-a/b %.1f rank-c %.1f emit %.1f extras %.1f near+far %.1f open %.1f stats %.1f table %.1f members %.1f\n",
                   f, byd[q].first, t[32 * f + 27], t[32 * f + 29], t[32 * f + 26], t[32 * f + 24], t[32 * f + 25], t[32 * f + 30], us(0, 1), us(1, 2), us(2, 3), t_count, t_closebits, us(14, 4), us(4, 5),
                   us(5, 6), us(6, 7), us(7, 8), us(8, 9), us(9, 10), us(10, 11), us(11, 13));
      continue;
    }
    std::fprintf(stderr, "[k_frame_lds] frame %u: %.1f us | keys %llu V %llu bricks %llu extras %llu hits %llu open %llu surviving %llu |", f, byd[q].first, t[32 * f + 27], t[32 * f + 29],
                 t[32 * f + 26], t[32 * f + 28], t[32 * f + 24], t[32 * f + 25], t[32 * f + 30]);
    for (int i = 0; i < 13; i++)
      std::fprintf(stderr, " %s %.1f", names[i], (t[32 * f + i + 1] - t[32 * f + i]) * 0.01);
    std::fprintf(stderr, " (count %.1f of rank-a/b; %llu bricks outside the largest component, %llu far hits)\n", (t[32 * f + 14] - t[32 * f + 3]) * 0.01, t[32 * f + 31] & 0xffffffffull,
                 t[32 * f + 31] >> 32);
  }
  if (!byd.empty())
    std::fprintf(stderr, "[k_frame_lds] %zu workgroups: span %.1f us, mean %.1f us\n", byd.size(), (t1 - t0) * 0.01, mean);
  // VOFOD_LDS_PROF_JSON=<file>: the phase table of the close-first frames of this launch (mean / median / max over the
  // frames, us), one JSON object per launch appended to the file - profiles/r05_frame_phases.json is made of these
  if (const char* jf = std::getenv("VOFOD_LDS_PROF_JSON"); jf && !byd.empty() && t[32 * byd[0].second + 31] == ~0ull)
  {
    static const int cuts[][2] = {{0, 16}, {16, 17}, {17, 18}, {18, 19}, {19, 20}, {20, 1}, {1, 2}, {2, 3}, {15, 14}, {3, 15}, {14, 4}, {4, 5}, {5, 6}, {6, 7}, {7, 8}, {8, 9}, {9, 10}, {10, 11}, {11, 13}, {0, 13}};
    static const char* cnames[] = {"input", "input_wait", "grid", "grid_wait", "fragile", "fragile_wait", "prefix", "words", "count", "closebits", "rank_ab", "rank_c", "emit", "extras_restore", "cf_edges", "cf_open", "cf_stats", "cf_table", "cf_members", "total"};
    if (FILE* fp = std::fopen(jf, "a"))
    {
      double busy = 0;
      for (auto& b : byd)
        busy += b.first;
      std::fprintf(fp, "{\"frames\": %zu, \"span_us\": %.1f, \"t0_abs_us\": %.1f, \"busy_us_sum\": %.1f, \"phases\": {", byd.size(), (t1 - t0) * 0.01, t0 * 0.01, busy);
      for (size_t c = 0; c < sizeof(cuts) / sizeof(cuts[0]); c++)
      {
        std::vector<double> v;
        for (auto& b : byd)
          v.push_back((t[32 * b.second + cuts[c][1]] - t[32 * b.second + cuts[c][0]]) * 0.01);
        std::fprintf(fp, "%s", c ? ", " : "");
        Quantiles(v).json(fp, cnames[c]);
      }
      // where in time the frames' workgroups started and ended relative to the first start (one CU per frame: late starts = a busy chip)
      std::vector<double> st, en;
      for (auto& b : byd)
      {
        st.push_back((t[32 * b.second] - t0) * 0.01);
        en.push_back((t[32 * b.second + 13] - t0) * 0.01);
      }
      std::sort(st.begin(), st.end());
      std::sort(en.begin(), en.end());
      // the input pass wave by wave (us from the frame's start): when the mean wave and the last wave left the loop, and the share
      // of its time in the loop the mean wave spent waiting for loads
      std::vector<double> w_mean, w_last, w_share;
      for (auto& b : byd)
      {
        const unsigned long long* w = &tw[32 * b.second];
        const unsigned long long f0 = t[32 * b.second];
        double e_sum = 0, e_max = 0, s_sum = 0;
        int nw = 0;
        for (int k = 0; k < FR_THREADS / 64; k++)
          if (w[2 * k] > f0)
          {
            const double e = (w[2 * k] - f0) * 0.01;
            e_sum += e;
            e_max = std::max(e_max, e);
            s_sum += w[2 * k + 1] / e;  // (ticks of 10 ns over us: per cent)
            nw++;
          }
        if (nw)
        {
          w_mean.push_back(e_sum / nw);
          w_last.push_back(e_max);
          w_share.push_back(s_sum / nw);
        }
      }
      std::fprintf(fp, "}");
      // the pure-far lists' lengths (slot 24), and how many of the frames keep the frame-wide rank passes for a long list
      {
        std::vector<double> npf;
        size_t over = 0;
        for (auto& b : byd)
        {
          npf.push_back(static_cast<double>(t[32 * b.second + 24]));
          over += t[32 * b.second + 24] > FR_LEAN_RANKS_MAX ? 1 : 0;
        }
        std::fprintf(fp, ", \"pure_far\": {");
        Quantiles(npf).json(fp, "bricks");  // (sorts)
        std::fprintf(fp, ", \"min\": %.0f, \"p10\": %.0f, \"over_lean_ranks_max\": %zu}", npf.front(), npf[npf.size() / 10], over);
      }
      // the lean count (slot 28 above the extras' 24 bits: the list's length, 20 bits; Vc, 16 bits; bit 63: counted from the list): the
      // lists' lengths and the voxels with a counter, and how many of the frames walked every code instead
      {
        std::vector<double> nlc, vc;
        size_t from_list = 0, over = 0;
        for (auto& b : byd)
        {
          const unsigned long long x = t[32 * b.second + 28];
          nlc.push_back(static_cast<double>((x >> 24) & 0xfffffull));
          vc.push_back(static_cast<double>((x >> 44) & 0xffffull));
          from_list += x >> 63;
          over += ((x >> 24) & 0xfffffull) > FR_LEAN_COUNT_MAX ? 1 : 0;
        }
        std::fprintf(fp, ", \"lean_count\": {");
        Quantiles(nlc).json(fp, "entries");
        std::fprintf(fp, ", ");
        Quantiles(vc).json(fp, "counters");
        std::fprintf(fp, ", \"from_list\": %zu, \"walked\": %zu, \"over_lean_count_max\": %zu}", from_list, byd.size() - from_list, over);
      }
      if (!w_mean.empty())
      {
        std::fprintf(fp, ", \"input_waves\": {");
        Quantiles(w_mean).json(fp, "mean_wave_end");
        std::fprintf(fp, ", ");
        Quantiles(w_last).json(fp, "last_wave_end");
        std::fprintf(fp, ", ");
        Quantiles(w_share).json(fp, "load_wait_pct");
        std::fprintf(fp, "}");
      }
      std::fprintf(fp, ", \"start_us\": {\"median\": %.1f, \"max\": %.1f}, \"end_us\": {\"median\": %.1f, \"max\": %.1f}", st[st.size() / 2], st.back(), en[en.size() / 2], en.back());
      // the classification tail of the same frames (k_tail_far's stamps): boxes + gates, flood fills, records; and how long after
      // the frame's own end its tail started
      std::vector<double> bx, ex, fi, to, lag;
      for (auto& b : byd)
      {
        const unsigned long long a0 = t[32 * b.second + 22], pk = t[32 * b.second + 23];
        if (!a0)
          continue;
        const double d1 = (pk & 0xfffffull) * 0.01, d2 = ((pk >> 20) & 0xfffffull) * 0.01, d3 = ((pk >> 40) & 0xfffffull) * 0.01;
        bx.push_back(d1);
        ex.push_back(d2 - d1);
        fi.push_back(d3 - d2);
        to.push_back(d3);
        lag.push_back((static_cast<double>(a0) - static_cast<double>(t[32 * b.second + 13])) * 0.01);
      }
      if (!to.empty())
      {
        std::fprintf(fp, ", \"tail\": {");
        Quantiles(bx).json(fp, "boxes_gates");
        std::fprintf(fp, ", ");
        Quantiles(ex).json(fp, "flood_fills");
        std::fprintf(fp, ", ");
        Quantiles(fi).json(fp, "records");
        std::fprintf(fp, ", ");
        Quantiles(to).json(fp, "total");
        std::fprintf(fp, ", ");
        Quantiles(lag).json(fp, "start_after_frame_end");
        std::fprintf(fp, "}");
      }
      std::fprintf(fp, "}\n");
      std::fclose(fp);
    }
  }
  HIPCHK(hipMemset(d_prof + 32 * static_cast<size_t>(s0), 0, sizeof(unsigned long long) * 32 * cnt));
  HIPCHK(hipMemset(d_wave, 0, sizeof(unsigned long long) * 32 * cnt));
  return VOFOD_OK;
}

// VOFOD_LDS_PROF=2: the frame kernel's stamps of this batch are printed when it is collected
int print_deferred_prof(vofod_handle* h, Workspace& ws, uint32_t n)
{
  if (!ws.prof_deferred || !h->d_prof_ccl)
    return VOFOD_OK;
  ws.prof_deferred = false;
  return print_frame_prof(h, ws.prof_slot0, n, false);
}

}  // namespace
