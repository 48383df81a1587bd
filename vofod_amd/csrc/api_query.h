// What the map-query entry points share on the host (included by api_render.h, api_match.h and api_distance.h, each for itself):
// the one reader of their environment switches, the one burst dispatcher, and the upload half of the staging of host-resident scans
// (scan_stage.h has the HIP-free half).
#pragma once

#include <cstdlib>
#include <type_traits>

#include "scan_stage.h"

namespace
{

// an integer environment switch of the query calls, read per call: unset or anything but a positive number is `kept`.
//   VOFOD_RENDER_BURST=1|2|4|8  (diagnostics, tools/map_render_bench.py) the burst lengths of k_map_render measured beside the one kept
//   VOFOD_MATCH_BURST=1|2|4|8   (diagnostics) the same for the scoring walk of the two match calls
//   VOFOD_MATCH_CHUNK=n         (diagnostics, tools/map_match_bench.py, and the tests' way to make a small scan straddle chunks) the
//                               points per block of the scoring walk
inline uint32_t env_int(const char* name, uint32_t kept)
{
  if (const char* e = std::getenv(name))
  {
    const long v = std::atol(e);
    if (v > 0 && v <= 0x7fffffffL)
      return static_cast<uint32_t>(v);
  }
  return kept;
}

// a run-time burst of 1 / 2 / 4 / 8 as a compile-time one: f(std::integral_constant<int, burst>), anything else selects KEPT
template <int KEPT, class F>
inline void with_burst(uint32_t burst, F&& f)
{
  switch (burst)
  {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, KEPT>{});
  }
}

// the host-resident scans of a query call on the device (scan_stage.h: what of each scan is `want`ed is gathered into one block,
// pose tables first), by ONE copy on the stream; h->qstage.at[v] is scan v as the kernels read it, device-resident scans
// untouched.  The block is free again behind the call's synchronisation.
inline int stage_scans(vofod_handle* h, const vofod_scan* scans, size_t n_scans, uint32_t want)
{
  const uint32_t width = static_cast<uint32_t>(h->sp.sensor_hrays), n = width * static_cast<uint32_t>(h->sp.sensor_vrays);
  const size_t words = vss::ScanStage::words(scans, n_scans, width, n, want);
  HIPCHK(h->d_qstage.reserve(words));
  h->qstage.gather(scans, n_scans, width, n, want, reinterpret_cast<uintptr_t>(h->d_qstage.p));
  if (words)
    HIPCHK(hipMemcpyAsync(h->d_qstage, h->qstage.block.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  return VOFOD_OK;
}

}  // namespace
