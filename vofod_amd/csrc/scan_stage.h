// Host-resident scans of the query calls (vofod_map_render_scans, vofod_map_match, vofod_map_match_field) on their way to the
// device: ONE block of 4-byte words per call - the pose tables of the list's host scans first, their columns behind them - filled
// here and uploaded by the driver with one copy (stage_scans, api_query.h).  A table is width * 48 bytes, so with the tables in
// front every staged table stays 16-byte aligned in a 16-byte aligned block (the aligned pose loads of k_map_render and of
// k_match_points<.., POSE16> are picked as for a table the caller aligned); a staged column has stride 4.  Device-resident scans
// pass through: their pointers and their stride come back as they were given.
// No HIP in this header: it is host pointer arithmetic over caller memory at any stride and alignment, and scan_stage_check.cpp
// runs it alone under the host compiler's sanitizers (tests/test_scan_stage_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vofod.h"

namespace vss
{

// n 4-byte elements at `stride` bytes from one another, from any address, behind one another at dst
inline void gather4(void* dst, const void* src, size_t stride, size_t n)
{
  if (stride == 4 && n)
    std::memcpy(dst, src, 4 * n);  // (packed already: a pose table, or a column the caller packed)
  else
    for (size_t i = 0; i < n; i++)
      std::memcpy(static_cast<char*>(dst) + 4 * i, static_cast<const char*>(src) + i * stride, 4);
}

// what a call reads of its scans: col_tfs where a scan carries one, the range column where it carries one, the x, y and z columns
enum : uint32_t
{
  WANT_TABLES = 1,
  WANT_RANGE = 2,
  WANT_POINTS = 4
};

// one scan as the kernels read it (vmm::ScanSource is this struct): device addresses; what was not asked for, or is not there, is null
struct Staged
{
  const char* range;   // range image: uint32 millimetres, pixel i at range + i * stride
  const char* x;       // point scan: floats at x / y / z + i * stride
  const char* y;
  const char* z;
  uint64_t stride;
  const float* poses;  // the scan's col_tfs, nullptr: none
};

struct ScanStage
{
  std::vector<uint32_t> block;  // what the driver uploads
  std::vector<Staged> at;       // one entry per scan

  // what is read of scan s, where the caller has it
  static Staged wanted(const vofod_scan& s, uint32_t want)
  {
    const bool range = (want & WANT_RANGE) && s.range, points = (want & WANT_POINTS) && s.x && s.y && s.z;
    const auto col = [](bool take, const void* p) { return take ? static_cast<const char*>(p) : nullptr; };
    return Staged{col(range, s.range), col(points, s.x), col(points, s.y), col(points, s.z), s.stride_bytes, (want & WANT_TABLES) ? s.col_tfs : nullptr};
  }

  // the words of the block for this list: the size of the device allocation, known before its address is
  static size_t words(const vofod_scan* scans, size_t n_scans, uint32_t width, uint32_t n_px, uint32_t want)
  {
    size_t n = 0;
    for (size_t v = 0; v < n_scans; v++)
      if (const Staged e = wanted(scans[v], want); scans[v].memspace == VOFOD_MEM_HOST)
        n += (e.poses ? 12 * static_cast<size_t>(width) : 0) + static_cast<size_t>(n_px) * (!!e.range + !!e.x + !!e.y + !!e.z);
    return n;
  }

  // fills `block` and `at`.  d_block is the address the block will have on the device: byte offsets are added to it, nothing is
  // read or written there.
  void gather(const vofod_scan* scans, size_t n_scans, uint32_t width, uint32_t n_px, uint32_t want, uintptr_t d_block)
  {
    block.clear();
    at.resize(n_scans);
    const auto stage = [&](const void* src, size_t stride, size_t n) {  // n words behind the block's end; their address on the device
      const size_t i = block.size();
      block.resize(i + n);
      gather4(block.data() + i, src, stride, n);
      return d_block + 4 * i;
    };
    for (size_t v = 0; v < n_scans; v++)  // every table first
      if (at[v] = wanted(scans[v], want); scans[v].memspace == VOFOD_MEM_HOST && at[v].poses)
        at[v].poses = reinterpret_cast<const float*>(stage(at[v].poses, 4, 12 * static_cast<size_t>(width)));
    for (size_t v = 0; v < n_scans; v++)
      if (scans[v].memspace == VOFOD_MEM_HOST)
      {
        for (const char** c : {&at[v].range, &at[v].x, &at[v].y, &at[v].z})
          if (*c)
            *c = reinterpret_cast<const char*>(stage(*c, scans[v].stride_bytes, n_px));
        at[v].stride = 4;
      }
  }
};

}  // namespace vss
