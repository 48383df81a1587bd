// The query calls' staging of host-resident scans (scan_stage.h) on the CPU: lists of scans of a 3 x 2 sensor at the strides, the
// addresses and the mixtures at which the gather can go wrong, every caller buffer allocated to the byte, so that the host compiler's
// sanitizers see any access beside one; every staged word is compared with a plain indexed reference kept beside the buffers.
//   scan_stage_check    exit status 0 and "scan_stage_check: ok", or the first failed line and exit status 1
// Includes scan_stage.h and nothing else of the library (tests/test_scan_stage_cpu.py builds it with the host compiler and
// -fsanitize=address,undefined, and runs it).
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "scan_stage.h"

#define CHECK(cond)                                                          \
  do                                                                         \
  {                                                                          \
    if (!(cond))                                                             \
    {                                                                        \
      std::fprintf(stderr, "scan_stage_check:%d: %s\n", __LINE__, #cond);   \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

constexpr uint32_t W = 3, H = 2, N = W * H;  // (a width that is no multiple of 4)
constexpr uintptr_t D_BLOCK = 0x7f0000001000u;  // where the block is said to stand on the device: 16-byte aligned, never dereferenced

// one scan of the list with the memory its pointers point into and, for a host scan, the values that lie there
struct Source
{
  vofod_scan scan{};
  std::unique_ptr<char[]> cols[4];  // range, x, y, z: each of exactly 1 + (N - 1) * stride + 4 bytes, the column at the odd address + 1
  std::unique_ptr<float[]> table;   // exactly 12 * W floats
  uint32_t col_ref[4][N];
  uint32_t tab_ref[12 * W];
};

static uint32_t value(size_t v, uint32_t c, uint32_t i) { return 0xA5000000u + (static_cast<uint32_t>(v) << 16) + (c << 8) + i; }

// scan v of a list.  has: which of range (bit 0) and points (bit 1) it carries
static void make_scan(Source& src, size_t v, bool host, size_t stride, uint32_t has, bool table)
{
  vofod_scan& s = src.scan;
  s.stride_bytes = stride;
  s.width = W, s.height = H;
  s.memspace = host ? VOFOD_MEM_HOST : VOFOD_MEM_DEVICE;
  const void** member[4] = {&s.range, &s.x, &s.y, &s.z};
  for (uint32_t c = 0; c < 4; c++)
  {
    if (!(has & (c == 0 ? 1u : 2u)))
      continue;
    if (!host)
    {  // an opaque value: it must come back as it is
      *member[c] = reinterpret_cast<const void*>(static_cast<uintptr_t>(0xD0000000u + (v << 12) + 4 * c));
      continue;
    }
    src.cols[c].reset(new char[1 + (N - 1) * stride + 4]);
    char* base = src.cols[c].get() + 1;
    for (uint32_t i = 0; i < N; i++)
    {
      src.col_ref[c][i] = value(v, c, i);
      std::memcpy(base + i * stride, &src.col_ref[c][i], 4);
    }
    *member[c] = base;
  }
  if (table && host)
  {
    src.table.reset(new float[12 * W]);
    for (uint32_t k = 0; k < 12 * W; k++)
    {
      src.tab_ref[k] = value(v, 7, k);
      std::memcpy(&src.table[k], &src.tab_ref[k], 4);
    }
    s.col_tfs = src.table.get();
  }
  else if (table)
    s.col_tfs = reinterpret_cast<const float*>(static_cast<uintptr_t>(0xE0000000u + (v << 12) + 4));  // (4-byte aligned, as a device table may be)
}

// stage `n` scans with `want` and hold every word and every pointer to the reference
static void check_list(const Source* src, size_t n, uint32_t want)
{
  std::unique_ptr<vofod_scan[]> scans(new vofod_scan[n]);  // (exactly n: a read behind the list is seen)
  for (size_t v = 0; v < n; v++)
    scans[v] = src[v].scan;
  // the layout, restated: every host table that is asked for, in list order; behind them every host column, in list order, range first
  size_t n_tab_words = 0, total = 0;
  for (size_t v = 0; v < n; v++)
    if (scans[v].memspace == VOFOD_MEM_HOST && (want & vss::WANT_TABLES) && scans[v].col_tfs)
      n_tab_words += 12 * W;
  total = n_tab_words;
  for (size_t v = 0; v < n; v++)
    if (scans[v].memspace == VOFOD_MEM_HOST)
      total += (((want & vss::WANT_RANGE) && scans[v].range ? 1 : 0) + ((want & vss::WANT_POINTS) && scans[v].x ? 3 : 0)) * N;
  CHECK(vss::ScanStage::words(scans.get(), n, W, N, want) == total);
  vss::ScanStage st;
  st.block.assign(7, 0xdeadbeefu);  // (what an earlier call left)
  st.at.resize(5);
  st.gather(scans.get(), n, W, N, want, D_BLOCK);
  CHECK(st.block.size() == total && st.at.size() == n);
  size_t i_tab = 0, i_col = n_tab_words;
  for (size_t v = 0; v < n; v++)
  {
    const vofod_scan& s = scans[v];
    const vss::Staged& e = st.at[v];
    const bool host = s.memspace == VOFOD_MEM_HOST;
    const char* got[4] = {e.range, e.x, e.y, e.z};
    const void* given[4] = {s.range, s.x, s.y, s.z};
    CHECK(e.stride == (host ? 4 : s.stride_bytes));
    if (!((want & vss::WANT_TABLES) && s.col_tfs))
      CHECK(e.poses == nullptr);
    else if (!host)
      CHECK(e.poses == s.col_tfs);
    else
    {
      CHECK(reinterpret_cast<uintptr_t>(e.poses) == D_BLOCK + 4 * i_tab && reinterpret_cast<uintptr_t>(e.poses) % 16 == 0);
      for (uint32_t k = 0; k < 12 * W; k++)
        CHECK(st.block[i_tab + k] == src[v].tab_ref[k]);
      i_tab += 12 * W;
    }
    for (uint32_t c = 0; c < 4; c++)
    {
      if (!((want & (c == 0 ? vss::WANT_RANGE : vss::WANT_POINTS)) && given[c]))
        CHECK(got[c] == nullptr);
      else if (!host)
        CHECK(got[c] == given[c]);
      else
      {
        CHECK(i_col >= n_tab_words && i_col + N <= total);  // (behind every table, inside the block)
        CHECK(reinterpret_cast<uintptr_t>(got[c]) == D_BLOCK + 4 * i_col);
        for (uint32_t i = 0; i < N; i++)
          CHECK(st.block[i_col + i] == src[v].col_ref[c][i]);
        i_col += N;
      }
    }
  }
  CHECK(i_tab == n_tab_words && i_col == total);  // (every word of the block is a table's or a column's: nothing overlaps, nothing is left)
}

int main()
{
  // gather4 alone: strides 4, 5 and 48 from an odd address, and nothing at all
  for (size_t stride : {size_t(4), size_t(5), size_t(48)})
  {
    Source s;
    make_scan(s, 0, true, stride, 1, false);
    std::unique_ptr<uint32_t[]> out(new uint32_t[N]);
    vss::gather4(out.get(), s.scan.range, stride, N);
    for (uint32_t i = 0; i < N; i++)
      CHECK(out[i] == s.col_ref[0][i]);
    vss::gather4(nullptr, nullptr, stride, 0);
  }
  const uint32_t wants[] = {0u,
                            vss::WANT_TABLES,
                            vss::WANT_RANGE,
                            vss::WANT_POINTS,
                            vss::WANT_TABLES | vss::WANT_RANGE,
                            vss::WANT_TABLES | vss::WANT_POINTS,
                            vss::WANT_TABLES | vss::WANT_RANGE | vss::WANT_POINTS};
  for (uint32_t want : wants)
  {
    check_list(nullptr, 0, want);
    for (size_t stride : {size_t(4), size_t(5), size_t(48)})
      for (uint32_t has = 1; has <= 3; has++)
        for (int table = 0; table < 2; table++)
        {
          // one scan, host and "device"
          Source one[2];
          make_scan(one[0], 0, true, stride, has, table != 0);
          make_scan(one[1], 1, false, stride, has, table != 0);
          check_list(&one[0], 1, want);
          check_list(&one[1], 1, want);
          // three scans in one list: a host scan without a table in front (the first staged column must still lie behind the
          // tables of the scans after it), a device scan in the middle, a host scan of another stride and make-up at the end
          Source three[3];
          make_scan(three[0], 0, true, stride, has, false);
          make_scan(three[1], 1, false, 12, 3, table != 0);
          make_scan(three[2], 2, true, stride == 5 ? 48 : 5, 4 - has, true);
          check_list(three, 3, want);
          // ... and every one of them host-resident with a table: three tables, each at a multiple of 16 bytes
          Source tabs[3];
          for (size_t v = 0; v < 3; v++)
            make_scan(tabs[v], v, true, stride, has, true);
          check_list(tabs, 3, want);
        }
  }
  std::puts("scan_stage_check: ok");
  return 0;
}
