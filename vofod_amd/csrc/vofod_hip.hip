// libvofod_hip.so — the product: C++ host driver + hand-written gfx950 kernels behind include/vofod.h.
// One handle owns one HIP stream, the three voxel maps in HBM and a per-frame workspace; a scan (or a
// batch of independent scans, one grid.y slice each) is one stream-ordered chain of kernels followed by
// a single read-back of the small cluster table, after which the host runs the sequential
// classification tail (host_tail.h) on the few candidate clusters.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "chain_plan.h"
#include "common.h"
#include "device_mem.h"
#include "host_tail.h"
#include "thread_pool.h"
#include "kernels_brick.h"
#include "kernels_brick_lds.h"
#include "kernels_classify.h"
#include "kernels_frame.h"
#include "kernels_cluster.h"
#include "kernels_raycast.h"
#include "kernels_slab.h"
#include "kernels_tail.h"
#include "kernels_far.h"
#include "kernels_voxelize.h"
#include "mapsync.h"
#include "range_decode.h"
#include "point_deskew.h"
#include "detection_points.h"
#include "detection_pixels.h"
#include "map_shift.h"
#include "scan_stage.h"
#include "map_render.h"
#include "map_match.h"
#include "map_distance.h"
#include "world_store.h"
#include "world_sync.h"

using namespace vk;

namespace
{

constexpr uint32_t SPEC_C = 192;   // cluster records read back speculatively with the header
constexpr uint32_t SPEC_M = 768;  // candidate members read back speculatively

struct CandMemberX
{
  uint32_t root, v;
  float x, y, z;
  uint32_t count;
};

struct PackedFrame
{
  FrameHdr hdr;
  uint32_t pad[32 - sizeof(FrameHdr) / 4];
  ClusterRec table[SPEC_C];
  CandMemberX members[SPEC_M];
};
static_assert(sizeof(FrameHdr) <= 128, "FrameHdr grew past its slot");

// a candidate member with its voxel's centre and point count, as the host tail reads it
__device__ __forceinline__ CandMemberX gather_member(const GridParams& g, uint32_t f, uint32_t t, const CandMember* cand_all, const VoxelArrays& va_all)
{
  const CandMember cm = cand_all[static_cast<size_t>(f) * g.vox_cap + t];
  const float4 p = va_all.pts[static_cast<size_t>(f) * g.vox_cap + cm.v];
  CandMemberX x;
  x.root = cm.root;
  x.v = cm.v;
  x.x = p.x;
  x.y = p.y;
  x.z = p.z;
  x.count = __float_as_uint(p.w);
  return x;
}

__global__ void k_pack(const GridParams g, const FrameHdr* hdrs, const ClusterRec* table_all, const CandMember* cand_all, VoxelArrays va_all, PackedFrame* out)
{
  uint32_t FRAME, BX, GX;
  if (!frame_block(g, FRAME, BX, GX))
    return;
  (void)GX;
  const uint32_t f = FRAME;
  const FrameHdr h = hdrs[f];
  PackedFrame& o = out[f];
  const uint32_t t = BX * blockDim.x + threadIdx.x;
  if (t == 0)
    o.hdr = h;
  if (t < min(h.C, SPEC_C))
    o.table[t] = table_all[static_cast<size_t>(f) * g.vox_cap + t];
  if (t < min(h.n_cand, SPEC_M))
    o.members[t] = gather_member(g, f, t, cand_all, va_all);
}

__global__ void k_gather_members(const GridParams g, uint32_t frame, uint32_t n, const CandMember* cand_all, VoxelArrays va_all, CandMemberX* out)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n)
    out[t] = gather_member(g, frame, t, cand_all, va_all);
}

using clk = std::chrono::steady_clock;
inline double ms_since(const clk::time_point& t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

inline float ulp32(float x)
{
  x = std::fabs(x);
  return std::nextafterf(x, INFINITY) - x;
}

}  // namespace

// VOFOD_CALLTRACE=1 (diagnostics): every HIP call of the driver that keeps the host longer than 0.3 ms is reported
struct SlowCall
{
  const char* what;
  int line;
  std::chrono::steady_clock::time_point t0;
  static bool on()
  {
    static const bool v = std::getenv("VOFOD_CALLTRACE") != nullptr;
    return v;
  }
  SlowCall(const char* w, int l) : what(w), line(l)
  {
    if (on())
      t0 = std::chrono::steady_clock::now();
  }
  ~SlowCall()
  {
    if (!on())
      return;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms > 0.3)
      std::fprintf(stderr, "[vofod calltrace] %.2f ms in %s (line %d)\n", ms, what, line);
  }
};

#define HIPCHK(expr)                                                                                         \
  do                                                                                                         \
  {                                                                                                          \
    SlowCall sc_(#expr, __LINE__);                                                                           \
    const hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess)                                                                                    \
    {                                                                                                        \
      h->err = std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"; \
      return VOFOD_ERR_DEVICE;                                                                               \
    }                                                                                                        \
  } while (0)

// (where there is no handle to report to: the caller returns the error code itself)
#define HIP_TRY(expr)                                      \
  do                                                       \
  {                                                        \
    if (const hipError_t e_ = (expr); e_ != hipSuccess)    \
      return e_;                                           \
  } while (0)

// (the same for the driver's own functions: a status other than VOFOD_OK ends the caller with it)
#define VCHK(expr)                             \
  do                                           \
  {                                            \
    if (const int r_ = (expr); r_ != VOFOD_OK) \
      return r_;                               \
  } while (0)

// ---- optional per-kernel timing with HIP events on the handle's stream (vofod_profile_*) ----------
struct Prof
{
  bool on = false;
  struct Rec
  {
    const char* name;
    hipEvent_t a, b;
  };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  std::vector<DevEvent> owned;  // every event of recs and pool: they live as long as the handle
  hipEvent_t get()
  {
    if (!pool.empty())
    {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    owned.emplace_back();
    (void)owned.back().create(hipEventCreate);
    return owned.back();
  }
};

// One kernel launch on the handle's stream: timed between two events when the profile is on (under `label`: the instantiations
// of one kernel share their algorithmic name), watched by VOFOD_CALLTRACE otherwise.
#define KLAUNCH_AS(h, label, kern, grid, block, ...)                        \
  do                                                                         \
  {                                                                          \
    if ((h)->prof.on)                                                        \
    {                                                                        \
      Prof::Rec r_{label, (h)->prof.get(), (h)->prof.get()};                 \
      (void)hipEventRecord(r_.a, (h)->stream);                               \
      hipLaunchKernelGGL(kern, grid, block, 0, (h)->stream, __VA_ARGS__);    \
      (void)hipEventRecord(r_.b, (h)->stream);                               \
      (h)->prof.recs.push_back(r_);                                          \
    }                                                                        \
    else                                                                     \
    {                                                                        \
      SlowCall sc_(label, __LINE__);                                         \
      hipLaunchKernelGGL(kern, grid, block, 0, (h)->stream, __VA_ARGS__);    \
    }                                                                        \
  } while (0)
#define KLAUNCH(h, kern, grid, block, ...) KLAUNCH_AS(h, #kern, kern, grid, block, __VA_ARGS__)

// A plain struct of pointers (what the kernels take by value; vr::SepState) cannot hold an owner: the owner stands beside it, and
// the struct's member `v` is the view of the owner's allocation.
template <class T>
hipError_t alloc_view(DevBuf<T>& own, T*& v, size_t n)
{
  const hipError_t e = own.alloc(n);
  v = own;
  return e;
}

struct Workspace
{
  uint32_t F = 0, pt_cap = 0, vox_cap = 0, words_cap = 0, nblk_cap = 0, bricks_cap = 0;
  // BrickArrays, VoxelArrays, SlabArrays and FrameScratch go to the kernels by value: they hold plain pointers, and the storage
  // behind every member has its owner here (sa.keys is the view of d_keys)
  BrickArrays ba{};
  VoxelArrays va{};
  SlabArrays sa{};  // key list / extras of the LDS-slab voxelisation
  FrameScratch fs{};  // row tables of the brick-first frame kernel (kernels_frame.h)
  DevBuf<unsigned long long> ba_bricks, fs_rowT, fs_nodeA, fs_bbsave;
  DevBuf<uint32_t> ba_bparent, ba_bmin, ba_bcmin, ba_blist, va_key, va_parent, va_csize, va_cclose, va_bb, sa_extras, sa_counts, fs_rowQ, fs_bmin;
  DevBuf<float4> va_pts, fs_frag;
  DevBuf<int32_t> va_cbox;
  DevBuf<unsigned long long> d_bconn;  // per brick: connectivity mask over the forward stencil (transitive reduction)
  DevBuf<FrameArgs> d_args;
  DevBuf<FrameHdr> d_hdrs;
  DevBuf<unsigned long long> d_bitmaps;
  DevBuf<uint32_t> d_wprefix;
  DevBuf<uint32_t> d_blocksums;
  DevBuf<uint32_t> d_labels;
  DevBuf<ClusterRec> d_table;
  DevBuf<CandMember> d_cand;
  DevBuf<uint32_t> d_keys;  // per frame: the key list of the slab voxeliser, the code list of the frame kernel (fs.keys_cap entries)
  DevBuf<float> d_stage;  // F * pt_cap * 5 words: x, y, z, intensity, range of host-resident inputs
  DevBuf<char> d_stage_aos;  // host-resident array-of-structs clouds (the nodelet's 48-byte ouster_ros::Point) cross the link as they are:
  size_t aos_pitch = 0;      // F * aos_pitch bytes, allocated on first use; the kernels read x / y / z in place at the struct's stride
  // range images of the batch (range_decode.h): their job list, written in pinned memory by stage_inputs and uploaded with the inputs -
  // the n_mjobs jobs that carry a pose per column first, the n_rjobs without behind them (a frame is one or the other: F entries) -
  // and the block host-resident pose tables are staged into: F * width * 12 floats, allocated on the first such scan of this workspace
  DevBuf<vrd::RangeJob> d_rjobs;
  PinBuf<vrd::RangeJob> h_rjobs;
  uint32_t n_mjobs = 0, n_rjobs = 0;
  DevBuf<float> d_poses;
  // point scans with a pose per column (point_deskew.h): their job list, in frame order, written and uploaded like the range jobs; their
  // host tables take slots of the same pose block (a frame is a range image or a point scan: F tables in all)
  DevBuf<vpd::PointJob> d_pjobs;
  PinBuf<vpd::PointJob> h_pjobs;
  uint32_t n_pjobs = 0;
  const float* first_poses = nullptr;  // the device copy of the pose table of the batch's FIRST scan (nullptr: it has none)
  DevBuf<PackedFrame> d_packed;
  PinBuf<PackedFrame> h_packed;
  bool prof_deferred = false;  // VOFOD_LDS_PROF=2: the frame kernel's stamps of this batch are printed when it is collected
  uint32_t prof_slot0 = 0;
  vplan::ChainPlan plan;  // the kernel chain of the launch this workspace holds (chain_plan.h): what the collect half reads of it
  DevBuf<vtd::TailCluster> d_tailc;
  DevBuf<vtd::FrameDets> d_dets;
  PinBuf<vtd::FrameDets> h_dets;  // mapped, coherent
  vtd::FrameDets* h_dets_dev = nullptr;  // the same slots as the device sees them (k_tail_finish writes the records there): an alias, not an allocation
  DevBuf<uint32_t> d_job_be;      // [2][F]: first and one-past-last explore job of every frame
  // per-frame launch arguments in pinned host memory: their upload is a true asynchronous copy, so a batch is enqueued while the
  // previous chain still runs (a copy from pageable memory makes the submitting thread wait for the stream)
  struct PinnedArgs
  {
    PinBuf<FrameArgs> buf;
    FrameArgs& operator[](size_t i) { return buf.p[i]; }
    const FrameArgs& operator[](size_t i) const { return buf.p[i]; }
    FrameArgs* data() { return buf; }
    hipError_t assign(size_t n, const FrameArgs& v)
    {
      HIP_TRY(buf.alloc(n));
      std::fill_n(buf.p, n, v);
      return hipSuccess;
    }
  } h_args;
  std::vector<vofod_scan> job_scans;  // the submitted batch (re-run when the LDS clustering kernel overflows)
  bool bitmap_clean = false;   // the occupancy bitmaps are all-zero (k_finalize clears the words it used)
  vofod_dyn_params job_dp{};   // the dynamic parameters the pending batch was submitted with
  bool rerun = false;          // the next launch repeats this workspace's batch (LDS overflow): frame arguments and staged columns are kept
  DevBuf<CandMemberX> d_members_big;  // vox_cap gathered candidate members: read-back of a frame whose list exceeds the packed slot
  // vofod_detection_points: what the record builders (frames_collect.h) returned last from this workspace - one entry per detection,
  // in the order returned.  Valid from the builder's return until the workspace is taken again (launch_frames, stage_inputs), the
  // map is replaced (vofod_reset, vofod_map_apply) or a failed call leaves nothing to answer for.
  struct DetRef
  {
    uint32_t id, frame, root, n_points;
  };
  std::vector<DetRef> det_refs;
  bool det_valid = false;
  bool det_submitted = false;  // ... by vofod_batch_collect (the ticket's source) rather than a synchronous call (VOFOD_POINTS_SYNC)
  uint32_t det_vox_cap = 0;    // stride of the frame slots the batch ran with
  // vofod_detection_pixels reads the frames' columns as well (detection_pixels.h lists their writers): the GridParams of the launch
  // (crop boxes, leaf), and the counts of the sizing kernel once a call has asked for them
  GridParams det_g{};
  std::vector<vpx::PixSize> det_px_sizes;
  void det_begin(bool submitted, const GridParams& g)
  {
    det_refs.clear();
    det_px_sizes.clear();
    det_valid = false;
    det_submitted = submitted;
    det_vox_cap = g.vox_cap;
    det_g = g;
  }
  DevBuf<vdp::DetDesc> d_detdesc;  // staging of a query, grown on use
  DevBuf<vdp::DetBox> d_detbox;
  DevBuf<float4> d_detpts;
  DevBuf<uint32_t> d_detidx;
  DevBuf<vpx::PixDesc> d_pxdesc;  // ... and of a vofod_detection_pixels query
  DevBuf<vpx::PixSize> d_pxsize;
  DevBuf<vpx::PixFound> d_pxfound;
  DevBuf<uint32_t> d_pxkey, d_pxrank, d_pxidx, d_pxmember;
  DevBuf<float> d_pxxyz;
  // state of a submitted, not yet collected batch (vofod_batch_submit / vofod_batch_collect)
  bool pending = false;
  uint32_t job_n = 0;
  GridParams job_g{};
  std::vector<float> job_tfs;
  DevEvent ev_done;
  DevEvent ev_packed;   // the read-back slots are complete on the chain's stream
  DevEvent ev_key;      // staged pipeline: the batch's streaming kernels (brick codes) are through
  DevEvent ev_h2d;      // the host-resident columns of a submitted batch have crossed the link (vofod_batch_submit returns behind it)

  // Grow to at least these capacities.  What was there is released first (two 6.4 GB workspaces must never coexist); a failure
  // leaves an empty workspace.
  hipError_t ensure(uint32_t F_, uint32_t pt_cap_, uint32_t vox_cap_, uint32_t words_cap_, uint32_t bricks_cap_ = 0)
  {
    if (F_ <= F && pt_cap_ <= pt_cap && vox_cap_ <= vox_cap && words_cap_ <= words_cap && bricks_cap_ <= bricks_cap)
      return hipSuccess;
    F_ = std::max(F_, F);
    pt_cap_ = std::max(pt_cap_, pt_cap);
    vox_cap_ = std::max(vox_cap_, vox_cap);
    words_cap_ = std::max(words_cap_, words_cap);
    bricks_cap_ = std::max(bricks_cap_, bricks_cap);
    *this = Workspace();
    const hipError_t e = allocate(F_, pt_cap_, vox_cap_, words_cap_, bricks_cap_);
    if (e != hipSuccess)
      *this = Workspace();
    return e;
  }

private:
  // every allocation of an empty workspace; the capacities are set last
  hipError_t allocate(const uint32_t F_, const uint32_t pt_cap_, const uint32_t vox_cap_, const uint32_t words_cap_, const uint32_t bricks_cap_)
  {
    const uint32_t nblk_cap_ = (words_cap_ + SCAN_WPB - 1) / SCAN_WPB + 1;
    const size_t FV = static_cast<size_t>(F_) * vox_cap_;
    const size_t FB = F_ * std::max<size_t>(bricks_cap_, 1);
    const size_t FW = F_ * (static_cast<size_t>(words_cap_) + 2);
    HIP_TRY(alloc_view(ba_bricks, ba.bricks, FB));
    HIP_TRY(hipMemset(ba.bricks, 0, sizeof(unsigned long long) * FB));
    HIP_TRY(d_bconn.alloc(FB));
    HIP_TRY(alloc_view(ba_bparent, ba.bparent, FB));
    HIP_TRY(alloc_view(ba_bmin, ba.bmin, FB));
    HIP_TRY(alloc_view(ba_bcmin, ba.bcmin, FB));
    HIP_TRY(hipMemset(ba.bmin, 0xff, sizeof(uint32_t) * FB));
    HIP_TRY(hipMemset(ba.bcmin, 0xff, sizeof(uint32_t) * FB));
    HIP_TRY(alloc_view(ba_blist, ba.blist, FV));
    HIP_TRY(d_args.alloc(F_));
    HIP_TRY(d_hdrs.alloc(F_));
    HIP_TRY(d_bitmaps.alloc(FW));
    HIP_TRY(d_wprefix.alloc(FW));
    HIP_TRY(d_blocksums.alloc(static_cast<size_t>(F_) * nblk_cap_));
    HIP_TRY(alloc_view(va_pts, va.pts, FV));
    HIP_TRY(alloc_view(va_key, va.key, FV));
    HIP_TRY(alloc_view(va_parent, va.parent, FV));
    HIP_TRY(alloc_view(va_csize, va.csize, FV));
    HIP_TRY(alloc_view(va_cbox, va.cbox, 6 * FV));
    HIP_TRY(alloc_view(va_cclose, va.cclose, FV));
    HIP_TRY(alloc_view(va_bb, va.bb, FV));
    HIP_TRY(d_labels.alloc(FV));
    HIP_TRY(d_table.alloc(FV));
    HIP_TRY(d_cand.alloc(FV));
    // (the frame kernel's code list: every wave of a frame's workgroup appends to a segment of its own - whole rounds of the input pass)
    fs.keys_cap = (pt_cap_ + IN_SEG_ALIGN - 1u) / IN_SEG_ALIGN * IN_SEG_ALIGN;
    HIP_TRY(d_keys.alloc(static_cast<size_t>(F_) * fs.keys_cap));
    HIP_TRY(alloc_view(sa_extras, sa.extras, static_cast<size_t>(F_) * pt_cap_));
    HIP_TRY(alloc_view(sa_counts, sa.counts, 2 * static_cast<size_t>(F_)));
    sa.keys = d_keys;
    HIP_TRY(d_stage.alloc(5 * static_cast<size_t>(F_) * pt_cap_));
    HIP_TRY(d_rjobs.alloc(F_));
    HIP_TRY(h_rjobs.alloc(F_));
    HIP_TRY(d_pjobs.alloc(F_));
    HIP_TRY(h_pjobs.alloc(F_));
    HIP_TRY(d_packed.alloc(F_));
    HIP_TRY(d_tailc.alloc(vtd::TP_MAXC * static_cast<size_t>(F_)));
    HIP_TRY(d_dets.alloc(F_));
    HIP_TRY(d_job_be.alloc(2 * static_cast<size_t>(F_)));
    HIP_TRY(d_members_big.alloc(vox_cap_));
    HIP_TRY(alloc_view(fs_rowT, fs.rowT, 4 * FR_ROWS_MAX * static_cast<size_t>(F_)));
    HIP_TRY(alloc_view(fs_rowQ, fs.rowQ, 4 * FR_ROWS_MAX * static_cast<size_t>(F_)));
    HIP_TRY(alloc_view(fs_bmin, fs.bmin, LB_MAX * static_cast<size_t>(F_)));
    HIP_TRY(alloc_view(fs_nodeA, fs.nodeA, 4 * LB_MAX * static_cast<size_t>(F_)));
    HIP_TRY(alloc_view(fs_bbsave, fs.bbsave, FR_BB64 * static_cast<size_t>(F_)));
    HIP_TRY(alloc_view(fs_frag, fs.frag, static_cast<size_t>(F_) * std::max<uint32_t>(pt_cap_, 1)));
    HIP_TRY(h_packed.alloc(F_));
    HIP_TRY(h_dets.alloc(F_, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h_dets, 0, sizeof(vtd::FrameDets) * F_);
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_dets_dev), h_dets, 0));
    HIP_TRY(h_args.assign(F_, FrameArgs{}));
    HIP_TRY(ev_done.create(hipEventCreateWithFlags, hipEventDisableTiming));
    HIP_TRY(ev_packed.create(hipEventCreateWithFlags, hipEventDisableTiming));
    HIP_TRY(ev_h2d.create(hipEventCreateWithFlags, hipEventDisableTiming));
    HIP_TRY(ev_key.create(hipEventCreateWithFlags, hipEventDisableTiming));
    // the memsets above run on the null stream, the kernels on non-blocking streams: wait for the fills to land
    HIP_TRY(hipDeviceSynchronize());
    F = F_;
    pt_cap = pt_cap_;
    vox_cap = vox_cap_;
    words_cap = words_cap_;
    bricks_cap = bricks_cap_;
    nblk_cap = nblk_cap_;
    return hipSuccess;
  }
};

struct ExploreBufs
{
  DevBuf<unsigned long long> d_overlay;
  DevBuf<uint32_t> d_stack, d_explored, d_touched, d_ovl_list, d_ovl_count, d_job_begin;
  DevBuf<uint32_t> d_visited;  // per frame slot: visited bits of the running flood fill (all-zero between fills)
  DevBuf<vc::ExploreJob> d_jobs;
  DevBuf<vc::ExploreResult> d_results;
  DevBuf<int> d_members;  // three words per member
  // frame slots of the per-frame buffers (d_visited is the last of them that ensure_explore allocates: it stands for all eight)
  uint32_t F() const { return static_cast<uint32_t>(d_visited.n / vc::EX_WORDS); }
};

struct HostCluster
{
  ClusterRec rec;
  int cclass = VOFOD_CLASS_NONE;
  vt::Gates gates;  // boxes and gates of a candidate cluster (not evaluated: obb_size NaN)
};

struct vofod_handle
{
  DevBuf<unsigned long long> d_prof_slab, d_prof_ccl;  // stamp buffers of the VOFOD_LDS_PROF diagnostics
  // A frame of a batch held more pure-far bricks than the close-first frame kernel takes (a cold map: nothing is "close"): the
  // batch ran again with the full clustering, and so do the following ones - until the map has gained background voxels
  // (nVoxelsOver well above the count at the overflow) or was reset.
  bool cf_off = false;
  uint64_t cf_off_bg = 0;
  bool bgcount_stale = false;  // k_finalize_far patched the nVoxelsOver counters on the device: n_bg_voxels is older than they are
  bool lds_ccl_off = false;  // a frame of the batch just collected overflowed the LDS kernels: the NEXT launch (its re-run) takes the global-memory kernels, then the flag drops
  std::mutex mtx;
  vofod_static_params sp{};
  vofod_dyn_params dp{};
  std::string err;
  Prof prof;
  int device = 0;
  hipStream_t stream = nullptr;  // where every KLAUNCH goes: borrowed (chain_stream[0] outside a StreamScope, which points it elsewhere for its length)
  DevStream stream_tail;  // tail (k_explore) of collected async batches
  DevStream stream_key;   // staged pipeline: streaming kernels of all submitted batches, lowest priority
  // staged pipeline: the frame kernels of the submitted batches take the frame streams in turn.  A stream runs its kernels one
  // after the other, and a frame kernel lasts from its first workgroup's start to its LAST workgroup's end - about two workgroup
  // durations once the starts are staggered: with two streams a CU whose workgroup ended early had nothing to run until the other
  // stream's previous kernel had drained completely (round 5: ~15 % of the CU time; the stamps of tools/phase_table.sh show it).
  static constexpr int MAX_FRAME_STREAMS = 8;
  DevStream stream_frames[MAX_FRAME_STREAMS];
  int n_frame_streams = 0;
  hipStream_t stream_frame = nullptr;  // == stream_frames[0] (borrowed)
  int frame_toggle = 0;
  // Batches in flight.  Slots are allocated on first use.  Large batches gain nothing beyond four; small ones (whole chains side
  // by side, tails included) gain up to eight PROVIDED their streams do not share hardware queues - the runtime deals a process's
  // streams onto four by default (GPU_MAX_HW_QUEUES): 142 k frames/s at 32 frames with four queues, 204-289 k with 16.
  static constexpr int MAX_INFLIGHT = 8;
  DevStream chain_stream[MAX_INFLIGHT];  // [0]: the handle's own stream; in-flight batches run their chains on separate streams and overlap on the device
  Workspace wsx[MAX_INFLIGHT - 1];              // workspaces of tickets 1..7 (ticket 0 uses ws)
  Workspace* slot(int t) { return t == 0 ? &ws : &wsx[t - 1]; }
  ExploreBufs explore_slot[MAX_INFLIGHT];  // flood-fill buffers of small submitted batches: their tails run on the tickets' own streams

  float exclude_center[3], oparea_center[3];
  uint64_t background_min_sufficient_pts = 0;

  MapGeom mg{};
  vt::Geom hg{};
  DevBuf<float> d_map, d_flags, d_ray;
  DevBuf<float> d_shift_spare;  // vofod_map_shift: destination of the out-of-place shift, swapped with the map it received (allocated on the first shift)
  vmr::Workspace render;  // vofod_map_render: pose table and host-output staging, grown to the largest n_views * w * h seen
  vmm::Workspace match;  // vofod_map_match: the live list, pose table and counts; and the occupancy image of a call's threshold (vofod_map_distance's too)
  vmd::Workspace dist;  // vofod_map_distance: the passes' two fields; vofod_map_match_field: a host field's staging, the sums
  vss::ScanStage qstage;  // the query calls' host-resident scans (scan_stage.h): the block they are gathered into
  DevBuf<uint32_t> d_qstage;  // ... and where it stands on the device
  vws::Store world;  // vofod_world_enable: the voxel map is a window onto it (world_store.h); indexed by world index, so no shift moves it
  vwy::State wsync;  // snapshots / deltas of the store (world_sync.h, world_sync_host.h): shadow pool, scratch and the two chains
  DevBuf<unsigned long long> d_mapbits;
  DevBuf<unsigned long long> d_mapclose;  // d_mapbits dilated by hasCloseTo's stencil (k_dilate), valid while gens match
  uint64_t mapbits_gen = 0, mapclose_gen = ~0ull;
  float mapclose_dist = -1.0f;
  DevBuf<unsigned long long> d_counter;  // scratch words
  DevBuf<unsigned long long> d_bgcount;
  PinBuf<unsigned long long> h_bgcount;  // MB_SLOTS partial nVoxelsOver counters (64 B apart); host pinned copy
  bool bgcount_fresh = false;
  DevEvent ev_stagger;  // the streaming kernels of the batch submitted last have finished
  bool ev_stagger_set = false;
  DevEvent ev_explore;  // the shared flood-fill buffers are free again (device tails of batches on different streams take turns)
  DevEvent ev_bgcount;  // recorded behind the device-to-host copy of the background count: waited for before the count is consumed
  PinBuf<unsigned long long> h_counter;
  bool mapbits_valid = false;
  float mapbits_thr = 0;
  uint64_t n_bg_voxels = 0;

  DevBuf<float> d_lut_dirs, d_lut_offs;
  DevBuf<uint8_t> d_mask;
  DevBuf<uint32_t> d_col_shift;  // vofod_set_column_shift: one shift per row, reduced to [0, width); zeros until set
  bool raycast_motion = false;   // vofod_set_raycast_motion: the raycast role casts a scan with col_tfs ray by ray from the columns' poses (k_raycast_motion)
  bool point_motion = false;     // vofod_set_point_motion: the per-scan entry points accept col_tfs on a point scan (k_point_deskew)
  bool raycast_exact = false;    // vofod_set_raycast_exact: the next raycast pass accumulates fixed-point units (k_raycast_exact)
  bool ray_pass_exact = false;   // the pass between begin and finish holds units in d_ray (the representation belongs to the pass: begin records it)
  int32_t ray_log2_units = -1;   // S and QMAX of EXACT RAYCAST ACCUMULATION, fixed at create (-1: no S fits, the switch is refused)
  uint32_t ray_qmax = 0;

  Workspace ws, aux, sepws;
  ExploreBufs explore;
  std::unique_ptr<vt::Pool> pool;
  struct ClusterTables
  {
    bool valid = false;
    float leaf[3] = {0, 0, 0}, tol = 0, cmax = 0;
    ClusterParams cp{};
    int n_rows = 0;
    DevBuf<StencilRow> d_rows;
    bool brick_ok = false;
    BrickParams bp{};
    DevBuf<BrickOff> d_boffs;
    DevBuf<unsigned long long> d_sure, d_amb;
    DevBuf<int8_t> d_pair;  // [64*64] stencil index of offset(o2) - offset(o1), -1 when outside the forward stencil
    DevBuf<LbTables> d_lbtab;  // row / octant tables of the LDS clustering (k_frame_lds)
    bool lds_ok = false;
  } ctab[2];
  int ctab_next = 0;
  struct CloseTables
  {
    bool valid = false;
    float max_dist = 0;
    int n_rows = 0;
  } closetab;
  bool ray_dirty = false;
  DevBuf<StencilRow> d_rows;
  DevBuf<CloseRow> d_crows;
  DevBuf<float> d_boxstage;
  DevBuf<uint64_t> d_idxstage;

  bool background_pts_sufficient = false, sure_background_sufficient = false;
  int detection_its = 0;
  uint32_t last_detection_id = 0;
  bool raycast_pending = false;
  int raycast_start_its = 0;
  vr::SepState sep;  // a view, like Workspace::ba: its buffers are owned by sep_own (words_cap / pts_cap are not used: the owners know)
  struct SepBufs
  {
    DevBuf<unsigned long long> d_tbits;
    DevBuf<uint32_t> d_tpop, d_tprefix, d_bsum, d_sure, d_sure_pre, d_vcnt, d_first, d_nsure, d_small;
    DevBuf<float> d_px, d_py, d_pz, d_pi;
    DevBuf<int> d_offsets;
    PinBuf<uint32_t> h_small;
  } sep_own;
  MapSyncState msync;  // snapshots / deltas of the maps (mapsync.h, mapsync_host.h)
  bool sep_pending = false;
  int sep_start_its = 0;
};

#include "frame_prof.h"

namespace
{

// ------------------------------------------------------------------ tables built on the host

// Decides, for a lattice offset (di,dj,dk), whether two voxel centres that far apart are within the tolerance:
// 1 certainly (nominal squared distance below tol^2 by more than the worst float evaluation error),
// 0 certainly not, 2 on the boundary -> the kernels evaluate FLANN's float expression on the actual centres.
struct EdgeClassifier
{
  double leaf[3], r2, delta;
  float r2f;
  EdgeClassifier(const float leaf_[3], float tol, float cmax)
  {
    r2f = tol * tol;
    r2 = r2f;
    for (int a = 0; a < 3; a++)
      leaf[a] = leaf_[a];
    delta = 2.0 * ulp32(cmax);  // error bound of one centre coordinate (two roundings)
  }
  int operator()(int di, int dj, int dk) const
  {
    const double ex = std::abs(di) * leaf[0], ey = std::abs(dj) * leaf[1], ez = std::abs(dk) * leaf[2];
    const double D = ex * ex + ey * ey + ez * ez;
    const double eps = 2.0 * delta + 3.0 * ulp32(static_cast<float>(std::max({ex, ey, ez, 1e-30})));
    const double E = 2.0 * eps * (ex + ey + ez) + 3.0 * eps * eps + 8.0 * D * 1.2e-7;
    if (D + E < r2)
      return 1;
    if (D - E >= r2)
      return 0;
    return 2;
  }
};

// Half stencil of the Euclidean predicate d2 < tol^2 on a lattice of pitch `leaf` (voxel-level kernel).
int build_cluster_stencil(const float leaf[3], float tol, float cmax, std::vector<StencilRow>& rows, ClusterParams& cp)
{
  rows.clear();
  int R[3];
  for (int a = 0; a < 3; a++)
  {
    R[a] = static_cast<int>(std::ceil(static_cast<double>(tol) / leaf[a])) + 1;
    if (R[a] > MAX_R)
      return VOFOD_ERR_INVALID_ARG;
  }
  const EdgeClassifier classify(leaf, tol, cmax);
  cp.row_gap = -1;
  for (int dk = 0; dk <= R[2]; dk++)
    for (int dj = (dk == 0 ? 0 : -R[1]); dj <= R[1]; dj++)
    {
      StencilRow row{};
      row.dj = static_cast<int16_t>(dj);
      row.dk = static_cast<int16_t>(dk);
      row.r_sure = -1;
      row.r_max = -1;
      row.amb = 0;
      bool sure_run = true;
      for (int di = 0; di <= R[0]; di++)
      {
        const int c = classify(di, dj, dk);
        if (c == 1 && sure_run)
          row.r_sure = static_cast<int16_t>(di);
        else
          sure_run = false;
        if (c == 1 && !sure_run)
          row.amb |= 1u << di;  // cannot happen for a monotone predicate; evaluate in float to stay safe
        if (c == 2)
          row.amb |= 1u << di;
        if (c != 0)
          row.r_max = static_cast<int16_t>(di);
      }
      if (row.r_max < 0)
        continue;
      if (dj == 0 && dk == 0)
      {
        if (row.r_max < 1)
          continue;
        cp.row_gap = std::max<int>(row.r_sure, 0);
      }
      rows.push_back(row);
    }
  if (rows.size() > MAX_STENCIL_ROWS)
    return VOFOD_ERR_INVALID_ARG;
  cp.n_rows = static_cast<int>(rows.size());
  cp.r2 = classify.r2f;
  if (cp.row_gap < 0)
    cp.row_gap = 0;
  return VOFOD_OK;
}

// Brick-level tables (kernels_brick.h).  Returns false when a 4x4x4 brick is not a clique for this tolerance.
bool build_brick_tables(const float leaf[3], float tol, float cmax, std::vector<BrickOff>& offs, std::vector<unsigned long long>& sure, std::vector<unsigned long long>& amb)
{
  offs.clear();
  sure.clear();
  amb.clear();
  const EdgeClassifier classify(leaf, tol, cmax);
  if (classify(3, 3, 3) != 1)
    return false;
  int Rb[3];
  for (int a = 0; a < 3; a++)
  {
    const int r_max = static_cast<int>(std::ceil(static_cast<double>(tol) / leaf[a])) + 1;
    Rb[a] = (r_max + 3 + 3) / 4;
  }
  for (int bz = 0; bz <= Rb[2]; bz++)
    for (int by = (bz == 0 ? 0 : -Rb[1]); by <= Rb[1]; by++)
      for (int bx = ((bz == 0 && by == 0) ? 1 : -Rb[0]); bx <= Rb[0]; bx++)
      {
        unsigned long long ms[64], ma[64];
        bool any = false, any_amb = false;
        for (int p = 0; p < 64; p++)
        {
          ms[p] = ma[p] = 0;
          const int px = p & 3, py = (p >> 2) & 3, pz = p >> 4;
          for (int q = 0; q < 64; q++)
          {
            const int qx = q & 3, qy = (q >> 2) & 3, qz = q >> 4;
            const int c = classify(4 * bx + qx - px, 4 * by + qy - py, 4 * bz + qz - pz);
            if (c == 1)
              ms[p] |= 1ull << q;
            else if (c == 2)
              ma[p] |= 1ull << q;
          }
          any |= (ms[p] | ma[p]) != 0;
          any_amb |= ma[p] != 0;
        }
        if (!any)
          continue;
        BrickOff bo{};
        bo.dx = static_cast<int8_t>(bx);
        bo.dy = static_cast<int8_t>(by);
        bo.dz = static_cast<int8_t>(bz);
        bo.has_amb = static_cast<uint8_t>(any_amb);
        for (int p = 0; p < 64; p++)
        {
          if (ms[p] | ma[p])
            bo.ua |= 1ull << p;
          bo.ub |= ms[p] | ma[p];
        }
        offs.push_back(bo);
        sure.insert(sure.end(), ms, ms + 64);
        amb.insert(amb.end(), ma, ma + 64);
      }
  return true;
}

// Tables of the LDS clustering (k_frame_lds) derived from the brick stencil: the offsets grouped into (dy,dz) rows, and per offset two
// 8x8 bit matrices over 2x2x2 octants: sure8 (every voxel pair of the two octants is certainly within the tolerance)
// and maybe8 (some pair is, certainly or on the boundary).
bool build_lds_tables(const EdgeClassifier& classify, const std::vector<BrickOff>& offs, const std::vector<unsigned long long>& sure, const std::vector<unsigned long long>& amb,
                      LbTables& t)
{
  std::memset(&t, 0, sizeof(t));
  // ball tables: every relative voxel offset the predicate can accept must lie within LB_RV per axis
  for (int c = LB_RV + 1; c <= 4 * 4 + 3; c++)
    if (classify(c, 0, 0) != 0 || classify(0, c, 0) != 0 || classify(0, 0, c) != 0)
      return false;
  for (int dz = -LB_RV; dz <= LB_RV; dz++)
    for (int dy = -LB_RV; dy <= LB_RV; dy++)
      for (int dx = -LB_RV; dx <= LB_RV; dx++)
      {
        const int c = classify(dx, dy, dz);
        if (c == 1)
          t.ball_sure[dz + LB_RV][dy + LB_RV] |= static_cast<uint16_t>(1u << (dx + LB_RV));
        else if (c == 2)
          t.ball_amb[dz + LB_RV][dy + LB_RV] |= static_cast<uint16_t>(1u << (dx + LB_RV));
      }
  if (offs.empty() || offs.size() > LB_MAX_OFF)
    return false;
  int R = 0;
  for (const auto& o : offs)
    R = std::max(R, std::abs(static_cast<int>(o.dx)));
  if (2 * R + 1 > LB_WIN)
    return false;
  t.R = R;
  for (size_t o = 0; o < offs.size(); o++)
  {
    int row = -1;
    for (int r = 0; r < t.n_rows; r++)
      if (t.rows[r].dy == offs[o].dy && t.rows[r].dz == offs[o].dz)
        row = r;
    if (row < 0)
    {
      if (t.n_rows == LB_MAX_ROWS)
        return false;
      row = t.n_rows++;
      t.rows[row].dy = offs[o].dy;
      t.rows[row].dz = offs[o].dz;
      for (auto& x : t.rows[row].o)
        x = -1;
    }
    if (std::abs(static_cast<int>(offs[o].dx)) <= 1 && std::abs(static_cast<int>(offs[o].dy)) <= 1 && std::abs(static_cast<int>(offs[o].dz)) <= 1)
      t.near_mask |= 1ull << o;
    if (std::abs(static_cast<int>(offs[o].dx)) + std::abs(static_cast<int>(offs[o].dy)) + std::abs(static_cast<int>(offs[o].dz)) == 1)
      t.axis_mask |= 1ull << o;
    const int s = offs[o].dx + R;
    t.rows[row].valid |= static_cast<uint8_t>(1u << s);
    t.rows[row].o[s] = static_cast<int8_t>(o);
    auto oct = [](int p) { return ((p & 3) >> 1) | ((((p >> 2) & 3) >> 1) << 1) | (((p >> 4) >> 1) << 2); };
    unsigned long long all = ~0ull, any = 0ull;
    bool seen[64] = {};
    for (int p = 0; p < 64; p++)
      for (int q = 0; q < 64; q++)
      {
        const int bit = oct(p) * 8 + oct(q);
        const bool is_sure = (sure[o * 64 + p] >> q) & 1ull, is_amb = (amb[o * 64 + p] >> q) & 1ull;
        if (!is_sure)
          all &= ~(1ull << bit);
        if (is_sure || is_amb)
          any |= 1ull << bit;
        seen[bit] = true;
      }
    (void)seen;
    t.oct[2 * o] = all;
    t.oct[2 * o + 1] = any;
  }
  return true;
}

// Rows of hasCloseTo's half-open cube (voxel_map.cpp:380-393), nearest rows first.
int build_close_rows(float max_dist, float vs_inv, std::vector<CloseRow>& rows)
{
  rows.clear();
  const float max_dist_idx = max_dist * vs_inv;
  const int d = static_cast<int>(std::ceil(max_dist_idx));
  if (d > MAX_R || d < 0)
    return VOFOD_ERR_INVALID_ARG;
  // int(sqrt(n2)) <= max_dist_idx  <=>  n2 <= n2max, found by direct evaluation of the reference's test
  for (int dy = -d; dy < d; dy++)
    for (int dz = -d; dz < d; dz++)
    {
      int lo = 1, hi = -1;
      for (int dx = -d; dx < d; dx++)
      {
        const int n2 = dx * dx + dy * dy + dz * dz;
        const int norm = static_cast<int>(std::sqrt(static_cast<double>(n2)));
        if (static_cast<float>(norm) <= max_dist_idx)
        {
          if (hi < lo)
            lo = dx;
          hi = dx;
        }
      }
      if (hi >= lo)
        rows.push_back(CloseRow{static_cast<int16_t>(dy), static_cast<int16_t>(dz), static_cast<int16_t>(lo), static_cast<int16_t>(hi)});
    }
  std::stable_sort(rows.begin(), rows.end(), [](const CloseRow& a, const CloseRow& b) { return a.dy * a.dy + a.dz * a.dz < b.dy * b.dy + b.dz * b.dz; });
  if (rows.size() > MAX_STENCIL_ROWS)
    return VOFOD_ERR_INVALID_ARG;
  return VOFOD_OK;
}

// the closed exclude box of the first crop, sensor frame (vofod_nodelet.cpp:626-629)
void exclude_box(const vofod_handle* h, float lo[3], float hi[3])
{
  for (int a = 0; a < 3; a++)
  {
    hi[a] = h->exclude_center[a] + h->sp.exclude_size[a] / 2;
    lo[a] = h->exclude_center[a] - h->sp.exclude_size[a] / 2;
  }
}

void fill_grid_params(vofod_handle* h, GridParams& g, const float leaf[3], bool align, const float align_center[3], const Workspace& ws)
{
  std::memset(&g, 0, sizeof(g));
  for (int a = 0; a < 3; a++)
  {
    g.leaf[a] = leaf[a];
    g.inv[a] = 1.0f / leaf[a];
    g.aco[a] = 0;
    if (align)
    {
      float aco = std::fmod(align_center[a] - leaf[a] / 2, leaf[a]);  // voxel_grid_weighted.cpp:86-97
      if (aco < 0)
        aco += leaf[a];
      g.aco[a] = aco;
    }
    g.op_max[a] = h->oparea_center[a] + h->sp.oparea_size[a] / 2;  // :645-648
    g.op_min[a] = h->oparea_center[a] - h->sp.oparea_size[a] / 2;
  }
  exclude_box(h, g.ex_min, g.ex_max);
  g.align = align;
  g.words_cap = ws.words_cap;
  g.vox_cap = ws.vox_cap;
  g.n_frames = 1;
  g.sparse_prefix = 0;
}

int ensure_boxstage(vofod_handle* h, size_t n)
{
  if (n > h->d_boxstage.n)
    HIPCHK(h->d_boxstage.alloc(std::max<size_t>(n, 1u << 20)));
  return VOFOD_OK;
}

// read the map cells [lo, lo+n) clipped to the map into a host box
int read_box(vofod_handle* h, const float* d_map, int lo[3], int hi[3], vt::Box& box)
{
  for (int a = 0; a < 3; a++)
  {
    lo[a] = std::max(lo[a], 0);
    hi[a] = std::min(hi[a], h->hg.s[a] - 1);
    box.lo[a] = lo[a];
    box.n[a] = std::max(hi[a] - lo[a] + 1, 0);
  }
  const size_t n = static_cast<size_t>(box.n[0]) * box.n[1] * box.n[2];
  box.v.resize(n);
  if (n == 0)
    return VOFOD_OK;
  VCHK(ensure_boxstage(h, n));
  KLAUNCH(h, k_read_box, dim3((n + 255) / 256), dim3(256), d_map, h->mg, lo[0], lo[1], lo[2], box.n[0], box.n[1], box.n[2], h->d_boxstage);
  HIPCHK(hipMemcpyAsync(box.v.data(), h->d_boxstage, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VOFOD_OK;
}

int scatter_set(vofod_handle* h, float* d_map, const std::vector<uint64_t>& idx, float value)
{
  if (idx.empty())
    return VOFOD_OK;
  if (idx.size() > h->d_idxstage.n)
    HIPCHK(h->d_idxstage.alloc(std::max<size_t>(idx.size(), 1u << 16)));
  HIPCHK(hipMemcpyAsync(h->d_idxstage, idx.data(), idx.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  KLAUNCH(h, k_scatter_set, dim3((idx.size() + 255) / 256), dim3(256), d_map, h->d_idxstage, static_cast<uint32_t>(idx.size()), value);
  HIPCHK(hipStreamSynchronize(h->stream));
  return VOFOD_OK;
}

int fill_map(vofod_handle* h, float* p, float v)
{
  KLAUNCH(h, k_fill, dim3(2048), dim3(256), p, h->mg.n, v);
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// reset() vofod_nodelet.cpp:1610-1632
int do_reset(vofod_handle* h)
{
  VCHK(fill_map(h, h->d_map, h->sp.score_init));
  VCHK(fill_map(h, h->d_flags, 0.0f));
  VCHK(fill_map(h, h->d_ray, 0.0f));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->detection_its = 0;
  h->raycast_pending = false;
  h->ray_pass_exact = false;
  h->sep_pending = false;
  h->mapbits_valid = false;
  return VOFOD_OK;
}

// one host column of n 4-byte elements at `stride` into `dst` (device), gathered first where the stride is not 4
int stage_host_column(vofod_handle* h, void* dst, const void* src, size_t stride, size_t n)
{
  std::vector<float> tmp;
  if (stride != 4)
  {
    tmp.resize(n);
    vss::gather4(tmp.data(), src, stride, n);
    src = tmp.data();
  }
  HIPCHK(hipMemcpyAsync(dst, src, n * 4, hipMemcpyHostToDevice, h->stream));
  if (stride != 4)
    HIPCHK(hipStreamSynchronize(h->stream));  // tmp goes away
  return VOFOD_OK;
}

// stage the columns of one cloud into the workspace if they live on the host; fill FrameArgs
int stage_cloud(vofod_handle* h, Workspace& ws, uint32_t f, const void* x, const void* y, const void* z, const void* intensity, const void* range, size_t stride,
                size_t n, int memspace, uint32_t flags, const float* tf)
{
  FrameArgs& a = ws.h_args[f];
  std::memset(&a, 0, sizeof(a));
  a.n = static_cast<uint32_t>(n);
  a.flags = flags;
  if (tf)
    std::memcpy(a.tf, tf, sizeof(float) * 12);
  if (memspace == VOFOD_MEM_DEVICE)
  {
    a.x = static_cast<const char*>(x);
    a.y = static_cast<const char*>(y);
    a.z = static_cast<const char*>(z);
    a.intensity = static_cast<const char*>(intensity);
    a.stride = stride;
    return VOFOD_OK;
  }
  // An array of structs in host memory (stride > 4, the three coordinates inside one struct: pcl::PointCloud<ouster_ros::Point>,
  // 48 bytes per point, what the nodelet holds - include/vofod/point_types.h) crosses the link with ONE copy of the whole block;
  // the kernels then read the columns in place at the struct's stride (the frame kernel's strided input pass, k_bbox / k_setbits / k_count).  Round 3 gathered every column on the
  // host (three passes over the cloud and a synchronisation per column: ~1 ms per frame).  4 x the bytes of packed columns over
  // PCIe: the link's ceiling for this layout is ~8 k frames/s of OS1-128.
  // The kernels dereference floats in place ON THE DEVICE, where the copy starts at the lowest of the three members: only
  // structs whose stride and whose members' distances from that lowest member are multiples of 4 take this path (the host
  // addresses need not be aligned: x at +1 of a packed 20-byte struct with y at +5 and z at +9 is read in place), a struct of
  // odd stride or with members an odd distance apart is gathered below.  The staging block is sized by the FIRST frame of a batch (or by
  // vofod_reserve's caller, which passes through here with frame 0 too); a later frame of the same batch whose struct is
  // larger than the block's pitch allows is gathered as well - growing the block there would free it under the earlier frames'
  // copies and pointers.
  if (stride > 4 && stride % 4 == 0 && !intensity && !range && n > 0)
  {
    const char* lo = std::min({static_cast<const char*>(x), static_cast<const char*>(y), static_cast<const char*>(z)});
    const char* hi = std::max({static_cast<const char*>(x), static_cast<const char*>(y), static_cast<const char*>(z)});
    const bool aligned = (static_cast<const char*>(x) - lo) % 4 == 0 && (static_cast<const char*>(y) - lo) % 4 == 0 && (static_cast<const char*>(z) - lo) % 4 == 0;
    if (aligned && static_cast<size_t>(hi - lo) + 4 <= stride)
    {
      const size_t block = (n - 1) * stride + static_cast<size_t>(hi - lo) + 4;
      if (f == 0 && (block > ws.aos_pitch || !ws.d_stage_aos))
      {
        const size_t pitch = (ws.pt_cap * stride + 255) & ~static_cast<size_t>(255);
        HIPCHK(hipStreamSynchronize(h->stream));
        ws.aos_pitch = 0;
        HIPCHK(ws.d_stage_aos.alloc(pitch * ws.F));
        ws.aos_pitch = pitch;
      }
      if (ws.d_stage_aos && block <= ws.aos_pitch)
      {
        char* dst = ws.d_stage_aos + static_cast<size_t>(f) * ws.aos_pitch;
        HIPCHK(hipMemcpyAsync(dst, lo, block, hipMemcpyHostToDevice, h->stream));
        a.x = dst + (static_cast<const char*>(x) - lo);
        a.y = dst + (static_cast<const char*>(y) - lo);
        a.z = dst + (static_cast<const char*>(z) - lo);
        a.intensity = nullptr;
        a.stride = stride;
        return VOFOD_OK;
      }
    }
  }
  float* base = ws.d_stage + static_cast<size_t>(f) * ws.pt_cap * 5;
  const void* cols[5] = {x, y, z, intensity, range};
  for (int c = 0; c < 5; c++)
    if (cols[c])
      VCHK(stage_host_column(h, base + static_cast<size_t>(c) * ws.pt_cap, cols[c], stride, n));
  a.x = reinterpret_cast<const char*>(base);
  a.y = reinterpret_cast<const char*>(base + ws.pt_cap);
  a.z = reinterpret_cast<const char*>(base + 2 * static_cast<size_t>(ws.pt_cap));
  a.intensity = intensity ? reinterpret_cast<const char*>(base + 3 * static_cast<size_t>(ws.pt_cap)) : nullptr;
  a.stride = 4;
  return VOFOD_OK;
}

// 1-D grid of a per-frame kernel: n_frames x gx blocks (see frame_block in kernels_voxelize.h)
inline dim3 fgrid(const GridParams& g, uint32_t gx) { return dim3(g.n_frames * gx); }
inline uint32_t emit_split(uint32_t n_frames) { return n_frames <= 16 ? EMIT_SPLIT : 1u; }

// Reference lattice of the frame kernel's input pass (kernels_frame.h): what voxel_grid_weighted.cpp:72-106 yields for a cloud
// whose minimum is the operation area's corner, and the band around cell boundaries inside which the frame's own offset may
// round a point into the neighbouring cell.  Bound: |q - O| <= 2c (c = largest |coordinate|), the subtraction and the product
// each round by 2^-24 relative -> 2 * 2c * inv * 2^-23 cells per offset; the two offsets differ from whole cells by their own
// roundings (2 * c * 2^-23 * inv) and by leaf * inv != 1 (<= 2^-22 per cell of distance).  eps is four times the sum.
RefLattice fill_ref_lattice(const GridParams& g)
{
  RefLattice rl{};
  float cmax = 0.0f, dmax = 0.0f, inv_max = 0.0f;
  for (int a = 0; a < 3; a++)
  {
    const int min_b = static_cast<int>(std::floor(g.op_min[a] * g.inv[a]));
    float offset = static_cast<float>(min_b) * g.leaf[a];
    if (g.align)
      offset = offset - g.aco[a];
    rl.off[a] = offset;
    rl.dims[a] = static_cast<int>(std::floor((g.op_max[a] - offset) * g.inv[a])) + 2;
    cmax = std::max(cmax, std::max(std::fabs(g.op_min[a]), std::fabs(g.op_max[a])) + g.leaf[a]);
    dmax = std::max(dmax, static_cast<float>(rl.dims[a]));
    inv_max = std::max(inv_max, g.inv[a]);
  }
  const float u = 1.1920929e-7f;  // 2^-23
  const float e1 = 2.0f * (2.0f * cmax) * inv_max * u, e2 = 2.0f * cmax * u * inv_max + dmax * 2.0f * u;
  rl.eps = 4.0f * (e1 + e2) + 1e-4f;
  // (eps < 0.05: a point is fragile when any of its three fractions lies within eps of a boundary - up to 1 - (1 - 2 eps)^3 = 27 %
  // of uniformly spread points; measured on OS1-16 scenes, whose ground sheet lies on a cell boundary: 45 % at eps 0.036 and 52 % at
  // eps 0.047, areas 3-4 km from the origin (tests/test_gpu_frame_inputs.py), 3 % on the default area.  The frame's side list holds
  // one entry per input point, so any share fits)
  // the frame kernel's bricks are bricks of this lattice: its brick bitmap has to fit LDS (LB_BITWORDS), its brick rows the
  // per-frame row tables, the brick coordinates the fields of a code (9 + 9 + 6 bits)
  for (int a = 0; a < 3; a++)
    rl.nb[a] = (rl.dims[a] + 3) / 4;
  const bool fits = rl.dims[0] > 0 && rl.dims[1] > 0 && rl.dims[2] > 0 && rl.nb[0] <= 512 && rl.nb[1] <= 512 && rl.nb[2] <= FR_MAX_NBZ &&
                    static_cast<long long>(rl.nb[0]) * rl.nb[1] * rl.nb[2] <= static_cast<long long>(LB_BITWORDS) * 32 && static_cast<uint32_t>(rl.nb[1]) * rl.nb[2] <= FR_ROWS_MAX;
  rl.on = rl.eps < 0.05f && fits;
  return rl;
}

// K3-K6 of the general voxeliser through the global occupancy bitmaps: bitmap (cleared first where `clear`) -> ranks -> weighted cloud
int launch_bitmap_chain(vofod_handle* h, Workspace& ws, const GridParams& g, uint32_t n, uint32_t max_pts, bool clear)
{
  const uint32_t gx = std::max(1u, std::min((max_pts + 255u) / 256u, 1024u));
  if (clear)
    HIPCHK(hipMemsetAsync(ws.d_bitmaps, 0, sizeof(unsigned long long) * ws.F * (static_cast<size_t>(ws.words_cap) + 2), h->stream));
  ws.bitmap_clean = false;  // set again by whoever runs the clearing pass
  KLAUNCH(h, k_setbits, fgrid(g, gx), dim3(256), ws.d_args, g, ws.d_hdrs, ws.d_bitmaps);
  KLAUNCH(h, k_scan_a, fgrid(g, ws.nblk_cap), dim3(256), g, ws.d_hdrs, ws.d_bitmaps, ws.d_blocksums, ws.nblk_cap);
  KLAUNCH(h, k_scan_b, dim3(n), dim3(1024), g, ws.d_hdrs, ws.d_blocksums, ws.nblk_cap);
  KLAUNCH(h, k_emit, fgrid(g, ws.nblk_cap * emit_split(n)), dim3(256), g, ws.d_hdrs, ws.d_bitmaps, ws.d_blocksums, ws.nblk_cap, ws.d_wprefix, ws.va, 0u, emit_split(n));
  KLAUNCH(h, k_count, fgrid(g, gx), dim3(256), ws.d_args, g, ws.d_hdrs, ws.d_bitmaps, ws.d_wprefix, ws.va);
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// the frames' arguments and fresh headers: all the frame kernel (kernels_frame.h), which reads the input itself, needs ahead of it
int launch_frame_args(vofod_handle* h, Workspace& ws, GridParams& g, uint32_t n)
{
  g.n_frames = n;
  HIPCHK(hipMemcpyAsync(ws.d_args, ws.h_args.data(), sizeof(FrameArgs) * n, hipMemcpyHostToDevice, h->stream));
  KLAUNCH(h, k_init_hdr, dim3(n), dim3(64), ws.d_hdrs);
  return VOFOD_OK;
}

// K1-K2 over frames [0,n): bbox -> lattice.  (A cloud voxelisation inspects the lattice's size before the bitmap is touched.)
int launch_lattice(vofod_handle* h, Workspace& ws, GridParams& g, uint32_t n, uint32_t max_pts)
{
  VCHK(launch_frame_args(h, ws, g, n));
  const uint32_t gb = std::max(1u, std::min((max_pts + 2047u) / 2048u, 1024u));  // 8 points per thread: few header atomics
  KLAUNCH(h, k_bbox, fgrid(g, gb), dim3(256), ws.d_args, g, ws.d_hdrs);
  KLAUNCH(h, k_grid, dim3(n), dim3(64), g, ws.d_hdrs);
  return VOFOD_OK;
}

// K1-K6 over frames [0,n) as planned: the general voxelisers - or, for the frame kernel (launched by launch_frame_kernel: input
// pass, voxel records and clustering on one LDS image; rounds 2-4 had a streaming kernel in front, k_key1, which is gone), only
// what it needs ahead of it
int launch_voxelize(vofod_handle* h, Workspace& ws, const vplan::ChainPlan& plan, GridParams& g, uint32_t n, uint32_t max_pts)
{
  if (plan.frame())
  {
    VCHK(launch_frame_args(h, ws, g, n));
    if (!h->ev_stagger)
      HIPCHK(h->ev_stagger.create(hipEventCreateWithFlags, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->ev_stagger, h->stream));  // the next batch's chain may start now
    h->ev_stagger_set = true;
    HIPCHK(hipGetLastError());
    return VOFOD_OK;
  }
  VCHK(launch_lattice(h, ws, g, n, max_pts));
  if (plan.voxeliser == vplan::Voxeliser::Bitmap)
    return launch_bitmap_chain(h, ws, g, n, max_pts, plan.clear_bitmap);
  // the bitmap is built slab by slab in LDS (kernels_slab.h)
  if (plan.clear_bitmap)
    HIPCHK(hipMemsetAsync(ws.d_bitmaps, 0, sizeof(unsigned long long) * ws.F * (static_cast<size_t>(ws.words_cap) + 2), h->stream));
  HIPCHK(hipMemsetAsync(ws.sa.counts, 0, sizeof(uint32_t) * 2 * n, h->stream));
  const uint32_t gk = std::max(1u, (max_pts + KEY_THREADS * KEY_PPT - 1) / (KEY_THREADS * KEY_PPT));
  KLAUNCH(h, k_key, fgrid(g, gk), dim3(KEY_THREADS), ws.d_args, g, ws.d_hdrs, ws.sa, ws.pt_cap);
  ws.bitmap_clean = false;
  const bool slab_emit = plan.voxeliser == vplan::Voxeliser::SlabEmit;
  if (slab_emit)
  {
    // batches that fill the chip: one workgroup per frame walks the slabs in order and emits the voxel records itself
    unsigned long long* d_prof = nullptr;
    VCHK(slab_emit_prof_buffer(h, d_prof));
    KLAUNCH(h, k_slab_emit, dim3(n), dim3(SLAB_THREADS), g, ws.d_hdrs, ws.sa, ws.pt_cap, ws.d_bitmaps, ws.d_wprefix, ws.va, 1u, d_prof);
    if (d_prof)
      VCHK(print_slab_emit_prof(h, n));
  }
  else
  {
    KLAUNCH(h, k_slab, fgrid(g, plan.slab_groups), dim3(SLAB_THREADS), g, ws.d_hdrs, ws.sa, ws.pt_cap, ws.d_bitmaps, ws.d_blocksums, ws.nblk_cap);
    KLAUNCH(h, k_scan_b, dim3(n), dim3(1024), g, ws.d_hdrs, ws.d_blocksums, ws.nblk_cap);
    KLAUNCH(h, k_emit, fgrid(g, ws.nblk_cap * emit_split(n)), dim3(256), g, ws.d_hdrs, ws.d_bitmaps, ws.d_blocksums, ws.nblk_cap, ws.d_wprefix, ws.va, 1u, emit_split(n));
  }
  // after k_slab_emit only the extras beyond its LDS staging area are left (none on ordinary scans)
  KLAUNCH(h, k_count_extras, fgrid(g, slab_emit ? 4 : 24), dim3(256), g, ws.d_hdrs, ws.sa, ws.pt_cap, ws.d_bitmaps, ws.d_wprefix, ws.va);
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// Stencil / brick tables of a clustering problem, cached per (leaf, tolerance, coordinate bound).
int cluster_tables(vofod_handle* h, const GridParams& g, float tol, float cmax, vofod_handle::ClusterTables** out)
{
  vofod_handle::ClusterTables* ct = nullptr;
  for (auto& c : h->ctab)
    if (c.valid && c.tol == tol && c.cmax == cmax && c.leaf[0] == g.leaf[0] && c.leaf[1] == g.leaf[1] && c.leaf[2] == g.leaf[2])
      ct = &c;
  if (!ct)
  {
    ct = &h->ctab[h->ctab_next];
    h->ctab_next ^= 1;
    // the slot's device tables are rewritten in place below: kernels of batches in flight (non-blocking streams) may still
    // read them.  A new tolerance is a rare event; the device is simply drained first.
    HIPCHK(hipDeviceSynchronize());
    ct->valid = false;
    ct->lds_ok = false;
    std::vector<StencilRow> rows;
    const int r = build_cluster_stencil(g.leaf, tol, cmax, rows, ct->cp);
    if (r != VOFOD_OK)
    {
      h->err = "cluster tolerance / leaf ratio exceeds the 63-bit neighbour window";
      return r;
    }
    std::vector<BrickOff> offs;
    std::vector<unsigned long long> sure, amb;
    ct->brick_ok = build_brick_tables(g.leaf, tol, cmax, offs, sure, amb);
    ct->d_boffs.reset();
    ct->d_sure.reset();
    ct->d_amb.reset();
    HIPCHK(ct->d_rows.alloc(rows.size()));
    HIPCHK(hipMemcpy(ct->d_rows, rows.data(), sizeof(StencilRow) * rows.size(), hipMemcpyHostToDevice));
    ct->n_rows = static_cast<int>(rows.size());
    if (ct->brick_ok)
    {
      HIPCHK(ct->d_boffs.alloc(offs.size()));
      HIPCHK(ct->d_sure.alloc(sure.size()));
      HIPCHK(ct->d_amb.alloc(amb.size()));
      HIPCHK(hipMemcpy(ct->d_boffs, offs.data(), sizeof(BrickOff) * offs.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(ct->d_sure, sure.data(), sizeof(unsigned long long) * sure.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(ct->d_amb, amb.data(), sizeof(unsigned long long) * amb.size(), hipMemcpyHostToDevice));
      ct->bp.n_off = static_cast<int>(offs.size());
      ct->bp.r2 = ct->cp.r2;
      ct->d_pair.reset();
      if (offs.size() <= 64)
      {
        std::vector<int8_t> pair(64 * 64, -1);
        for (size_t o1 = 0; o1 < offs.size(); o1++)
          for (size_t o2 = 0; o2 < offs.size(); o2++)
          {
            const int dx = offs[o2].dx - offs[o1].dx, dy = offs[o2].dy - offs[o1].dy, dz = offs[o2].dz - offs[o1].dz;
            for (size_t o3 = 0; o3 < offs.size(); o3++)
              if (offs[o3].dx == dx && offs[o3].dy == dy && offs[o3].dz == dz)
                pair[o1 * 64 + o2] = static_cast<int8_t>(o3);
          }
        HIPCHK(ct->d_pair.alloc(pair.size()));
        HIPCHK(hipMemcpy(ct->d_pair, pair.data(), pair.size(), hipMemcpyHostToDevice));
      }
      LbTables lt;
      ct->lds_ok = build_lds_tables(EdgeClassifier(g.leaf, tol, cmax), offs, sure, amb, lt);
      if (ct->lds_ok)
      {
        HIPCHK(ct->d_lbtab.reserve(1));
        HIPCHK(hipMemcpy(ct->d_lbtab, &lt, sizeof(LbTables), hipMemcpyHostToDevice));
      }
    }
    ct->tol = tol;
    ct->cmax = cmax;
    for (int a = 0; a < 3; a++)
      ct->leaf[a] = g.leaf[a];
    ct->valid = true;
  }
  *out = ct;
  return VOFOD_OK;
}

// What plan_chain (chain_plan.h) takes from the handle, a workspace and the cached cluster tables.  The call, the reference
// lattice, the layout of the staged inputs and `patchable` are the caller's to add.
vplan::PlanInputs plan_inputs(const vofod_handle* h, const Workspace& ws, const vofod_handle::ClusterTables* ct, const vplan::Switches& sw)
{
  vplan::PlanInputs in;
  in.sw = sw;
  in.vox_cap = ws.vox_cap;
  in.words_cap = ws.words_cap;
  in.bricks_cap = ws.bricks_cap;
  in.bitmap_clean = ws.bitmap_clean;
  in.brick_ok = ct->brick_ok;
  in.lds_ok = ct->lds_ok;
  in.n_off = ct->bp.n_off;
  in.pair_table = ct->d_pair.p != nullptr;
  in.n_rows = ct->n_rows;
  in.cf_off = h->cf_off;
  in.lds_ccl_off = h->lds_ccl_off;
  in.far_max = FAR_MAX;
  in.lb_max = LB_MAX;
  in.slab_words64 = SLAB_WORDS64;
  return in;
}

// The plan of a clustering on its own (vofod_cluster, the sepclusters role): one frame whose map-updating caller reads the
// labels of every cluster - the general kernels, brick or voxel level.
vplan::ChainPlan plan_cluster_only(const vofod_handle* h, const Workspace& ws, const vofod_handle::ClusterTables* ct)
{
  vplan::PlanInputs in = plan_inputs(h, ws, ct, vplan::read_switches());
  in.n = 1;
  in.dbg = true;
  return vplan::plan_chain(in);
}

// K1-K7 in one kernel: the brick-first frame kernel (kernels_frame.h) reads the input itself, builds the voxel records and
// clusters them on the same LDS image - the far voxels only where the plan says close first (read-only batches: only the far
// clusters are ever used, vofod_nodelet.cpp:946-963).  Four instantiations: close first or not, packed 16-byte column loads or
// strided ones; the profile names the algorithmic variant, k_frame_lds_far / k_frame_lds_full, and the strided input pass by
// the suffix _strided.
int launch_frame_kernel(vofod_handle* h, Workspace& ws, const vplan::ChainPlan& plan, const GridParams& g, uint32_t n, const vofod_handle::ClusterTables* ct, const RefLattice& ref_lattice,
                        const UpdateParams& up)
{
  BrickParams bp = ct->bp;
  bp.bricks_cap = ws.bricks_cap;
  unsigned long long* d_prof = nullptr;
  VCHK(frame_prof_slots(h, ws, d_prof));
  if (n + ws.prof_slot0 > FR_PROF_FRAMES)
    d_prof = nullptr;  // (a launch beyond the stamp buffer's frames leaves no stamps)
  const unsigned long long* mapclose = plan.use_dilated ? h->d_mapclose.p : nullptr;
  // Lean emission: a production batch reads the voxel records of the candidates' members only - voxels of pure-far bricks -, so
  // k_frame_lds_far writes, and counts the points of, those bricks' voxels alone.  The far-only debug
  // view reads the whole cloud and keeps the full emission; VOFOD_LEAN_EMIT=0 keeps it everywhere.  Bit 1 of the kernel's `lean`:
  // the rank tables are built for those bricks only, too (VOFOD_LEAN_RANKS=0: for every brick, as in a full emission).
  const bool far = plan.clusterer == vplan::Clusterer::FrameFar, packed = plan.in_packed;
  const auto kern = far ? (packed ? k_frame_lds_far_p : k_frame_lds_far) : (packed ? k_frame_lds_full_p : k_frame_lds_full);
  const char* label = far ? (packed ? "k_frame_lds_far" : "k_frame_lds_far_strided") : (packed ? "k_frame_lds_full" : "k_frame_lds_full_strided");
  KLAUNCH_AS(h, label, kern, dim3(n), dim3(FR_THREADS), g, bp, ct->d_lbtab, ws.d_hdrs, ws.sa, ws.pt_cap, ws.va, ws.d_labels, plan.lb_limit, reinterpret_cast<uint32_t*>(ws.d_table.p), ws.fs, h->mg, mapclose,
             h->d_mapbits, h->d_crows, h->closetab.n_rows, up, ws.d_table, ws.d_cand, plan.write_tables ? 1 : 0, d_prof, ref_lattice, ws.d_args, far ? plan.close_first : 0, plan.lean ? 1 | (plan.lean_ranks ? 2 : 0) | (plan.lean_count ? 4 : 0) : 0);
  if (d_prof && !ws.prof_deferred)
    VCHK(print_frame_prof(h, 0, n, true));
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// K7: Euclidean clustering of the voxel records in `ws` by the general kernels - brick level where a 4x4x4 brick is a clique for
// the tolerance, voxel level otherwise (VOFOD_CCL=voxel forces it: the tests compare both families against the oracle)
int launch_cluster(vofod_handle* h, Workspace& ws, const vplan::ChainPlan& plan, const GridParams& g, const vofod_handle::ClusterTables* ct)
{
  const uint32_t gv = (ws.vox_cap + 255u) / 256u;
  const unsigned long long* mapclose = plan.use_dilated ? h->d_mapclose.p : nullptr;  // k_flatten then answers hasCloseTo through the dilated image
  if (plan.bricks)
  {
    BrickParams bp = ct->bp;
    bp.bricks_cap = ws.bricks_cap;
    // (Fusing the brick registration into k_emit was measured slower - 194 us vs 96 + 50 us for 32 frames: the returning
    // atomicOr sits inside the load-balanced emission loop - so it is a kernel of its own.)
    KLAUNCH(h, k_brick_set, fgrid(g, gv), dim3(256), g, bp, ws.d_hdrs, ws.va, ws.ba);
    // the stencil's pairs as per-brick connectivity masks + transitive reduction; a stencil beyond 64 offsets (or without the
    // pair tables) takes the fused probe + union kernel.  (Round 1 also had "masks + batched hooking" behind VOFOD_BRICK_MODE=2:
    // CAS storms, 470 us against 206 us - removed in round 4.)
    if (plan.clusterer == vplan::Clusterer::BrickMasks)
    {
      // ws.d_table is free until k_finalize: it holds the per-brick connectivity masks (list order) in between
      unsigned long long* conn = reinterpret_cast<unsigned long long*>(ws.d_table.p);
      KLAUNCH(h, k_brick_conn, fgrid(g, gv * CONN_LANES), dim3(256), g, bp, ct->d_boffs, ct->d_sure, ct->d_amb, ws.d_hdrs, ws.ba, conn, ws.d_bconn);
      KLAUNCH(h, k_brick_link_tr, fgrid(g, gv), dim3(256), g, bp, ct->d_boffs, ct->d_pair, ws.d_hdrs, ws.ba, conn, ws.d_bconn);
    }
    else
      KLAUNCH(h, k_brick_union<1>, fgrid(g, gv), dim3(256), g, bp, ct->d_boffs, ct->d_sure, ct->d_amb, ws.d_hdrs, ws.ba);
    KLAUNCH(h, k_brick_root, fgrid(g, gv), dim3(256), g, bp, ws.d_hdrs, ws.ba, ws.d_bitmaps, ws.d_wprefix);
    KLAUNCH(h, k_flatten<1>, fgrid(g, gv), dim3(256), g, ws.d_hdrs, ws.va, ws.d_labels, ws.ba, ws.bricks_cap, h->mg, mapclose, h->d_mapbits, h->d_crows, h->closetab.n_rows);
    KLAUNCH(h, k_brick_clear, fgrid(g, gv), dim3(256), g, bp, ws.d_hdrs, ws.ba);
  }
  else
  {
    KLAUNCH(h, k_union<2>, fgrid(g, gv), dim3(256), g, ct->cp, ct->d_rows, ws.d_hdrs, ws.d_bitmaps, ws.d_wprefix, ws.va);
    KLAUNCH(h, k_flatten<0>, fgrid(g, gv), dim3(256), g, ws.d_hdrs, ws.va, ws.d_labels, ws.ba, 0u, h->mg, mapclose, h->d_mapbits, h->d_crows, h->closetab.n_rows);
  }
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// nVoxelsOver + occupancy image of the map, cached while the map and the threshold are unchanged
// nVoxelsOver (:715) from the patched counters of a sensor stream - fetched only when it can still change something (the
// background latch not yet set, debug output): a round trip of ~10 us per scan otherwise
int refresh_bgcount(vofod_handle* h)
{
  if (!h->bgcount_stale)
    return VOFOD_OK;
  h->bgcount_stale = false;
  if (!h->mapbits_valid)
    return VOFOD_OK;  // (the image is about to be rebuilt, the count with it)
  HIPCHK(hipMemcpy(h->h_bgcount, h->d_bgcount, sizeof(unsigned long long) * 8 * MB_SLOTS, hipMemcpyDeviceToHost));
  uint64_t t = 0;
  for (int i = 0; i < MB_SLOTS; i++)
    t += h->h_bgcount[8 * i];
  h->n_bg_voxels = t;
  h->bgcount_fresh = false;
  return VOFOD_OK;
}

int ensure_mapbits(vofod_handle* h, float thr)
{
  if (h->mapbits_valid && h->mapbits_thr == thr)
    return VOFOD_OK;
  h->bgcount_stale = false;  // (rebuilt below: image and count)
  // the image is shared with every batch in flight (their chains read it from streams of their own): let them finish first
  for (int t = 0; t < vofod_handle::MAX_INFLIGHT; t++)
    if (h->slot(t)->pending && h->slot(t)->ev_done)
      HIPCHK(hipEventSynchronize(h->slot(t)->ev_done));
  HIPCHK(hipMemsetAsync(h->d_bgcount, 0, sizeof(unsigned long long) * 8 * MB_SLOTS, h->stream));
  KLAUNCH(h, k_mapbits, dim3(1024), dim3(256), h->d_map, h->mg.n, thr, h->d_mapbits, h->d_bgcount);
  HIPCHK(hipMemcpyAsync(h->h_bgcount, h->d_bgcount, sizeof(unsigned long long) * 8 * MB_SLOTS, hipMemcpyDeviceToHost, h->stream));
  if (!h->ev_bgcount)
    HIPCHK(h->ev_bgcount.create(hipEventCreateWithFlags, hipEventDisableTiming));
  HIPCHK(hipEventRecord(h->ev_bgcount, h->stream));
  h->bgcount_fresh = true;
  h->mapbits_gen++;
  h->mapbits_valid = true;
  h->mapbits_thr = thr;
  return VOFOD_OK;  // h_counter is valid after the next stream sync
}

// the dilated occupancy image for read-only batches (see k_dilate); call after ensure_mapbits and the close-row upload
int ensure_mapclose(vofod_handle* h, const CloseParams& cpar)
{
  if (h->mapclose_gen == h->mapbits_gen && h->mapclose_dist == h->closetab.max_dist)
    return VOFOD_OK;
  const size_t words = (h->mg.n + 63) / 64 + 2;
  HIPCHK(hipMemsetAsync(h->d_mapclose, 0, words * sizeof(unsigned long long), h->stream));
  const uint64_t chunks = static_cast<uint64_t>(h->mg.sz) * h->mg.sy * ((h->mg.sx + 63) / 64);
  KLAUNCH(h, k_dilate, dim3(static_cast<uint32_t>((chunks + 255) / 256)), dim3(256), h->mg, cpar, h->d_crows, h->d_mapbits, h->d_mapclose);
  HIPCHK(hipStreamSynchronize(h->stream));  // other chains read it from their own streams
  h->mapclose_gen = h->mapbits_gen;
  h->mapclose_dist = h->closetab.max_dist;
  return VOFOD_OK;
}

float map_cmax(const vofod_handle* h)
{
  float c = 0;
  for (int a = 0; a < 3; a++)
  {
    c = std::max(c, std::fabs(h->mg.off[a]));
    c = std::max(c, std::fabs(h->mg.off[a] + h->mg.vs * (a == 0 ? h->mg.sx : a == 1 ? h->mg.sy : h->mg.sz)));
  }
  return c + 2 * h->mg.vs;
}

int raycast_begin_locked(vofod_handle* h, const vofod_scan* scan, const float tf[12], const float* d_staged_poses);
int raycast_finish_locked(vofod_handle* h);

int ensure_explore(vofod_handle* h, ExploreBufs& eb, uint32_t F, size_t n_jobs, size_t n_members)
{
  const size_t ovl_words = (h->mg.n + 63) / 64;
  if (eb.F() < F)
  {
    // (all eight go before the first comes back: the overlay is large.  Without d_visited there are no frame slots.)
    for (DevBuf<uint32_t>* b : {&eb.d_visited, &eb.d_stack, &eb.d_explored, &eb.d_touched, &eb.d_ovl_list, &eb.d_ovl_count, &eb.d_job_begin})
      b->reset();
    HIPCHK(eb.d_overlay.alloc(ovl_words * F));
    HIPCHK(hipMemset(eb.d_overlay, 0, sizeof(unsigned long long) * ovl_words * F));
    HIPCHK(eb.d_stack.alloc(static_cast<size_t>(vc::EX_CELLS) * F));
    HIPCHK(eb.d_explored.alloc(static_cast<size_t>(vc::EX_CELLS) * F));
    HIPCHK(eb.d_touched.alloc(static_cast<size_t>(vc::EX_CELLS) * F));
    HIPCHK(eb.d_ovl_list.alloc(static_cast<size_t>(vc::EX_CELLS) * F));
    HIPCHK(eb.d_ovl_count.alloc(F));
    HIPCHK(hipMemset(eb.d_ovl_count, 0, sizeof(uint32_t) * F));
    HIPCHK(eb.d_job_begin.alloc(F + 1));
    HIPCHK(eb.d_visited.alloc(static_cast<size_t>(vc::EX_WORDS) * F));
    HIPCHK(hipMemset(eb.d_visited, 0, sizeof(uint32_t) * vc::EX_WORDS * F));
    HIPCHK(hipDeviceSynchronize());  // null-stream memsets vs non-blocking streams
  }
  if (eb.d_results.n < n_jobs)  // (allocated behind d_jobs: it stands for both)
  {
    const size_t cap = std::max<size_t>(n_jobs * 2, 1024);
    eb.d_results.reset();
    HIPCHK(eb.d_jobs.alloc(cap));
    HIPCHK(eb.d_results.alloc(cap));
  }
  if (eb.d_members.n < 3 * n_members)
    HIPCHK(eb.d_members.alloc(3 * std::max<size_t>(n_members * 2, 1 << 16)));
  return VOFOD_OK;
}

// Fallback of k_explore for one frame: the same flood fills and sums on read-back boxes of the map.
int host_explore_frame(vofod_handle* h, std::vector<HostCluster>& cl, const vt::MemberIndex& by_root, const std::vector<int>& job_of,
                       const std::vector<vc::ExploreJob>& jobs, std::vector<vc::ExploreResult>& results, bool no_update, float thr_frontiers, float thr_new, const vofod_dyn_params& dp)
{
  std::vector<uint64_t> pending;  // voxels this scan's classification turned into frontiers (:1712-1715)
  auto unlin = [&](uint64_t li, int i3[3]) {
    i3[0] = static_cast<int>(li % h->hg.s[0]);
    i3[1] = static_cast<int>((li / h->hg.s[0]) % h->hg.s[1]);
    i3[2] = static_cast<int>(li / (static_cast<uint64_t>(h->hg.s[0]) * h->hg.s[1]));
  };
  for (size_t ci = 0; ci < cl.size(); ci++)
  {
    const int ji = job_of[ci];
    if (ji < 0)
      continue;
    const vc::ExploreJob& job = jobs[ji];
    const vt::MemberSpan mem = by_root.of(cl[ci].rec.root);
    const int R = job.R;
    int lo[3], hi[3];
    for (int a = 0; a < 3; a++)
    {
      lo[a] = INT32_MAX;
      hi[a] = INT32_MIN;
    }
    for (const vt::Member& m : mem)
    {
      int o[3];
      h->hg.coordToIdx(m.p, o);
      for (int a = 0; a < 3; a++)
      {
        lo[a] = std::min(lo[a], o[a] - R - 1);
        hi[a] = std::max(hi[a], o[a] + R + 1);
      }
    }
    vt::Box box;
    VCHK(read_box(h, h->d_map, lo, hi, box));
    for (const uint64_t li : pending)
    {
      int i3[3];
      unlin(li, i3);
      if (box.has(i3))
        box.v[box.at(i3)] = thr_frontiers;
    }
    bool is_floating = true;
    std::vector<uint64_t> explored;
    for (const vt::Member& m : mem)
    {
      if (vt::explore_to_ground(h->hg, box, m.p, thr_frontiers, thr_new, static_cast<float>(R), explored))
      {
        is_floating = false;
        break;
      }
      for (const uint64_t li : explored)
      {
        int i3[3];
        unlin(li, i3);
        box.v[box.at(i3)] = thr_frontiers;
        pending.push_back(li);
      }
    }
    results[ji].floating = is_floating;
  }
  if (!no_update && !pending.empty())
  {
    VCHK(scatter_set(h, h->d_map, pending, thr_frontiers));
    h->mapbits_valid = false;
  }
  // uncertainty sums (:851-865) after every frontier write of the frame
  for (size_t ci = 0; ci < cl.size(); ci++)
  {
    const int ji = job_of[ci];
    if (ji < 0 || !results[ji].floating)
      continue;
    const vc::ExploreJob& job = jobs[ji];
    const vt::MemberSpan mem = by_root.of(cl[ci].rec.root);
    int mn[3] = {job.box_lo[0], job.box_lo[1], job.box_lo[2]}, mx[3] = {job.box_hi[0], job.box_hi[1], job.box_hi[2]};
    vt::Box sub;
    VCHK(read_box(h, h->d_map, mn, mx, sub));
    if (no_update)
      for (const uint64_t li : pending)
      {
        int i3[3];
        unlin(li, i3);
        if (sub.has(i3))
          sub.v[sub.at(i3)] = thr_frontiers;
      }
    const float ray = static_cast<float>(dp.voxel_map__scores__ray);
    for (const vt::Member& m : mem)
    {
      int o[3];
      h->hg.coordToIdx(m.p, o);
      if (sub.has(o))
        sub.v[sub.at(o)] = ray;
    }
    double u = 0.0;
    for (const float val : sub.v)
      u += 1.0 - val / dp.voxel_map__scores__ray;
    results[ji].conf_sum = u;
  }
  return VOFOD_OK;
}

}  // namespace

#include "frames_launch.h"
#include "frames_collect.h"
#include "api_gate.h"
#include "api_host.h"
#include "driver_aux.h"
#include "api_maps.h"
#include "api_render.h"
#include "api_match.h"
#include "api_distance.h"
#include "api_frames.h"
#include "collective.h"
#include "mapsync_host.h"
#include "world_sync_host.h"
