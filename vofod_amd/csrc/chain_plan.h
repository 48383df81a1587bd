// The kernel chain of one launch, decided once (the fallback contract, as code): the switches, what the host knows
// before the first kernel of the call is enqueued, and plan_chain, a pure function from the one to the other.  Host only: no HIP
// header, no handle, no workspace, no device pointer - vofod_amd/csrc/chain_plan_check.cpp compiles this file alone and prints
// the plan of any input (tests/test_chain_plan_cpu.py holds the table of DESIGN 5.4 against it).  The stages of a launch
// (frames_launch.h, vofod_hip.hip) execute the plan and decide nothing.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace vplan
{

// VOFOD_<NAME>=0 switches a fast path off (README "Environment switches").  Read on every call, not cached: a dozen getenv per
// batch cost ~1 us, and the tests flip the fallbacks inside one process (a `static const` here made every switch stick to
// its first reading - and every in-process fallback test after the first call vacuous).
inline bool switch_off(const char* name)
{
  const char* v = std::getenv(name);
  return v && std::atoi(v) == 0;
}

// The switches that route a launch (true: the fast path is on), as one entry-point call reads them.
struct Switches
{
  bool close_first = true;   // VOFOD_CLOSE_FIRST=0: the full clustering everywhere
  bool lean_emit = true;     // VOFOD_LEAN_EMIT=0: the close-first frame kernel emits every voxel record
  bool lean_ranks = true;    // VOFOD_LEAN_RANKS=0: a lean launch still builds its rank tables for every brick
  bool lean_count = true;    // VOFOD_LEAN_COUNT=0: a lean launch still counts its weights by walking every code
  bool device_tail = true;   // VOFOD_DEVICE_TAIL=0: the full tables come back for the host tail
  bool brick_lds = true;     // VOFOD_BRICK_LDS=0: the global-memory clustering kernels
  bool brick_ccl = true;     // VOFOD_CCL=voxel: the voxel-level clustering kernels
  bool dilate = true;        // VOFOD_DILATE=0: hasCloseTo by stencil sweep instead of the map's dilated image
  bool slabs = true;         // VOFOD_SLABS=0: the global-atomic voxeliser
  bool slab_emit = true;     // VOFOD_SLAB_EMIT=0: the separate emission kernels behind k_slab for every batch size
  int lds_max_bricks = -1;   // VOFOD_LDS_MAX_BRICKS=n: bricks per frame the LDS clustering takes (not set, or negative: its own limit)
};

inline Switches read_switches()
{
  Switches s;
  s.close_first = !switch_off("VOFOD_CLOSE_FIRST");
  s.lean_emit = !switch_off("VOFOD_LEAN_EMIT");
  s.lean_ranks = !switch_off("VOFOD_LEAN_RANKS");
  s.lean_count = !switch_off("VOFOD_LEAN_COUNT");
  s.device_tail = !switch_off("VOFOD_DEVICE_TAIL");
  s.brick_lds = !switch_off("VOFOD_BRICK_LDS");
  const char* ccl = std::getenv("VOFOD_CCL");
  s.brick_ccl = !(ccl && std::strcmp(ccl, "voxel") == 0);
  s.dilate = !switch_off("VOFOD_DILATE");
  s.slabs = !switch_off("VOFOD_SLABS");
  s.slab_emit = !switch_off("VOFOD_SLAB_EMIT");
  if (const char* v = std::getenv("VOFOD_LDS_MAX_BRICKS"))
    s.lds_max_bricks = std::atoi(v);
  return s;
}

// What the host knows when it plans a launch.  All by value.
struct PlanInputs
{
  Switches sw;
  // the call
  uint32_t n = 1;             // frames
  bool no_update = false;     // VOFOD_SCAN_NO_MAP_UPDATE
  bool submitted = false;     // vofod_batch_submit: collected by another call
  bool dbg = false;           // debug output - or any caller that reads the labels of EVERY cluster (vofod_cluster, sepclusters)
  bool dbg_far_only = false;  // ... its far-only view (vofod_scan_debug::far_only)
  bool auto_raycast = false;  // VOFOD_SCAN_AUTO_RAYCAST
  // the workspace
  uint32_t vox_cap = 0, words_cap = 0, bricks_cap = 0;
  bool bitmap_clean = false;  // its occupancy bitmaps are all-zero
  // the cached cluster tables of (leaf, tolerance, coordinate bound)
  bool brick_ok = false;      // a 4x4x4 brick is a clique for the tolerance
  bool lds_ok = false;        // ... and the tables of the LDS clustering exist
  int n_off = 0;              // brick offsets of the forward stencil
  bool pair_table = false;    // ... and their pair table (at most 64 offsets)
  int n_rows = 0;             // rows of the voxel-level stencil
  // the two latches, as they stand when the plan is made
  bool cf_off = false;        // a batch overflowed the close-first capacities and the background has not grown since
  bool lds_ccl_off = false;   // this launch is the re-run of a batch that overflowed the LDS kernels
  // the reference lattice of the frame kernel computed from the grid parameters: it fits, and eps < 0.05
  bool ref_lattice_on = false;
  // the staged inputs: every frame's columns at stride 4, a multiple of four points (four at least), 16-byte bases
  bool layout_packed = false;
  // the update: one voxel of the scan per map cell (the aligned lattice), and the frontier value is no background value
  bool patchable = false;
  // capacities of the kernels (kernels_far.h, kernels_brick_lds.h, kernels_slab.h)
  uint32_t far_max = 0, lb_max = 0, slab_words64 = 1;
};

enum class Voxeliser { Frame, SlabEmit, Slabs, Bitmap };        // the frame kernel reads the input itself: nothing runs ahead of it
enum class Clusterer { FrameFar, FrameFull, FarSingle, BrickMasks, BrickUnion, Voxel };
enum class CloseFar { Fused, InPlace, Split };                  // k_closefar: not needed / sweeps in place / hands a list to k_closefar_sweep
enum class Finalize { Fused, Finalize, FinalizeFar };           // cluster table + map update: by the clustering / k_finalize / k_finalize_far
enum class Tail { Far, ThreeKernels, Pack };                    // k_tail_far / k_tail_prep + k_explore + k_tail_finish / k_pack for the host tail

// names for trace lines, in the enumerators' order
inline const char* name(Voxeliser v) { static const char* const s[] = {"frame", "k_slab_emit", "k_slab", "bitmap"}; return s[static_cast<int>(v)]; }
inline const char* name(Clusterer c) { static const char* const s[] = {"k_frame_lds_far", "k_frame_lds_full", "far_single", "brick_masks", "k_brick_union", "voxel"}; return s[static_cast<int>(c)]; }
inline const char* name(CloseFar c) { static const char* const s[] = {"fused", "k_closefar", "k_closefar+sweep"}; return s[static_cast<int>(c)]; }
inline const char* name(Finalize f) { static const char* const s[] = {"fused", "k_finalize", "k_finalize_far"}; return s[static_cast<int>(f)]; }
inline const char* name(Tail t) { static const char* const s[] = {"k_tail_far", "k_tail_prep+k_explore+k_tail_finish", "k_pack"}; return s[static_cast<int>(t)]; }

// What runs, and the few scalars the launches take.
struct ChainPlan
{
  // map images
  bool no_update = false;
  bool use_dilated = false;     // read-only batches: the map's dilated image answers hasCloseTo with one bit per voxel
  bool single_update = false;   // one map-updating scan, synchronous: the reference's own mode
  // the chain
  Voxeliser voxeliser = Voxeliser::Bitmap;
  Clusterer clusterer = Clusterer::Voxel;
  CloseFar closefar = CloseFar::InPlace;
  Finalize finalize = Finalize::Finalize;
  Tail tail = Tail::Pack;
  bool dtail = false;           // the classification tail runs on the device (tail != Pack)
  bool raycast_ahead = false;   // the raycast role of VOFOD_SCAN_AUTO_RAYCAST runs between the chain and the device tail
  // clustering family
  bool bricks = false;          // brick-level clustering (GridParams::sparse_prefix)
  bool lds = false;             // ... inside one workgroup's LDS
  uint32_t lb_limit = 0;        // bricks per frame the LDS clustering takes
  // voxeliser
  bool in_packed = false;       // frame kernel: the input pass uses 16-byte loads
  bool clear_bitmap = false;    // the occupancy bitmaps are cleared ahead of the voxeliser
  uint32_t slab_groups = 0;     // k_slab: workgroups per frame
  // close first
  int close_first = 0;          // frame kernel: 1 = cluster the far voxels only, 2 = the same with labels for the far-only debug view
  bool keep_dirty = false;      // nobody reads the bitmaps past their set bits: k_finalize does not clean them
  bool far_single = false;      // a single map-updating scan clusters close first on the general path (kernels_far.h)
  bool far_ran = false;         // cluster table and member list are in the order k_tail_far reads
  bool lean = false;            // k_frame_lds_far writes the voxel records of pure-far bricks only
  bool lean_ranks = false;      // ... and ranks through tables built for those bricks only (kernels_frame.h, pass 4)
  bool lean_count = false;      // ... and counts the weights from a filtered list of those bricks' codes (kernels_frame.h, pass 3b)
  bool write_tables = false;    // the frame kernel writes cluster table and candidate list itself
  bool mapbits_patched = false; // k_finalize_far keeps the map's occupancy image and counters up to date with the scan's update
  bool bitmap_clean_after = false;  // Workspace::bitmap_clean once the chain is enqueued

  bool frame() const { return voxeliser == Voxeliser::Frame; }
};

// Read-only batches of four frames and more answer hasCloseTo from the map's dilated image.  (On its own as well: the image is
// prepared before the cluster tables - a plan input - are looked up.)
inline bool wants_dilated(const Switches& sw, bool no_update, uint32_t n) { return sw.dilate && no_update && n >= 4; }

inline ChainPlan plan_chain(const PlanInputs& in)
{
  const Switches& sw = in.sw;
  const uint32_t n = in.n;
  ChainPlan p;
  // ---- map images, tail
  p.no_update = in.no_update;
  p.use_dilated = wants_dilated(sw, in.no_update, n);
  p.single_update = !in.no_update && n == 1 && !in.submitted;
  p.dtail = sw.device_tail && !in.dbg && ((n >= 4 && in.no_update) || p.single_update);
  p.raycast_ahead = p.dtail && p.single_update && in.auto_raycast;
  // ---- clustering family: bricks where a 4x4x4 brick is a clique for the tolerance, inside LDS for read-only batches
  p.bricks = sw.brick_ccl && in.brick_ok && in.bricks_cap > 0;
  p.lds = in.no_update && n >= 4 && sw.brick_lds && p.bricks && in.lds_ok && !in.lds_ccl_off;
  p.lb_limit = std::min<uint32_t>(in.lb_max, static_cast<uint32_t>(sw.lds_max_bricks));
  // ---- voxeliser: the frame kernel needs the LDS clustering and its reference lattice; lattices of at most 32 slabs of 1 Mi cells
  // are built slab by slab in LDS (a single frame is served faster by the whole chip through the global bitmap)
  const uint32_t n_slabs = (in.words_cap + in.slab_words64 - 1) / in.slab_words64;
  if (p.lds && in.ref_lattice_on)
    p.voxeliser = Voxeliser::Frame;
  else if (sw.slabs && n >= 4 && n_slabs <= 32)
    p.voxeliser = (sw.slab_emit && n >= 128) ? Voxeliser::SlabEmit : Voxeliser::Slabs;
  else
    p.voxeliser = Voxeliser::Bitmap;
  const bool slab = p.voxeliser == Voxeliser::SlabEmit || p.voxeliser == Voxeliser::Slabs;
  p.in_packed = p.frame() && in.layout_packed;
  // (voxel-level clustering: neighbour windows run into the words past the lattice, they must read as zero)
  p.clear_bitmap = !in.bitmap_clean && (p.voxeliser == Voxeliser::Bitmap || (slab && !p.bricks));
  // (all slabs in parallel for small batches, fewer workgroups walking several slabs otherwise)
  p.slab_groups = n <= 32 ? n_slabs : std::max(1u, std::min(n_slabs, 512u / n));
  // ---- close first.  k_slab rewrites the bitmap densely and the brick clustering reads it at set bits only, the frame kernel
  // does not touch it at all: no need to clean it after use
  p.keep_dirty = p.frame() || (slab && p.bricks);
  p.close_first = (sw.close_first && p.use_dilated && !in.cf_off) ? (in.dbg ? (in.dbg_far_only ? 2 : 0) : 1) : 0;
  p.far_single = sw.close_first && !in.cf_off && !in.dbg && p.single_update && sw.device_tail && !p.frame() && !p.keep_dirty && in.n_rows > 0 && in.vox_cap >= in.far_max;
  const bool up_tables = p.keep_dirty && in.no_update;  // the clustering gets the update parameters
  p.far_ran = p.frame() && up_tables && p.use_dilated && p.close_first != 0;
  p.lean = p.far_ran && p.close_first == 1 && sw.lean_emit;
  p.lean_ranks = p.lean && sw.lean_ranks;
  p.lean_count = p.lean && sw.lean_count;
  p.write_tables = p.frame() && up_tables && p.use_dilated;
  if (p.far_single)
    p.clusterer = Clusterer::FarSingle;
  else if (p.frame())
    p.clusterer = p.far_ran ? Clusterer::FrameFar : Clusterer::FrameFull;
  else if (p.bricks)
    p.clusterer = (in.n_off <= 64 && in.pair_table) ? Clusterer::BrickMasks : Clusterer::BrickUnion;
  else
    p.clusterer = Clusterer::Voxel;
  // (k_flatten and the frame kernel answer hasCloseTo through the dilated image, k_closefar of the far-single chain by stencil;
  // few frames: the undecided voxels go through a list to a sweep kernel with 16 lanes per voxel; many: swept in place)
  p.closefar = (p.far_single || p.use_dilated) ? CloseFar::Fused : (n < 8 && !p.use_dilated) ? CloseFar::Split : CloseFar::InPlace;
  p.finalize = p.far_single ? Finalize::FinalizeFar : p.write_tables ? Finalize::Fused : Finalize::Finalize;
  p.mapbits_patched = p.far_single && in.patchable;
  p.bitmap_clean_after = p.frame() ? in.bitmap_clean : !p.keep_dirty;
  p.tail = !p.dtail ? Tail::Pack : ((p.far_ran && p.close_first == 1) || p.far_single) ? Tail::Far : Tail::ThreeKernels;
  return p;
}

}  // namespace vplan
