// The fallback contract on the command line: the plan of a launch from its inputs, on the CPU.
//   chain_plan_check [key=value ...]     prints plan_chain's answer in one line of names
// Every field of vplan::PlanInputs and vplan::Switches is a key; the defaults are the benchmarked batch (128 submitted frames of
// OS1-128 at 0.25 m on a warmed map, every switch on).  Includes chain_plan.h and nothing else of the library
// (tests/test_chain_plan_cpu.py builds it with the host compiler and its sanitizers, and holds the kernels' constants below
// to the headers that define them).
#include <cstdio>
#include <map>
#include <string>

#include "chain_plan.h"

// the plan in one line of names
static std::string describe(const vplan::ChainPlan& p)
{
  std::string s = std::string("voxeliser=") + name(p.voxeliser) + " clusterer=" + name(p.clusterer) + " closefar=" + name(p.closefar) + " finalize=" + name(p.finalize) + " tail=" + name(p.tail);
  const auto flag = [&](const char* k, long v) { s += std::string(" ") + k + "=" + std::to_string(v); };
  flag("use_dilated", p.use_dilated);
  flag("single_update", p.single_update);
  flag("dtail", p.dtail);
  flag("raycast_ahead", p.raycast_ahead);
  flag("bricks", p.bricks);
  flag("lds", p.lds);
  flag("lb_limit", p.lb_limit);
  flag("in_packed", p.in_packed);
  flag("clear_bitmap", p.clear_bitmap);
  flag("slab_groups", p.slab_groups);
  flag("close_first", p.close_first);
  flag("keep_dirty", p.keep_dirty);
  flag("far_single", p.far_single);
  flag("far_ran", p.far_ran);
  flag("lean", p.lean);
  flag("write_tables", p.write_tables);
  flag("mapbits_patched", p.mapbits_patched);
  flag("bitmap_clean_after", p.bitmap_clean_after);
  return s;
}

int main(int argc, char** argv)
{
  vplan::PlanInputs in;
  in.n = 128;
  in.no_update = true;
  in.submitted = true;
  in.vox_cap = 65536;
  in.words_cap = 309444;  // 482 x 402 x 102 cells
  in.bricks_cap = 318240;
  in.bitmap_clean = true;
  in.brick_ok = in.lds_ok = in.pair_table = true;
  in.n_off = 62;
  in.n_rows = 13;
  in.ref_lattice_on = in.layout_packed = in.patchable = true;
  in.far_max = 4096;       // kernels_far.h FAR_MAX
  in.lb_max = 7168;        // kernels_brick_lds.h LB_MAX
  in.slab_words64 = 16384; // kernels_slab.h SLAB_WORDS64
  const std::map<std::string, bool*> flags = {
      {"close_first", &in.sw.close_first}, {"lean_emit", &in.sw.lean_emit}, {"lean_ranks", &in.sw.lean_ranks}, {"lean_count", &in.sw.lean_count}, {"device_tail", &in.sw.device_tail}, {"brick_lds", &in.sw.brick_lds}, {"brick_ccl", &in.sw.brick_ccl},
      {"dilate", &in.sw.dilate}, {"slabs", &in.sw.slabs}, {"slab_emit", &in.sw.slab_emit}, {"no_update", &in.no_update}, {"submitted", &in.submitted}, {"dbg", &in.dbg},
      {"dbg_far_only", &in.dbg_far_only}, {"auto_raycast", &in.auto_raycast}, {"bitmap_clean", &in.bitmap_clean}, {"brick_ok", &in.brick_ok}, {"lds_ok", &in.lds_ok},
      {"pair_table", &in.pair_table}, {"cf_off", &in.cf_off}, {"lds_ccl_off", &in.lds_ccl_off}, {"ref_lattice_on", &in.ref_lattice_on}, {"layout_packed", &in.layout_packed},
      {"patchable", &in.patchable}};
  const std::map<std::string, uint32_t*> counts = {{"n", &in.n}, {"vox_cap", &in.vox_cap}, {"words_cap", &in.words_cap}, {"bricks_cap", &in.bricks_cap},
                                                   {"far_max", &in.far_max}, {"lb_max", &in.lb_max}, {"slab_words64", &in.slab_words64}};
  for (int i = 1; i < argc; i++)
  {
    const std::string arg = argv[i];
    const size_t eq = arg.find('=');
    if (eq == std::string::npos)
    {
      std::fprintf(stderr, "%s: not key=value\n", argv[i]);
      return 2;
    }
    const std::string key = arg.substr(0, eq);
    const long v = std::strtol(arg.c_str() + eq + 1, nullptr, 10);
    if (const auto f = flags.find(key); f != flags.end())
      *f->second = v != 0;
    else if (const auto c = counts.find(key); c != counts.end())
      *c->second = static_cast<uint32_t>(v);
    else if (key == "n_off")
      in.n_off = static_cast<int>(v);
    else if (key == "n_rows")
      in.n_rows = static_cast<int>(v);
    else if (key == "lds_max_bricks")  // (VOFOD_LDS_MAX_BRICKS; -1: not set)
      in.sw.lds_max_bricks = static_cast<int>(v);
    else
    {
      std::fprintf(stderr, "%s: unknown key\n", key.c_str());
      return 2;
    }
  }
  if (in.n == 0 || in.slab_words64 == 0)
  {
    std::fprintf(stderr, "n and slab_words64 must be positive (an empty batch launches nothing)\n");
    return 2;
  }
  std::printf("%s\n", describe(vplan::plan_chain(in)).c_str());
  return 0;
}
