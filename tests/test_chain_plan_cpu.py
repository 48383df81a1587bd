"""The fallback contract as an executable table: plan_chain (vofod_amd/csrc/chain_plan.h), the pure function that
decides a launch's kernel chain, behind the command line of vofod_amd/csrc/chain_plan_check.cpp - built here with the host
compiler and its address / undefined-behaviour sanitizers, nothing of the GPU, nothing loaded into this process.

Every row of the 5.4 table that the plan decides stands here in both directions: WITH the switch the general path, and WITHOUT
it, under the condition the table names, the same path.  (VOFOD_EXPLORE=host is read by the host tail at collect time: it is no
part of the plan.)  The program's defaults are the benchmarked batch: 128 submitted read-only frames, every switch on."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vofod_amd" / "csrc"
SLAB_WORDS64 = 16384

SCAN = dict(n=1, no_update=0, submitted=0)           # one map-updating scan, synchronous
BATCH4 = dict(n=4, submitted=0)                       # a synchronous read-only batch
UPDATING_BATCH = dict(n=4, no_update=0, submitted=0)  # a batch that updates the map


@pytest.fixture(scope="module")
def check():
    r = subprocess.run(["make", "-C", str(CSRC), "chain_plan_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = CSRC / "chain_plan_check"
    cache = {}

    def plan(**kv):
        key = tuple(sorted(kv.items()))
        if key not in cache:
            out = subprocess.run([str(exe)] + [f"{k}={int(v)}" for k, v in kv.items()], capture_output=True, text=True)
            assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands on stderr)
            cache[key] = dict(w.split("=", 1) for w in out.stdout.split())
        return cache[key]

    return plan


def has(plan, **want):
    got = {k: plan[k] for k in want}
    assert got == {k: str(v) for k, v in want.items()}, plan


def test_the_programs_constants_are_the_kernels():
    src = (CSRC / "chain_plan_check.cpp").read_text()
    for field, header, name in (("far_max", "kernels_far.h", "FAR_MAX"), ("lb_max", "kernels_brick_lds.h", "LB_MAX"), ("slab_words64", "kernels_slab.h", "SLAB_WORDS64")):
        mine = int(re.search(rf"in\.{field} = (\d+);", src).group(1))
        theirs = int(re.search(rf"constexpr \w+ {name} = (\d+);", (CSRC / header).read_text()).group(1))
        assert mine == theirs, (field, mine, theirs)
    assert int(re.search(r"in\.slab_words64 = (\d+);", src).group(1)) == SLAB_WORDS64
    # host only: no HIP header, and nothing of the library that includes one
    includes = re.findall(r'#include [<"]([^>"]+)[>"]', (CSRC / "chain_plan.h").read_text())
    assert includes and all("hip" not in i and not i.endswith(".h") for i in includes), includes
    assert re.findall(r'#include "([^"]+)"', src) == ["chain_plan.h"]


def test_benchmarked_default(check):
    """frame kernel, close first, packed input pass, lean emission, the one-kernel tail; nothing else in the chain"""
    has(check(), voxeliser="frame", clusterer="k_frame_lds_far", in_packed=1, lean=1, tail="k_tail_far", closefar="fused", finalize="fused", close_first=1, far_ran=1,
        write_tables=1, use_dilated=1, dtail=1, bricks=1, lds=1, lb_limit=7168, keep_dirty=1, clear_bitmap=0, far_single=0, raycast_ahead=0, mapbits_patched=0)
    has(check(layout_packed=0), voxeliser="frame", clusterer="k_frame_lds_far", in_packed=0)
    # the frame kernel leaves the bitmaps as they were
    has(check(bitmap_clean=1), bitmap_clean_after=1)
    has(check(bitmap_clean=0), bitmap_clean_after=0, clear_bitmap=0)


def test_close_first(check):
    full = dict(clusterer="k_frame_lds_full", close_first=0, far_ran=0, lean=0, tail="k_tail_prep+k_explore+k_tail_finish")
    has(check(close_first=0), voxeliser="frame", write_tables=1, **full)
    has(check(cf_off=1), voxeliser="frame", write_tables=1, **full)                                # the latch
    has(check(dbg=1, **BATCH4), clusterer="k_frame_lds_full", close_first=0, tail="k_pack")        # debug output of all clusters
    has(check(dbg=1, dbg_far_only=1, **BATCH4), clusterer="k_frame_lds_far", close_first=2, far_ran=1, tail="k_pack")
    has(check(**UPDATING_BATCH), voxeliser="k_slab", clusterer="brick_masks", close_first=0, use_dilated=0, dtail=0)  # map-updating batches
    # a single map-updating scan: close first on the general path, the brick kernels otherwise
    far = dict(clusterer="far_single", far_single=1, closefar="fused", finalize="k_finalize_far", tail="k_tail_far", voxeliser="bitmap", mapbits_patched=1)
    bricks = dict(clusterer="brick_masks", far_single=0, closefar="k_closefar+sweep", finalize="k_finalize", tail="k_tail_prep+k_explore+k_tail_finish", mapbits_patched=0)
    has(check(**SCAN), single_update=1, **far)
    has(check(patchable=0, **SCAN), far_single=1, mapbits_patched=0)
    has(check(close_first=0, **SCAN), **bricks)
    has(check(cf_off=1, **SCAN), **bricks)
    has(check(vox_cap=4095, **SCAN), **bricks)   # FAR_MAX - 1
    has(check(vox_cap=4096, **SCAN), **far)      # FAR_MAX
    has(check(n_rows=0, **SCAN), **bricks)
    has(check(dbg=1, **SCAN), clusterer="brick_masks", far_single=0, tail="k_pack")
    has(check(device_tail=0, **SCAN), clusterer="brick_masks", far_single=0, tail="k_pack")
    has(check(n=1, no_update=0, submitted=1), single_update=0, far_single=0, dtail=0)


def test_lean_emit(check):
    has(check(lean_emit=0), clusterer="k_frame_lds_far", close_first=1, lean=0, tail="k_tail_far")  # same kernels, same label
    has(check(dbg=1, dbg_far_only=1, **BATCH4), clusterer="k_frame_lds_far", lean=0)               # the far-only view reads the whole cloud
    has(check(close_first=0), clusterer="k_frame_lds_full", lean=0)


def test_lds_max_bricks_and_the_rerun(check):
    has(check(lds_max_bricks=64), lb_limit=64, voxeliser="frame")
    has(check(lds_max_bricks=100000), lb_limit=7168)
    general = dict(voxeliser="k_slab_emit", clusterer="brick_masks", lds=0, close_first=1, far_ran=0, closefar="fused", finalize="k_finalize",
                   tail="k_tail_prep+k_explore+k_tail_finish", keep_dirty=1, bitmap_clean_after=0)
    has(check(lds_ccl_off=1), **general)         # the re-run of a batch that overflowed the LDS kernels
    # a reference lattice that does not fit: the same general kernels, directly (the clustering family stays "LDS", no frame kernel)
    has(check(ref_lattice_on=0), **{**general, "lds": 1})


def test_brick_lds(check):
    general = dict(voxeliser="k_slab_emit", clusterer="brick_masks", lds=0, finalize="k_finalize")
    has(check(brick_lds=0), **general)
    has(check(lds_ccl_off=1), **general)                                             # that re-run
    has(check(lds_ok=0), **general)
    has(check(n=3, submitted=0), voxeliser="bitmap", clusterer="brick_masks", lds=0)  # every batch of < 4 frames
    has(check(n=4, submitted=0), voxeliser="frame", lds=1)
    has(check(dbg=1, **SCAN), voxeliser="bitmap", clusterer="brick_masks", lds=0)     # single scans with debug output
    has(check(cf_off=1, **SCAN), voxeliser="bitmap", clusterer="brick_masks", lds=0)  # ... or on a cold map
    # the brick graph by connectivity masks while the stencil has at most 64 offsets and a pair table
    has(check(brick_lds=0, n_off=64), clusterer="brick_masks")
    has(check(brick_lds=0, n_off=65), clusterer="k_brick_union")
    has(check(brick_lds=0, pair_table=0), clusterer="k_brick_union")


def test_ccl_voxel(check):
    voxel = dict(clusterer="voxel", bricks=0, lds=0, voxeliser="k_slab_emit", keep_dirty=0, bitmap_clean_after=1)
    has(check(brick_ccl=0), **voxel)
    has(check(brick_ok=0), **voxel)      # a brick is no clique for the tolerance
    has(check(bricks_cap=0), **voxel)
    # voxel-level neighbour windows read past the lattice: a dirty bitmap is cleared ahead of the slab voxeliser, a brick family's is not
    has(check(brick_ccl=0, bitmap_clean=0), clear_bitmap=1)
    has(check(brick_lds=0, bitmap_clean=0), clear_bitmap=0)
    has(check(brick_ccl=0, bitmap_clean=0, **SCAN), voxeliser="bitmap", clear_bitmap=1)
    has(check(bitmap_clean=0, **SCAN), voxeliser="bitmap", clear_bitmap=1)
    has(check(bitmap_clean=1, **SCAN), voxeliser="bitmap", clear_bitmap=0)


def test_dilate_and_the_split_sweep(check):
    has(check(dilate=0), use_dilated=0, close_first=0, clusterer="k_frame_lds_full", write_tables=0, closefar="k_closefar", finalize="k_finalize")
    has(check(dilate=0, n=8, submitted=0), closefar="k_closefar")
    has(check(dilate=0, n=7, submitted=0), closefar="k_closefar+sweep")
    has(check(dbg=1, **SCAN), use_dilated=0, closefar="k_closefar+sweep")         # every map-updating scan
    has(check(n=3, submitted=0), use_dilated=0, closefar="k_closefar+sweep")      # batches of < 4 frames
    has(check(n=4, submitted=0), use_dilated=1, closefar="fused")
    has(check(n=8, no_update=0, submitted=0), use_dilated=0, closefar="k_closefar")


def test_slabs(check):
    has(check(brick_lds=0, slabs=0), voxeliser="bitmap", keep_dirty=0, bitmap_clean_after=1)
    has(check(brick_lds=0, n=3, submitted=0), voxeliser="bitmap")                                   # < 4 frames
    has(check(brick_lds=0, n=4, submitted=0), voxeliser="k_slab", slab_groups=19)
    has(check(brick_lds=0, words_cap=32 * SLAB_WORDS64), voxeliser="k_slab_emit")                   # 32 slabs
    has(check(brick_lds=0, words_cap=32 * SLAB_WORDS64 + 1), voxeliser="bitmap")                    # n_slabs = 33
    # workgroups per frame of k_slab: every slab for small batches, fewer walking several slabs otherwise
    has(check(brick_lds=0, n=32, submitted=0), voxeliser="k_slab", slab_groups=19)
    has(check(brick_lds=0, n=64, submitted=0), voxeliser="k_slab", slab_groups=8)


def test_slab_emit(check):
    has(check(brick_lds=0, slab_emit=0), voxeliser="k_slab")
    has(check(brick_lds=0, n=127), voxeliser="k_slab")       # batches of 4-127 frames that do not take the frame kernel
    has(check(brick_lds=0, n=128), voxeliser="k_slab_emit")
    has(check(n=127), voxeliser="frame")


def test_device_tail(check):
    has(check(device_tail=0), tail="k_pack", dtail=0, clusterer="k_frame_lds_far", close_first=1, lean=1)
    has(check(dbg=1, **BATCH4), tail="k_pack", dtail=0)      # debug output
    has(check(n=3, submitted=0), tail="k_pack", dtail=0)     # batches of < 4 frames
    has(check(n=4, submitted=0), tail="k_tail_far", dtail=1)
    has(check(**UPDATING_BATCH), tail="k_pack", dtail=0)
    # the raycast role runs ahead of the device tail of a single map-updating scan
    has(check(auto_raycast=1, **SCAN), raycast_ahead=1)
    has(check(auto_raycast=1, device_tail=0, **SCAN), raycast_ahead=0)
    has(check(auto_raycast=1, dbg=1, **SCAN), raycast_ahead=0)
    has(check(auto_raycast=1), raycast_ahead=0)
