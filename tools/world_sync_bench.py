"""World snapshots (include/vofod.h WORLD SNAPSHOTS): what vofod_world_export and vofod_world_apply cost, full and delta, on the warmed
walks of tools/world_store_bench.py at 0.25 m (OS1-128 defaults) and 0.1 m (OS2-128 x 2048).  Writes <out>/r25_world_sync.json and
<out>/r25_world_sync.txt (kept as profiles/r25_world_sync.*).

An owner with the store enabled walks world_store_bench's shifts there and back, so that its tiles exist; a follower with the same
margins applies what the owner exports.  Records travel through a device buffer (VOFOD_MEM_DEVICE on both sides: no host copy in
the times).  Every call is timed as a whole between two HIP events, the wall clock beside it; medians of CALLS calls:
  full      export of every allocated tile, and its apply on the follower (which empties its store first);
  delta     after a shift of (64, 0, 0) whose leaving slab was given new values in its known voxels: export, and its apply (every
            timed delta follows the forward shift; the delta behind the shift back, whose leaving slab entered as init, has its own line);
  unchanged a delta of a store nobody wrote: the compare pass alone, 128 bytes.
The kernels' own times come from a further pass with the library's HIP-event profiler on.  Each time stands beside its byte model:
  full export   directory 2 x 4 B x tiles of the box + carried tiles x 2 KiB x 3 (pool read, shadow written, record written)
  delta export  directory as above + allocated tiles x 2 KiB x 2 (pool and shadow read) + carried tiles x 2 KiB x 3
  apply         carried tiles x 2 KiB x 2 (record read, pool written) + the index list twice
--parent-lib PATH: vofod_map_shift with the store ON with another build of the library (the parent commit's) and with this one, in
child processes on the same device, REPEATS times over and in turns, so that the run-to-run spread of both is known: the existing
store kernels and what a shift launches are the parent's, so the two must agree inside that spread."""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import vofod_amd  # noqa: E402
import world_store_bench as wsb  # noqa: E402
from vofod_amd import capi, mapsync  # noqa: E402

CALLS = 12
REPEATS = 3
DELTA_SHIFT = (64, 0, 0)
SYNC_KERNELS = ("k_world_select", "k_gscan_a", "k_gscan_b", "k_gscan_c", "k_world_emit", "k_world_check", "k_world_scatter")
med = statistics.median


class DeviceBuffer:
    def __init__(self, rt, nbytes):
        rt.hipMalloc.argtypes, rt.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        self.rt, self.p, self.n = rt, C.c_void_p(), nbytes
        assert rt.hipMalloc(C.byref(self.p), nbytes) == 0 and self.p.value % 16 == 0

    def free(self):
        assert self.rt.hipFree(self.p) == 0


def stats(ts):
    return {"wall_ms_median": round(med(w for w, _ in ts), 4), "event_ms_median": round(med(e for _, e in ts), 4), "event_ms_min": round(min(e for _, e in ts), 4),
            "event_ms_max": round(max(e for _, e in ts), 4)}


def run_config(lib, key, n_scans):
    name, sensor, vs = wsb.CONFIGS[key]
    ev = wsb.Events()
    owner = wsb.warmed(lib, sensor, vs, n_scans)
    follower = wsb.make(lib, sensor, vs)
    for d in (owner, follower):
        d.world_enable(wsb.MARGIN, wsb.MARGIN, wsb.MAX_TILES)
    mover = wsb.Mover(owner, vs)
    for s in wsb.SHIFTS:  # the warmed walk: every rim of world_store_bench has left once, its tiles exist
        mover.step(s)
        mover.step(tuple(-v for v in s))
    info = owner.world_info()
    used = int(info.tiles_used)
    n_dir = int(np.prod([-(-(int(h) - int(l)) // 8) for l, h in zip(info.box_lo, info.box_hi)]))
    buf = DeviceBuffer(ev.rt, mapsync.world_nbytes(used + 4096))
    sizes = {}

    def export(kind):
        sizes[kind] = owner.world_export(kind, device=(buf.p.value, buf.n))

    def apply(kind):
        follower.world_apply((buf.p.value, sizes[kind]))

    F, D = capi.SNAPSHOT_FULL, capi.SNAPSHOT_DELTA
    export(F)  # not recorded: the first export allocates the shadow pool and the scratch, the first apply the follower's
    apply(F)
    t = {k: [] for k in ("full_export", "full_apply", "delta_export", "delta_apply", "back_export", "back_apply", "unchanged_export", "unchanged_apply")}
    for _ in range(CALLS):
        t["full_export"].append(ev.timed(lambda: export(F)))
        t["full_apply"].append(ev.timed(lambda: apply(F)))
    carried = []

    def touch(r):
        """new values in the known voxels of the slabs the next shift pushes out, so that the delta has tiles to carry"""
        m = owner.read_map(capi.MAP_VOXELS)
        for sl in (np.s_[:, :, : DELTA_SHIFT[0]], np.s_[:, :, -DELTA_SHIFT[0]:]):
            m[sl] = np.where(m[sl] != np.float32(owner.sp.score_init), np.float32(-1.0 - r), m[sl])
        owner.write_map(capi.MAP_VOXELS, m)

    back_carried = []
    for r in range(CALLS):  # every timed delta follows the forward shift, whose leaving slab holds the warmed map's known voxels
        touch(r)
        mover.step(DELTA_SHIFT)
        t["delta_export"].append(ev.timed(lambda: export(D)))
        carried.append((sizes[D] - 128) // 2052)
        t["delta_apply"].append(ev.timed(lambda: apply(D)))
        mover.step(tuple(-v for v in DELTA_SHIFT))  # the way back pushes out a slab that entered as init: its delta is on its own line
        t["back_export"].append(ev.timed(lambda: export(D)))
        back_carried.append((sizes[D] - 128) // 2052)
        t["back_apply"].append(ev.timed(lambda: apply(D)))
    assert min(carried) > 0, carried
    for _ in range(CALLS):
        t["unchanged_export"].append(ev.timed(lambda: export(D)))
        assert sizes[D] == 128
        t["unchanged_apply"].append(ev.timed(lambda: apply(D)))
    used = int(owner.world_info().tiles_used)
    export(F)
    n_full = (sizes[F] - 128) // 2052
    apply(F)
    # the kernels' own times
    kern = {}
    for d in (owner, follower):
        d.lib.profile_enable(d.h, 1)
        wsb.prof(d)
    for label, kind, move in (("full", F, False), ("delta", D, True), ("unchanged", D, False)):
        if move:
            touch(CALLS)
            mover.step(DELTA_SHIFT)
            wsb.prof(owner)
        export(kind)
        apply(kind)
        p = {**wsb.prof(owner), **wsb.prof(follower)}
        kern[label] = {k: [round(p.get(k, (0.0, 0))[0], 4), p.get(k, (0.0, 0))[1]] for k in SYNC_KERNELS}
        kern[label]["carried_tiles"] = (sizes[kind] - 128) // 2052
    for d in (owner, follower):
        d.lib.profile_enable(d.h, 0)
    n_delta = int(med(carried))
    tile = 2048
    model = {"full_export_bytes": 8 * n_dir + 3 * tile * n_full, "delta_export_bytes": 8 * n_dir + 2 * tile * used + 3 * tile * n_delta, "unchanged_export_bytes": 8 * n_dir + 2 * tile * used,
             "full_apply_bytes": 2 * tile * n_full + 8 * n_full, "delta_apply_bytes": 2 * tile * n_delta + 8 * n_delta}
    res = {"config": name, "sensor": sensor, "voxel_size": vs, "map_size": list(owner.map_size), "margins": list(wsb.MARGIN), "max_tiles": wsb.MAX_TILES, "directory_tiles": n_dir, "tiles_used": used,
           "full_tiles": n_full, "full_bytes": mapsync.world_nbytes(n_full), "delta_tiles_median": n_delta, "delta_tiles": carried, "delta_tiles_on_the_way_back": back_carried, "calls_per_median": CALLS, "warm_scans": n_scans,
           "times": {k: stats(v) for k, v in t.items()}, "byte_model": model, "ms_at_4_TBs": {k[:-6]: round(v / 4e12 * 1e3, 4) for k, v in model.items()}, "kernels_ms_calls": kern}
    buf.free()
    owner.close()
    follower.close()
    return res


def run_shift_on(lib, key, n_scans, reps):
    """vofod_map_shift with the store on, alone in a process (the parent's library has the store too): event and wall medians per shift"""
    name, sensor, vs = wsb.CONFIGS[key]
    ev = wsb.Events()
    det = wsb.warmed(lib, sensor, vs, n_scans)
    det.world_enable(wsb.MARGIN, wsb.MARGIN, wsb.MAX_TILES)
    m = wsb.Mover(det, vs)
    m.step((4, 0, 0))
    m.step((-4, 0, 0))
    out = {}
    for s in wsb.SHIFTS:
        back = tuple(-v for v in s)
        m.step(s)
        m.step(back)
        ts = [ev.timed(lambda: m.step(s if r % 2 == 0 else back)) for r in range(2 * reps)]
        out[str(list(s))] = {"wall_ms_median": round(med(w for w, _ in ts), 4), "event_ms_median": round(med(e for _, e in ts), 4)}
    det.close()
    return out


def child(lib_path, key, n_scans, reps):
    print(f"[world_sync_bench] child process: {lib_path} at {wsb.CONFIGS[key][0]}", file=sys.stderr, flush=True)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), "--role", "shift-on", "--lib", str(lib_path), "--only", key, "--warm-scans", str(n_scans), "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=900)
    return json.loads(r.stdout.strip().splitlines()[-1])


def headline(res):
    """the record's first line: what DESIGN.md quotes (tools/assemble_design.py)"""
    parts = []
    for c in res["configs"]:
        t, at = c["times"], c["ms_at_4_TBs"]
        parts.append(f"at {c['config']} ({c['sensor']}, directory {c['directory_tiles']:,} tiles, {c['tiles_used']:,} allocated) a full snapshot of {c['full_tiles']:,} tiles "
                     f"({c['full_bytes'] / 1e6:.1f} MB) exports in {t['full_export']['event_ms_median']:.4f} ms (byte model {at['full_export']:.4f} ms at 4 TB/s) and applies in "
                     f"{t['full_apply']['event_ms_median']:.4f} ms ({at['full_apply']:.4f}); a delta of {c['delta_tiles_median']:,} tiles (each of the {c['calls_per_median']} timed deltas carried {min(c['delta_tiles']):,}-{max(c['delta_tiles']):,}) after a shift of {DELTA_SHIFT} exports in "
                     f"{t['delta_export']['event_ms_median']:.4f} ms ({at['delta_export']:.4f}) and applies in {t['delta_apply']['event_ms_median']:.4f} ms ({at['delta_apply']:.4f}); the delta of an "
                     f"unchanged store - the compare pass alone, 128 bytes - takes {t['unchanged_export']['event_ms_median']:.4f} ms ({at['unchanged_export']:.4f})")
    return "measured: " + "; ".join(parts) + "."


def text(res):
    lines = [headline(res), "",
             "vofod_world_export / vofod_world_apply on the warmed walks of tools/world_store_bench.py (tools/world_sync_bench.py, one MI355X)",
             "whole call between two HIP events (the wall clock beside it), records in device memory on both sides; medians", ""]
    for c in res["configs"]:
        sx, sy, sz = c["map_size"]
        t, m, at = c["times"], c["byte_model"], c["ms_at_4_TBs"]
        lines.append(f"{c['config']}: {c['sensor']}, map {sx} x {sy} x {sz}, directory {c['directory_tiles']:,} tiles, {c['tiles_used']:,} allocated, {c['calls_per_median']} calls per median")
        for label, what, nt in (("full", "full", c["full_tiles"]), ("delta", "delta", c["delta_tiles_median"]), ("unchanged", "unchanged", 0)):
            e, a = t[f"{what}_export"], t[f"{what}_apply"]
            lines.append(f"  {label:9s} {nt:,} tiles carried ({mapsync.world_nbytes(nt):,} B)")
            lines.append(f"    export    {e['event_ms_median']:9.4f} ms  (wall {e['wall_ms_median']:.4f}; events min {e['event_ms_min']:.4f} max {e['event_ms_max']:.4f})  byte model: "
                         f"{m[what + '_export_bytes']:,} B = {at[what + '_export']:.4f} ms at 4 TB/s")
            am = f"  byte model: {m[what + '_apply_bytes']:,} B = {at[what + '_apply']:.4f} ms at 4 TB/s" if what != "unchanged" else ""
            lines.append(f"    apply     {a['event_ms_median']:9.4f} ms  (wall {a['wall_ms_median']:.4f}; events min {a['event_ms_min']:.4f} max {a['event_ms_max']:.4f}){am}")
            k = c["kernels_ms_calls"][label]
            lines.append("    kernels   " + "  ".join(f"{n[2:]} {k[n][0]:.4f}" + (f" x{k[n][1]}" if k[n][1] != 1 else "") for n in SYNC_KERNELS) + f" ms (profiler on, {k['carried_tiles']:,} tiles carried)")
        bk = c["delta_tiles_on_the_way_back"]
        lines.append(f"  the delta behind the shift back ({min(bk):,}-{max(bk):,} tiles carried): export {t['back_export']['event_ms_median']:.4f} ms, apply {t['back_apply']['event_ms_median']:.4f} ms")
        par = c.get("parent")
        if par:
            for s in wsb.SHIFTS:
                key = str(list(s))
                theirs = [r[key]["event_ms_median"] for r in par["runs"]]
                ours = [r[key]["event_ms_median"] for r in par["own_runs"]]
                lines.append(f"  vofod_map_shift, store on, s = {s}: parent {med(theirs):.4f} ms (its {len(theirs)} runs: {', '.join(f'{v:.4f}' for v in theirs)}); this build {med(ours):.4f} ms "
                             f"({', '.join(f'{v:.4f}' for v in ours)})")
        lines.append("")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=tuple(wsb.CONFIGS), default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles"), help="directory of r25_world_sync.json / .txt")
    ap.add_argument("--warm-scans", type=int, default=4)
    ap.add_argument("--reps", type=int, default=wsb.REPS)
    ap.add_argument("--parent-lib", default=None, help="libvofod_hip.so of the parent commit: its store-on shifts are timed in child processes, in turns with this build's")
    ap.add_argument("--role", choices=("main", "shift-on"), default="main")
    ap.add_argument("--lib", default=None, help="(shift-on) the library to time")
    args = ap.parse_args()
    keys = [args.only] if args.only else list(wsb.CONFIGS)
    if args.role == "shift-on":
        lib = wsb.load_library(args.lib) if args.lib else vofod_amd.library()
        print(json.dumps(run_shift_on(lib, keys[0], args.warm_scans, args.reps)))
        return
    lib = vofod_amd.library()
    res = {"tool": "world_sync_bench", "configs": []}
    for key in keys:
        print(f"[world_sync_bench] {wsb.CONFIGS[key][0]}: export and apply", file=sys.stderr, flush=True)
        c = run_config(lib, key, args.warm_scans)
        if args.parent_lib:
            c["parent"] = {"runs": [], "own_runs": []}
            for _ in range(REPEATS):  # parent, this build, parent, ...: a drift of the box over the minutes falls on both
                c["parent"]["runs"].append(child(args.parent_lib, key, args.warm_scans, args.reps))
                c["parent"]["own_runs"].append(child(vofod_amd.LIB_PATH, key, args.warm_scans, args.reps))
        res["configs"].append(c)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "r25_world_sync.json").write_text(json.dumps(res) + "\n")
    (out / "r25_world_sync.txt").write_text(text(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
