"""World store (include/vofod.h WORLD STORE): what vofod_map_shift costs with the store off and on, on a warmed map, at 0.25 m
(OS1-128 defaults) and 0.1 m (OS2-128 x 2048), for s = (1, 0, 0), (64, 0, 0) and (64, 64, 8).  Writes <out>/r23_world_store.json
and <out>/r23_world_store.txt (kept as profiles/r23_world_store.*).

Two handles in one process hold the same warmed maps, one with the store enabled; their calls are interleaved - off, on, off, on -
each shift followed by its inverse so that the offset does not wander.  Every call is timed as a whole, with the wall clock and
between two HIP events recorded round it (the call ends with its own hipStreamSynchronize, so both bracket the same work);
medians over 2 * REPS calls.  The first call of a case with the store on allocates that case's tiles and is reported on its own
(cold); the medians are the calls after it, whose tiles exist.  The new kernels' own times come from a further pass with the
library's HIP-event profiler on (vofod_profile_read).
--parent-lib PATH: the same store-off calls with another build of the library (the parent commit's), in child processes of this
tool on the same device, REPEATS times over and in turns with this build, so that the run-to-run spread of both is known.

YARDSTICKS (recorded, judged in DESIGN.md 5.15): store off against the parent's call, inside the parent's spread; store on minus
store off against the byte model - rim voxels x 12 B (mark reads 4, put reads 4, get reads or writes 4) plus new tiles x 2 KiB -
and the launch floors of four small kernels; on minus off at (1, 0, 0) below on minus off at (64, 0, 0), or the walk follows the
map and not the rim."""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import vofod_amd  # noqa: E402
from vofod_amd import capi, synth  # noqa: E402
from vofod_amd.detector import VoFOD, default_params  # noqa: E402

REPS = 6      # there and back: 12 timed calls per case
REPEATS = 3   # runs of the child process per library
SHIFTS = ((1, 0, 0), (64, 0, 0), (64, 64, 8))
CONFIGS = {"025": ("0.25 m", "os1-128", 0.25), "01": ("0.1 m", "os2-128x2048", 0.1)}
MARGIN = (72, 72, 16)
MAX_TILES = 400_000  # 0.8 GB of pool: both rims of the largest shift at 0.1 m with every voxel known
WORLD_KERNELS = ("k_world_mark", "k_world_claim", "k_world_put", "k_world_get")
MAPS = (capi.MAP_VOXELS, capi.MAP_FLAGS, capi.MAP_RAYCAST)
med = statistics.median


def make(lib, sensor, vs):
    h, w, vfov_deg, _ = synth.SENSORS[sensor]
    sp, dp = default_params(lib)
    sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = vs, w, h, 1
    sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
    return VoFOD(lib, sp, dp)


def prof(det):
    names, ms, calls = (C.c_char * (64 * 128))(), (C.c_double * 128)(), (C.c_uint64 * 128)()
    n = det.lib.profile_read(det.h, names, ms, calls, 128)
    return {names[64 * i : 64 * i + 64].split(b"\0", 1)[0].decode(): (float(ms[i]), int(calls[i])) for i in range(n)}


class Events:
    """two HIP events of the runtime the library was loaded with"""

    def __init__(self):
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.rt = rt = C.CDLL(path)
        for name, args in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]), ("hipEventSynchronize", [C.c_void_p]),
                           ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
            getattr(rt, name).argtypes, getattr(rt, name).restype = args, C.c_int
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        assert rt.hipEventCreate(C.byref(self.e0)) == 0 and rt.hipEventCreate(C.byref(self.e1)) == 0

    def timed(self, fn):
        """(wall ms, event ms) of fn()"""
        rt = self.rt
        rt.hipEventRecord(self.e0, None)
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        rt.hipEventRecord(self.e1, None)
        rt.hipEventSynchronize(self.e1)
        ms = C.c_float(0)
        assert rt.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return wall, float(ms.value)


def offset_of(base, k, vs):
    return tuple(float(np.float32(b + int(kk) * vs)) for b, kk in zip(base, k))


class Mover:
    def __init__(self, det, vs):
        self.det, self.vs = det, vs
        self.base = tuple(float(v) for v in det.sp.oparea_offset)
        self.k = np.zeros(3, dtype=np.int64)

    def step(self, s):
        self.k += np.array(s)
        self.det.map_shift(s, offset_of(self.base, self.k, self.vs))


def rim_voxels(S, s):
    keep = 1
    for n, a in zip(S, s):
        keep *= max(n - abs(a), 0)
    return int(np.prod(S)) - keep


def warmed(lib, sensor, vs, n_scans):
    det = make(lib, sensor, vs)
    synth.warm_map(det, synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=0), sensor, n_scans)
    return det


def time_cases(movers, ev, reps):
    """{shift: {name: {"cold": (wall, event), "wall": [...], "event": [...]}}}; the movers' calls interleaved"""
    out = {}
    for s in SHIFTS:
        back = tuple(-v for v in s)
        rec = {name: {"wall": [], "event": []} for name in movers}
        for name, m in movers.items():  # the first pair: with the store on it allocates the case's tiles
            rec[name]["cold"] = ev.timed(lambda: m.step(s))
            m.step(back)
        for r in range(2 * reps):
            step = s if r % 2 == 0 else back
            for name, m in movers.items():
                w, e = ev.timed(lambda: m.step(step))
                rec[name]["wall"].append(w)
                rec[name]["event"].append(e)
        out[s] = rec
    return out


def run_config(lib, key, n_scans, reps):
    name, sensor, vs = CONFIGS[key]
    ev = Events()
    off = warmed(lib, sensor, vs, n_scans)
    on = make(lib, sensor, vs)
    for m in MAPS:
        on.write_map(m, off.read_map(m))
    on.load_apriori(np.zeros((0, 3), dtype=np.float32))
    known = int((off.read_map(capi.MAP_VOXELS) != np.float32(off.sp.score_init)).sum())
    on.world_enable(MARGIN, MARGIN, MAX_TILES)
    movers = {"off": Mover(off, vs), "on": Mover(on, vs)}
    for m in movers.values():  # the spare buffer
        m.step((4, 0, 0))
        m.step((-4, 0, 0))
    S = off.map_size
    cases = []
    timed = time_cases(movers, ev, reps)
    # the kernels' own times, profiler on: one more pair per shift on the handle with the store
    on.lib.profile_enable(on.h, 1)
    for s in SHIFTS:
        info0 = on.world_info()
        prof(on)
        movers["on"].step(s)
        p = prof(on)
        movers["on"].step(tuple(-v for v in s))
        rec = timed[s]
        info = on.world_info()
        d = {k: round(med(rec["on"][k]) - med(rec["off"][k]), 4) for k in ("wall", "event")}
        rim = rim_voxels(S, s)
        cases.append({
            "shift": list(s), "rim_voxels": rim, "rim_share": round(rim / off.n_voxels, 5),
            "off": {"wall_ms_median": round(med(rec["off"]["wall"]), 4), "event_ms_median": round(med(rec["off"]["event"]), 4), "event_ms_min": round(min(rec["off"]["event"]), 4),
                    "event_ms_max": round(max(rec["off"]["event"]), 4)},
            "on": {"wall_ms_median": round(med(rec["on"]["wall"]), 4), "event_ms_median": round(med(rec["on"]["event"]), 4), "cold_first_call_event_ms": round(rec["on"]["cold"][1], 4)},
            "on_minus_off_ms": d,
            "byte_model": {"rim_bytes": 12 * rim, "ms_at_4_TBs": round(12 * rim / 4e12 * 1e3, 4)},
            "kernels_ms": {k: round(p.get(k, (0.0, 0))[0], 4) for k in WORLD_KERNELS + ("k_map_shift",)},
            "launches": {k: p.get(k, (0.0, 0))[1] for k in WORLD_KERNELS + ("k_map_shift",)},
            "tiles_used_after": int(info.tiles_used), "tiles_used_before_profiled_call": int(info0.tiles_used), "shifts_short_of_tiles": int(info.shifts_short_of_tiles),
            "voxels_forgotten": int(info.voxels_forgotten),
        })
    on.lib.profile_enable(on.h, 0)
    res = {"config": name, "sensor": sensor, "voxel_size": vs, "M": off.n_voxels, "map_size": list(S), "known_voxels": known, "warm_scans": n_scans, "calls_per_median": 2 * reps, "margins": list(MARGIN),
           "max_tiles": MAX_TILES, "cases": cases}
    on.close()
    off.close()
    return res


def run_off_only(lib, key, n_scans, reps):
    """the store-off calls alone (the parent's library has no store): event and wall medians per shift"""
    name, sensor, vs = CONFIGS[key]
    ev = Events()
    det = warmed(lib, sensor, vs, n_scans)
    m = Mover(det, vs)
    m.step((4, 0, 0))
    m.step((-4, 0, 0))
    out = {}
    for s in SHIFTS:
        back = tuple(-v for v in s)
        m.step(s)
        m.step(back)
        t = [ev.timed(lambda: m.step(s if r % 2 == 0 else back)) for r in range(2 * reps)]
        out[str(list(s))] = {"wall_ms_median": round(med(w for w, _ in t), 4), "event_ms_median": round(med(e for _, e in t), 4)}
    det.close()
    return out


def text(res):
    lines = ["vofod_map_shift with the world store off and on (tools/world_store_bench.py, one MI355X)",
             "whole call between two HIP events (the wall clock beside it); medians; store off and on interleaved in one process on a warmed map", ""]
    for c in res["configs"]:
        sx, sy, sz = c["map_size"]
        lines.append(f"{c['config']}: {c['sensor']}, map {sx} x {sy} x {sz}, M = {c['M']:,} voxels, {c['known_voxels']:,} of them differ from init, {c['calls_per_median']} calls per median")
        for k in c["cases"]:
            km, off, on = k["kernels_ms"], k["off"], k["on"]
            lines += [
                f"  s = {tuple(k['shift'])}: rim {k['rim_voxels']:,} voxels ({100 * k['rim_share']:.3f} % of the map), tiles used afterwards {k['tiles_used_after']:,}",
                f"    store off   {off['event_ms_median']:9.4f} ms  (wall {off['wall_ms_median']:.4f}; events min {off['event_ms_min']:.4f} max {off['event_ms_max']:.4f})",
                f"    store on    {on['event_ms_median']:9.4f} ms  (wall {on['wall_ms_median']:.4f}; first call, allocating the tiles: {on['cold_first_call_event_ms']:.4f})",
                f"    on - off    {k['on_minus_off_ms']['event']:9.4f} ms  byte model: {k['byte_model']['rim_bytes']:,} B = {k['byte_model']['ms_at_4_TBs']:.4f} ms at 4 TB/s, plus four launches",
                f"    kernels     mark {km['k_world_mark']:.4f}  claim {km['k_world_claim']:.4f}  put {km['k_world_put']:.4f}  get {km['k_world_get']:.4f}  3 x k_map_shift {km['k_map_shift']:.4f} ms (profiler on)",
            ]
            par = c.get("parent")
            if par:
                key = str(k["shift"])
                theirs = [r[key]["event_ms_median"] for r in par["runs"]]
                ours = [r[key]["event_ms_median"] for r in par["own_runs"]]
                lines.append(f"    parent      {med(theirs):9.4f} ms  (its {len(theirs)} runs: {', '.join(f'{v:.4f}' for v in theirs)}); this build, store off, alone in a process: {', '.join(f'{v:.4f}' for v in ours)}")
        lines.append("")
    return "\n".join(lines) + "\n"


def load_library(path):
    """capi.Library on a build that may predate entry points the header declares today (the parent commit's)"""
    have = [n for n in capi.declared_entry_points() if hasattr(C.CDLL(str(path)), "vofod_" + n)]
    declared = capi.declared_entry_points
    capi.declared_entry_points = lambda: have
    try:
        return capi.Library(path, "vofod_")
    finally:
        capi.declared_entry_points = declared


def child(lib_path, key, n_scans, reps):
    print(f"[world_store_bench] child process: {lib_path} at {CONFIGS[key][0]}", file=sys.stderr, flush=True)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), "--role", "off-only", "--lib", str(lib_path), "--only", key, "--warm-scans", str(n_scans), "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=900)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=tuple(CONFIGS), default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles"), help="directory of r23_world_store.json / .txt")
    ap.add_argument("--warm-scans", type=int, default=4)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--parent-lib", default=None, help="libvofod_hip.so of the parent commit: its store-off calls are timed in child processes")
    ap.add_argument("--role", choices=("main", "off-only"), default="main")
    ap.add_argument("--lib", default=None, help="(off-only) the library to time")
    args = ap.parse_args()
    keys = [args.only] if args.only else list(CONFIGS)
    if args.role == "off-only":
        lib = load_library(args.lib) if args.lib else vofod_amd.library()
        print(json.dumps(run_off_only(lib, keys[0], args.warm_scans, args.reps)))
        return
    lib = vofod_amd.library()
    res = {"tool": "world_store_bench", "configs": []}
    for key in keys:
        print(f"[world_store_bench] {CONFIGS[key][0]}: store off and on", file=sys.stderr, flush=True)
        c = run_config(lib, key, args.warm_scans, args.reps)
        if args.parent_lib:
            c["parent"] = {"runs": [], "own_runs": []}
            for _ in range(REPEATS):  # parent, this build, parent, ...: a drift of the box over the minutes falls on both
                c["parent"]["runs"].append(child(args.parent_lib, key, args.warm_scans, args.reps))
                c["parent"]["own_runs"].append(child(vofod_amd.LIB_PATH, key, args.warm_scans, args.reps))
        res["configs"].append(c)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "r23_world_store.json").write_text(json.dumps(res) + "\n")
    (out / "r23_world_store.txt").write_text(text(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
