"""vofod_map_match at the shapes of tools/map_render_scans_bench.py: the three kernels of a call for 1 / 64 / 1024 / 4096 candidate
poses (lattices of vofod_pose_lattice around the scan's pose, one voxel and 0.01 rad apart), the C call on the host clock, look-ups
per second, and the chunk and burst tables - beside what a caller had before: k_map_render_scans with the same poses as views of
the same scan, up to 64 views, of a library built from the parent commit (--parent-lib; without it, of this tree's library).  The two
answer different questions - a ray walk per pixel and pose, a look-up per return and pose - so the figures stand side by side, no
ratio is asked of them.  Writes profiles/r31_map_match.txt (first line: the summary DESIGN.md quotes, then one JSON line per shape)
- or to --out.

OS1-128 at 0.25 m on bench.py's warmed map, then OS2-128 x 2048 at 0.1 m (--big 0 leaves it out); threshold = thresholds/new_obstacles.
The scan is the bench's frame 0 as a range image in device memory, stride 4.  Per figure: the median over --rounds calls of the
kernels' device times from the library's profiler (vofod_profile_read).  The tables are taken first (the chunk at 1024 and 4096 poses, the burst at 1024); the other
figures are then taken with the fastest chunk and burst of the tables set through VOFOD_MATCH_CHUNK / VOFOD_MATCH_BURST, and the
line says which they were.
A report, not a gate."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import vofod_amd  # noqa: E402
from vofod_amd import capi, synth  # noqa: E402
from vofod_amd.detector import ScanData, VoFOD, default_params, pose_lattice  # noqa: E402

F = np.float32
KERNELS = ("k_match_bits", "k_match_points", "k_match_score")
LATTICES = {1: ((1, 1, 1), 1), 64: ((4, 4, 4), 1), 1024: ((8, 8, 4), 4), 4096: ((16, 16, 4), 4)}
CHUNKS, BURSTS = (64, 128, 256, 512, 2048), (1, 2, 4, 8)


def prof(det):
    names, ms, calls = (C.c_char * (64 * 128))(), (C.c_double * 128)(), (C.c_uint64 * 128)()
    n = det.lib.profile_read(det.h, names, ms, calls, 128)
    return {names[64 * i : 64 * i + 64].split(b"\0", 1)[0].decode(): (float(ms[i]), int(calls[i])) for i in range(n)}


def older_library(path):
    """a library that may lack the newest entry points (the parent commit's): bound as far as it goes"""
    lib = capi.Library.__new__(capi.Library)
    try:
        lib.__init__(path, "vofod_")
    except ImportError:
        pass
    return lib


def stats(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 5), "spread": round((max(ms) - min(ms)) / med, 4) if med else 0.0}


def timed(det, names, call, args):
    """medians over the rounds: every kernel of `names` (one launch each per call) and the call on the host clock"""
    per, host = {k: [] for k in names}, []
    for r in range(args.warmup + args.rounds):
        det.lib.profile_enable(det.h, 1)
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        p = prof(det)
        det.lib.profile_enable(det.h, 0)
        assert sorted(p) == sorted(names) and all(c == 1 for _, c in p.values()), p
        if r >= args.warmup:
            host.append((t1 - t0) * 1e3)
            for k in names:
                per[k].append(p[k][0])
    return {**{k: stats(v) for k, v in per.items()}, "host_call": stats(host)}


def set_env(chunk, burst):
    for name, v in (("VOFOD_MATCH_CHUNK", chunk), ("VOFOD_MATCH_BURST", burst)):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)


def measure(args, sensor, voxel_size, warm_scans, pool, torch, dev, parent):
    lib = vofod_amd.library()
    h, w, vfov_deg, _ = synth.SENSORS[sensor]
    n = h * w

    def make(lb):
        sp, dp = default_params(lb)
        sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = voxel_size, w, h, 1
        sp.sensor_vfov = F(np.deg2rad(vfov_deg))
        return VoFOD(lb, sp, dp)

    det = make(lib)
    scene = synth.bench_scene()
    synth.warm_map(det, scene, sensor, warm_scans, pmap=pool.map)
    frame = synth.bench_frames(scene, sensor, 1, 0, pmap=pool.map)[0]
    tf = np.asarray(frame.tf, F)
    thr = float(det.dp.voxel_map__thresholds__new_obstacles)
    ref_lib, ref = (parent, make(parent)) if parent is not None else (lib, det)
    if parent is not None:
        ref.write_map(capi.MAP_VOXELS, det.read_map())
    rng = torch.from_numpy(np.ascontiguousarray(frame.scan.range, np.uint32).view(np.int32)).to(dev)
    scan = ScanData.range_image(rng.data_ptr(), w, h, memspace=capi.MEM_DEVICE)
    cs = scan.as_c()
    res = {"sensor": sensor, "voxel_size": voxel_size, "map": list(det.map_size), "bits_MB": round(det.n_voxels / 8 / 1e6, 1), "warm_scans": warm_scans, "threshold": thr,
           "reference": "parent" if parent is not None else "this tree", "poses": {}}

    def match_call(tfs, counts, best):
        t = np.ascontiguousarray(tfs, F).reshape(-1)

        def call():
            st = lib.map_match(det.h, C.byref(cs), capi.ptr(t), len(tfs), C.c_float(thr), capi.ptr(counts), C.byref(best))
            assert st == capi.OK, st

        return call

    def lattice(k):
        cnt, n_yaw = LATTICES[k]
        return pose_lattice(lib, tf, (voxel_size,) * 3, cnt, 0.01, n_yaw)

    # ---- the tables first: the chunk at 1024 and at 4096 poses, the burst at 1024 poses with the chunk that is fastest there
    res["chunk_table"], res["burst_table"] = {}, {}
    for k in (1024, 4096):
        tfs = lattice(k)
        counts, best = np.zeros((k, 4), np.uint32), C.c_int32(-1)
        res["chunk_table"][str(k)] = {}
        for c in CHUNKS:
            set_env(c, None)
            res["chunk_table"][str(k)][str(c)] = timed(det, KERNELS, match_call(tfs, counts, best), args)["k_match_score"]
    at = res["chunk_table"]["1024"]
    res["chunk"] = int(min(at, key=lambda c: at[c]["median_ms"]))
    tfs = lattice(1024)
    counts, best = np.zeros((1024, 4), np.uint32), C.c_int32(-1)
    for u in BURSTS:
        set_env(res["chunk"], u)
        res["burst_table"][str(u)] = timed(det, KERNELS, match_call(tfs, counts, best), args)["k_match_score"]
    res["burst"] = int(min(res["burst_table"], key=lambda u: res["burst_table"][u]["median_ms"]))
    set_env(res["chunk"], res["burst"])
    # ---- the call per candidate count, and the walk of the same poses beside it
    for k in LATTICES:
        tfs = lattice(k)
        counts, best = np.zeros((k, 4), np.uint32), C.c_int32(-1)
        per = timed(det, KERNELS, match_call(tfs, counts, best), args)
        n_live = n - int(counts[0, 0])
        assert (counts.sum(axis=1) == n).all() and (counts[:, 0] == counts[0, 0]).all()
        score_ms = per["k_match_score"]["median_ms"]
        per.update(n_live=n_live, best=int(best.value), occupied_best=int(counts[best.value, 3]),
                   lookups_per_s=round(n_live * k / (score_ms * 1e-3)) if score_ms else None,
                   us_per_pose=round(sum(per[x]["median_ms"] for x in KERNELS) * 1e3 / k, 4))
        nv = min(k, 64)
        arr = (capi.Scan * nv)(*[cs] * nv)
        tf_nv = np.ascontiguousarray(tfs[:nv], F).reshape(-1)
        vc = np.zeros((nv, 8), np.uint32)
        length = float(det.dp.raycast__max_distance)

        def walk():
            st = ref_lib.map_render_scans(ref.h, arr, capi.ptr(tf_nv), nv, C.c_float(thr), C.c_float(length), C.c_float(voxel_size), None, None, None, None, None, capi.ptr(vc), C.c_int32(capi.MEM_HOST))
            assert st == capi.OK, st

        wk = timed(ref, ("k_map_render_scans",), walk, args)
        per["walk"] = {"views": nv, **wk["k_map_render_scans"], "host_call": wk["host_call"], "us_per_pose": round(wk["k_map_render_scans"]["median_ms"] * 1e3 / nv, 3)}
        res["poses"][str(k)] = per
    set_env(None, None)
    det.close()
    if parent is not None:
        ref.close()
    return res


def summary(results):
    parts = []
    for r in results:
        bits = []
        for k, per in r["poses"].items():
            us = lambda name: per[name]["median_ms"] * 1e3
            wk = per["walk"]
            bits.append(f"{k} pose{'s' if k != '1' else ''}: `k_match_bits` {us('k_match_bits'):.1f} us, `k_match_points` {us('k_match_points'):.1f} us, `k_match_score` {us('k_match_score'):.1f} us, "
                        f"the C call {us('host_call'):.0f} us on the host clock, {per['lookups_per_s'] / 1e9:.2f} G look-ups/s, {per['us_per_pose']:.3f} us per pose; the walk "
                        f"(`k_map_render_scans` of the {r['reference']}'s library, {wk['views']} view{'s' if wk['views'] != 1 else ''}) {wk['median_ms'] * 1e3:.1f} us = {wk['us_per_pose']:.1f} us per pose "
                        f"(spread over its twelve calls {wk['spread'] * 100:.1f} %)")
        head = (f"{r['sensor']} at {r['voxel_size']} m ({r['map'][0]} x {r['map'][1]} x {r['map'][2]} voxels, bit image {r['bits_MB']} MB, warmed by {r['warm_scans']} scans), threshold {r['threshold']}, "
                f"{r['poses']['1']['n_live']} live returns, chunk {r['chunk']}, burst {r['burst']}: ")
        row = lambda t: " / ".join(f"{v['median_ms'] * 1e3:.1f}" for v in t.values())
        tab = ("; `k_match_score` by chunk " + " / ".join(map(str, CHUNKS)) + ": " + "; ".join(f"at {k} poses {row(t)} us" for k, t in r["chunk_table"].items()) + "; by burst "
               + " / ".join(r["burst_table"]) + f" at 1024 poses and chunk {r['chunk']}: {row(r['burst_table'])} us")
        parts.append(head + "; ".join(bits) + tab)
    return "measured: " + ". ".join(parts) + ".\n" + "".join(json.dumps(r) + "\n" for r in results)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--map-warm-scans", type=int, default=96)
    ap.add_argument("--big", type=int, default=1, help="also OS2-128 x 2048 at 0.1 m")
    ap.add_argument("--big-warm-scans", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libvofod_hip.so built from the parent commit: its k_map_render_scans is the reference")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r31_map_match.txt"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("map_match_bench.py needs a GPU: no timing without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    parent = older_library(args.parent_lib) if args.parent_lib else None
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    results = [measure(args, "os1-128", 0.25, args.map_warm_scans, pool, torch, dev, parent)]
    if args.big:
        results.append(measure(args, "os2-128x2048", 0.1, args.big_warm_scans, pool, torch, dev, parent))
    pool.shutdown()
    text = summary(results)
    if Path(args.out).exists():
        text += "".join(l + "\n" for l in Path(args.out).read_text().splitlines() if l.startswith(("resources: ", "bench: ", "mutations: ", "suite: ")))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
