"""vofod_map_distance and vofod_map_match_field at the shapes of tools/map_match_bench.py.  The distance: the four kernels of a call
(k_match_bits, k_dist_x, k_dist_y, k_dist_z) for radii 4 / 8 / 16 / 64 / 255 into a device buffer, and the C call on the host clock
- beside what a caller had before: vofod_read_map plus scipy.ndimage.distance_transform_edt on the host, timed once per map.  Both
numbers are stated, no ratio is asked of them.  The field match: k_match_field beside k_match_score of the same library for 1 / 64
/ 1024 / 4096 candidate poses (the same lattices, the field of radius 8 in device memory), and k_match_field by chunk and by burst.
With --parent-lib (a libvofod_hip.so built from the parent commit, as tools/map_match_bench.py takes one) the field-match table is
taken from that library too, on the same map, field, scan and poses, the parent before this tree at every candidate count.
Writes profiles/r32_map_distance.txt (first line: the summary DESIGN.md quotes, then one JSON line per shape) - or to --out.

OS1-128 at 0.25 m on bench.py's warmed map, then OS2-128 x 2048 at 0.1 m (--big 0 leaves it out); threshold = thresholds/new_obstacles.
Per figure: the median over --rounds calls of the kernels' device times from the library's profiler (vofod_profile_read); a call
that takes longer than --slow-ms is measured over three rounds.
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
sys.path.insert(0, str(ROOT / "tools"))

import vofod_amd  # noqa: E402
from map_match_bench import LATTICES, older_library, prof, set_env, stats  # noqa: E402
from vofod_amd import capi, synth  # noqa: E402
from vofod_amd.detector import ScanData, VoFOD, default_params, pose_lattice  # noqa: E402

F = np.float32
DIST_KERNELS = ("k_match_bits", "k_dist_x", "k_dist_y", "k_dist_z")
FIELD_KERNELS = ("k_match_points", "k_match_field")
SCORE_KERNELS = ("k_match_bits", "k_match_points", "k_match_score")
RADII = (4, 8, 16, 64, 255)
CHUNKS, BURSTS = (64, 128, 256), (1, 2, 4, 8)
FIELD_RADIUS = 8


def timed(det, names, call, args):
    """medians over the rounds: every kernel of `names` (one launch each per call) and the call on the host clock"""
    per, host = {k: [] for k in names}, []
    warmup, rounds, r = args.warmup, args.rounds, 0
    while r < warmup + rounds:
        det.lib.profile_enable(det.h, 1)
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        p = prof(det)
        det.lib.profile_enable(det.h, 0)
        assert sorted(p) == sorted(names) and all(c == 1 for _, c in p.values()), p
        if r == 0 and (t1 - t0) * 1e3 > args.slow_ms:
            warmup, rounds = 1, 3
        if r >= warmup:
            host.append((t1 - t0) * 1e3)
            for k in names:
                per[k].append(p[k][0])
        r += 1
    print(f"[map_distance_bench] {' + '.join(names)}: {statistics.median(host):.3f} ms per call", file=sys.stderr, flush=True)  # (progress: the long shapes say they are alive)
    return {**{k: stats(v) for k, v in per.items()}, "host_call": stats(host), "rounds": rounds}


def measure(args, sensor, voxel_size, warm_scans, pool, torch, dev, parent=None):
    lib = vofod_amd.library()
    h, w, vfov_deg, _ = synth.SENSORS[sensor]
    n_px = h * w

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
    n = det.n_voxels
    field = torch.zeros(n, dtype=torch.int16, device=dev)
    res = {"sensor": sensor, "voxel_size": voxel_size, "map": list(det.map_size), "field_MB": round(2 * n / 1e6, 1), "warm_scans": warm_scans, "threshold": thr, "radii": {}, "poses": {}}

    # ---- the distance by radius, into device memory
    def distance_call(R):
        def call():
            st = lib.map_distance(det.h, C.c_float(thr), R, C.c_void_p(field.data_ptr()), n, capi.MEM_DEVICE)
            assert st == capi.OK, st

        return call

    for R in RADII:
        per = timed(det, DIST_KERNELS, distance_call(R), args)
        per["kernels_ms"] = round(sum(per[k]["median_ms"] for k in DIST_KERNELS), 5)
        res["radii"][str(R)] = per
    # ---- what a caller had before: the map read back and scipy's transform on the host, once
    if n <= args.host_edt_max_voxels:
        from scipy import ndimage

        print("[map_distance_bench] the host transform", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        m = det.read_map()
        t1 = time.perf_counter()
        with np.errstate(invalid="ignore"):
            free = ~(m > F(thr))
        edt = ndimage.distance_transform_edt(free) if not free.all() else None
        t2 = time.perf_counter()
        res["host"] = {"read_map_ms": round((t1 - t0) * 1e3, 1), "edt_ms": round((t2 - t1) * 1e3, 1), "occupied": int((~free).sum())}
        if edt is not None:  # (and the device's field is that transform, where the clamp does not bite)
            distance_call(255)()
            got = field.cpu().numpy().view(np.uint16).reshape(m.shape)
            assert (got == np.minimum(np.rint(edt**2), 255 * 255).astype(np.uint16)).all()
        del m, free, edt
    # ---- the field match beside the count: the field of radius 8 in device memory
    distance_call(FIELD_RADIUS)()
    rng = torch.from_numpy(np.ascontiguousarray(frame.scan.range, np.uint32).view(np.int32)).to(dev)
    cs = ScanData.range_image(rng.data_ptr(), w, h, memspace=capi.MEM_DEVICE).as_c()

    def lattice(k):
        cnt, n_yaw = LATTICES[k]
        return pose_lattice(lib, tf, (voxel_size,) * 3, cnt, 0.01, n_yaw)

    def field_call(tfs, counts, cost, best, lib=lib, det=det):
        t = np.ascontiguousarray(tfs, F).reshape(-1)

        def call():
            st = lib.map_match_field(det.h, C.byref(cs), capi.ptr(t), len(tfs), C.c_void_p(field.data_ptr()), n, capi.MEM_DEVICE, FIELD_RADIUS, FIELD_RADIUS * FIELD_RADIUS, capi.ptr(counts),
                                     capi.ptr(cost), C.byref(best))
            assert st == capi.OK, st

        return call

    def score_call(tfs, counts, best, lib=lib, det=det):
        t = np.ascontiguousarray(tfs, F).reshape(-1)

        def call():
            st = lib.map_match(det.h, C.byref(cs), capi.ptr(t), len(tfs), C.c_float(thr), capi.ptr(counts), C.byref(best))
            assert st == capi.OK, st

        return call

    res["chunk_table"], res["burst_table"] = {}, {}
    for k in (1024, 4096):
        tfs = lattice(k)
        counts, cost, best = np.zeros((k, 4), np.uint32), np.zeros(k, np.uint64), C.c_int32(-1)
        res["chunk_table"][str(k)] = {}
        for c in CHUNKS:
            set_env(c, None)
            res["chunk_table"][str(k)][str(c)] = timed(det, FIELD_KERNELS, field_call(tfs, counts, cost, best), args)["k_match_field"]
    tfs = lattice(1024)
    counts, cost, best = np.zeros((1024, 4), np.uint32), np.zeros(1024, np.uint64), C.c_int32(-1)
    for u in BURSTS:
        set_env(None, u)
        res["burst_table"][str(u)] = timed(det, FIELD_KERNELS, field_call(tfs, counts, cost, best), args)["k_match_field"]
    set_env(None, None)  # the kept chunk and burst
    ref = None
    if parent is not None:  # the parent's library on the same map: it reads the same field, scan and poses
        ref = make(parent)
        ref.write_map(capi.MAP_VOXELS, det.read_map())
    for k in LATTICES:
        tfs = lattice(k)
        counts, cost, best = np.zeros((k, 4), np.uint32), np.zeros(k, np.uint64), C.c_int32(-1)
        before = None
        if ref is not None:
            before = timed(ref, FIELD_KERNELS, field_call(tfs, counts, cost, best, parent, ref), args)
            before["score"] = timed(ref, SCORE_KERNELS, score_call(tfs, np.zeros((k, 4), np.uint32), best, parent, ref), args)["k_match_score"]
            was = counts.copy(), cost.copy()
        per = timed(det, FIELD_KERNELS, field_call(tfs, counts, cost, best), args)
        if before is not None:
            assert (counts == was[0]).all() and (cost == was[1]).all()  # (the two libraries answer alike)
            per["parent"] = before
        assert (counts.sum(axis=1) == n_px).all() and (counts[:, 0] == counts[0, 0]).all()
        per.update(n_live=n_px - int(counts[0, 0]), best=int(best.value), cost_best=int(cost[best.value]))
        occ = np.zeros((k, 4), np.uint32)
        per["score"] = timed(det, SCORE_KERNELS, score_call(tfs, occ, best), args)["k_match_score"]
        res["poses"][str(k)] = per
    det.close()
    if ref is not None:
        ref.close()
    return res


def summary(results):
    parts = []
    for r in results:
        us = lambda v: v["median_ms"] * 1e3
        head = f"{r['sensor']} at {r['voxel_size']} m ({r['map'][0]} x {r['map'][1]} x {r['map'][2]} voxels, field {r['field_MB']} MB, warmed by {r['warm_scans']} scans), threshold {r['threshold']}: "
        radii = "; ".join(f"radius {R}: `k_match_bits` {us(p['k_match_bits']):.1f} us, `k_dist_x` {us(p['k_dist_x']):.1f} us, `k_dist_y` {us(p['k_dist_y']):.1f} us, `k_dist_z` {us(p['k_dist_z']):.1f} us, "
                          f"the C call {p['host_call']['median_ms']:.2f} ms on the host clock (medians of {p['rounds']} calls)" for R, p in r["radii"].items())
        host = (f"; before: `vofod_read_map` {r['host']['read_map_ms']:.0f} ms plus `scipy.ndimage.distance_transform_edt` {r['host']['edt_ms']:.0f} ms on the host, timed once ({r['host']['occupied']} voxels occupied; "
                "the device's field at radius 255 equals that transform, clamped)") if "host" in r else "; the host transform was not timed on this map"
        was = lambda p: (f" (the parent's library: {us(p['parent']['k_match_field']):.1f} us, {us(p['parent']['score']):.1f} us, {us(p['parent']['host_call']):.0f} us)" if "parent" in p else "")
        poses = "; ".join(f"{k} pose{'s' if k != '1' else ''}: `k_match_field` {us(p['k_match_field']):.1f} us beside `k_match_score` {us(p['score']):.1f} us, the C call {us(p['host_call']):.0f} us" + was(p)
                          for k, p in r["poses"].items())
        row = lambda t: " / ".join(f"{us(v):.1f}" for v in t.values())
        tab = ("; `k_match_field` by chunk " + " / ".join(map(str, CHUNKS)) + ": " + "; ".join(f"at {k} poses {row(t)} us" for k, t in r["chunk_table"].items()) + "; by burst "
               + " / ".join(r["burst_table"]) + f" at 1024 poses and the kept chunk: {row(r['burst_table'])} us")
        parts.append(head + radii + host + f"; the field match, {r['poses']['1']['n_live']} live returns, field of radius {FIELD_RADIUS}: " + poses + tab)
    return "measured: " + ". ".join(parts) + ".\n" + "".join(json.dumps(r) + "\n" for r in results)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--map-warm-scans", type=int, default=96)
    ap.add_argument("--big", type=int, default=1, help="also OS2-128 x 2048 at 0.1 m")
    ap.add_argument("--big-warm-scans", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slow-ms", type=float, default=200.0, help="a call slower than this is measured over three rounds")
    ap.add_argument("--host-edt-max-voxels", type=int, default=400_000_000, help="maps above this are not transformed on the host")
    ap.add_argument("--parent-lib", default=None, help="libvofod_hip.so built from the parent commit: the field-match table is taken from it too, the parent first")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r32_map_distance.txt"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("map_distance_bench.py needs a GPU: no timing without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    parent = older_library(args.parent_lib) if args.parent_lib else None
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    keep = "".join(l + "\n" for l in Path(args.out).read_text().splitlines() if l.startswith(("resources: ", "bench: ", "mutations: "))) if Path(args.out).exists() else ""
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    results = []
    for shape in [("os1-128", 0.25, args.map_warm_scans)] + ([("os2-128x2048", 0.1, args.big_warm_scans)] if args.big else []):
        results.append(measure(args, *shape, pool, torch, dev, parent))
        Path(args.out).write_text(summary(results) + keep)  # (after every shape: the second one is long)
    pool.shutdown()
    sys.stdout.write(summary(results) + keep)


if __name__ == "__main__":
    main()
