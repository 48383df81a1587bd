"""The map-query calls of this tree beside those of a library built from the parent commit, in turns: both
libraries in one process on the same warmed map, distance field, scan and candidate poses; --pairs times over, the parent first in
each pair, the medians of twelve calls of
  - `k_match_score` and `k_match_field` from the library's profiler (the scan a range image in device memory) at 1 / 64 / 1024 / 4096 poses,
  - the host clock of `vofod_map_match` and `vofod_map_match_field` with a host-resident scan that carries a pose table,
  - `k_map_render_scans` and the host clock of `vofod_map_render_scans` with 1 and 64 host-resident views,
and the two libraries' answers compared bit for bit.  OS1-128 at 0.25 m on bench.py's warmed map, then OS2-128 x 2048 at 0.1 m
(--big 0 leaves it out).  Per figure the parent's span over its turns is the margin: `inside`, `below` or `ABOVE` says where the
largest of the change's medians lies.  Writes the table and one JSON line per shape behind the summary lines (`measured: `,
`resources: `, `bench: `, `mutations: `, `suite: `) that OUT already holds.
usage: tools/map_queries_ab.py PARENT_LIB [OUT] [--pairs 3] [--big 1]
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
from map_match_bench import LATTICES, prof  # noqa: E402
from vofod_amd import capi, synth  # noqa: E402
from vofod_amd.detector import ScanData, VoFOD, default_params, pose_lattice  # noqa: E402

F = np.float32
ROUNDS, WARMUP = 12, 3


def timed(det, call, kernel=None):
    """median device time of `kernel` (None: no profile) and median host-clock time of the call, over ROUNDS calls"""
    dev_ms, host = [], []
    for r in range(WARMUP + ROUNDS):
        if kernel:
            det.lib.profile_enable(det.h, 1)
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if kernel:
            p = prof(det)
            det.lib.profile_enable(det.h, 0)
            if r >= WARMUP:
                dev_ms.append(p[kernel][0])
        if r >= WARMUP:
            host.append((t1 - t0) * 1e3)
    return (statistics.median(dev_ms) * 1e3 if kernel else None), statistics.median(host) * 1e3


def shape(sensor, voxel_size, warm_scans, pool, torch, dev, libs, pairs):
    h, w, vfov_deg, _ = synth.SENSORS[sensor]
    n_px = h * w

    def make(lb):
        sp, dp = default_params(lb)
        sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = voxel_size, w, h, 1
        sp.sensor_vfov = F(np.deg2rad(vfov_deg))
        return VoFOD(lb, sp, dp)

    dets = {"change": make(libs["change"])}
    scene = synth.bench_scene()
    synth.warm_map(dets["change"], scene, sensor, warm_scans, pmap=pool.map)
    dets["parent"] = make(libs["parent"])
    dets["parent"].write_map(capi.MAP_VOXELS, dets["change"].read_map())
    frame = synth.bench_frames(scene, sensor, 1, 0, pmap=pool.map)[0]
    tf = np.asarray(frame.tf, F)
    det0 = dets["change"]
    thr = float(det0.dp.voxel_map__thresholds__new_obstacles)
    length = float(det0.dp.raycast__max_distance)
    n = det0.n_voxels
    field = torch.zeros(n, dtype=torch.int16, device=dev)
    st = libs["parent"].map_distance(dets["parent"].h, C.c_float(thr), 8, C.c_void_p(field.data_ptr()), n, capi.MEM_DEVICE)
    assert st == capi.OK, st
    rng_host = np.ascontiguousarray(frame.scan.range, np.uint32)
    rng_dev = torch.from_numpy(rng_host.view(np.int32)).to(dev)
    cs_dev = ScanData.range_image(rng_dev.data_ptr(), w, h, memspace=capi.MEM_DEVICE).as_c()
    table = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=F), (w, 1, 1)))
    host_scan = ScanData.range_image(rng_host, w, h, col_tfs=table)
    cs_host = host_scan.as_c()
    res = {}  # metric -> {"parent": [..], "change": [..]}
    answers = {}

    def note(metric, who, v):
        res.setdefault(metric, {"parent": [], "change": []})[who].append(round(v, 2))

    for pair in range(pairs):
        for who in ("parent", "change"):
            lib, det = libs[who], dets[who]
            for k, (cnt, n_yaw) in LATTICES.items():
                tfs = pose_lattice(libs["change"], tf, (voxel_size,) * 3, cnt, 0.01, n_yaw)
                t = np.ascontiguousarray(tfs, F).reshape(-1)
                counts, fcounts, cost, best = np.zeros((k, 4), np.uint32), np.zeros((k, 4), np.uint32), np.zeros(k, np.uint64), C.c_int32(-1)

                def score(cs):
                    def call():
                        s_ = lib.map_match(det.h, C.byref(cs), capi.ptr(t), k, C.c_float(thr), capi.ptr(counts), C.byref(best))
                        assert s_ == capi.OK, s_
                    return call

                def by_field(cs):
                    def call():
                        s_ = lib.map_match_field(det.h, C.byref(cs), capi.ptr(t), k, C.c_void_p(field.data_ptr()), n, capi.MEM_DEVICE, 8, 64, capi.ptr(fcounts), capi.ptr(cost), C.byref(best))
                        assert s_ == capi.OK, s_
                    return call

                note(f"k_match_score us, {k} poses", who, timed(det, score(cs_dev), "k_match_score")[0])
                note(f"k_match_field us, {k} poses", who, timed(det, by_field(cs_dev), "k_match_field")[0])
                note(f"vofod_map_match host scan, host us, {k} poses", who, timed(det, score(cs_host))[1])
                note(f"vofod_map_match_field host scan, host us, {k} poses", who, timed(det, by_field(cs_host))[1])
                key = (k, counts.tobytes(), fcounts.tobytes(), cost.tobytes())
                assert answers.setdefault(k, key) == key, f"the two libraries differ at {k} poses"
            for nv in (1, 64):
                tfs = pose_lattice(libs["change"], tf, (voxel_size,) * 3, LATTICES[nv][0], 0.01, LATTICES[nv][1])
                t = np.ascontiguousarray(tfs, F).reshape(-1)
                arr = (capi.Scan * nv)(*[cs_host] * nv)
                vc = np.zeros((nv, 8), np.uint32)

                def walk():
                    s_ = lib.map_render_scans(det.h, arr, capi.ptr(t), nv, C.c_float(thr), C.c_float(length), C.c_float(voxel_size), None, None, None, None, None, capi.ptr(vc), C.c_int32(capi.MEM_HOST))
                    assert s_ == capi.OK, s_

                d_us, h_us = timed(det, walk, "k_map_render_scans")
                note(f"k_map_render_scans us, {nv} host views", who, d_us)
                note(f"vofod_map_render_scans host scans, host us, {nv} views", who, h_us)
                key = vc.tobytes()
                assert answers.setdefault(("walk", nv), key) == key
        print(f"[map_queries_ab] {sensor}: pair {pair + 1} of {pairs}", file=sys.stderr, flush=True)
    for d in dets.values():
        d.close()
    lines = [f"{sensor} at {voxel_size} m ({n_px} pixels, {n_px - int(counts[0, 0])} live, map {list(det0.map_size)}, warmed by {warm_scans} scans); medians of {ROUNDS} calls, {pairs} pairs, parent first in each pair"]
    for metric, v in res.items():
        lo, hi = min(v["parent"]), max(v["parent"])
        worst = max(v["change"])
        verdict = "inside" if lo <= worst <= hi else ("below" if worst < lo else "ABOVE")
        lines.append(f"  {metric:62s} parent {v['parent']} span [{lo}, {hi}]   change {v['change']}   {verdict}")
    return lines, {"sensor": sensor, "voxel_size": voxel_size, "metrics": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib")
    ap.add_argument("out", nargs="?", default=str(ROOT / "profiles" / "r33_map_queries.txt"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--big", type=int, default=1)
    args = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    libs = {"parent": capi.Library(args.parent_lib, "vofod_"), "change": vofod_amd.library()}
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    keep = "".join(l + "\n" for l in Path(args.out).read_text().splitlines() if l.startswith(("measured: ", "resources: ", "bench: ", "mutations: ", "suite: "))) if Path(args.out).exists() else ""
    text, js = [], []
    for s in [("os1-128", 0.25, 96)] + ([("os2-128x2048", 0.1, 8)] if args.big else []):
        lines, j = shape(*s, pool, torch, dev, libs, args.pairs)
        text += lines
        js.append(j)
        Path(args.out).write_text(keep + "\n".join(text) + "\n" + "".join(json.dumps(x) + "\n" for x in js))
    pool.shutdown()
    print("\n".join(text))


if __name__ == "__main__":
    main()
