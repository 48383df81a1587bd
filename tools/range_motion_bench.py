"""Motion-compensated range images (include/vofod.h: a range image with col_tfs) at the benchmark's shape: what the pose per column
costs in the decode kernel and in the batch rate.  Prints one JSON line (recorded in profiles/r15_range_motion.txt).

256 x OS1-128 at 0.25 m, the warmed map and the submit / collect pipeline of bench.py, ONE process, device events:
  kernel   k_range_decode_motion against k_range_decode on the same device-resident range images: synchronous batches under the
           library's HIP-event profiler, the two legs alternating, median of five.  Both move 16 B per pixel plus the LUT; the pose
           tables (48 KB per 2 MB frame) are cache-resident.  Condition: at most 1.25 x k_range_decode's time.
  batches  a batch of compensated range images against the same batch without poses, host-resident (pinned, constant pitch: one 2-D
           copy for the ranges, one for the tables) and device-resident, `--inflight` batches in flight, frames/s; legs alternating,
           `--rounds` times each."""
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
from vofod_amd.detector import ScanData, VoFOD, column_poses, default_params  # noqa: E402


def prof(det):
    names, ms, calls = (C.c_char * (64 * 128))(), (C.c_double * 128)(), (C.c_uint64 * 128)()
    n = det.lib.profile_read(det.h, names, ms, calls, 128)
    return {names[64 * i : 64 * i + 64].split(b"\0", 1)[0].decode(): (float(ms[i]), int(calls[i])) for i in range(n)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--sensor", default="os1-128")
    ap.add_argument("--voxel-size", type=float, default=0.25)
    ap.add_argument("--map-warm-scans", type=int, default=96)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12, help="batches per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    F = args.frames
    lib = vofod_amd.library()
    h, w, vfov_deg, _ = synth.SENSORS[args.sensor]
    n_pts = h * w
    sp, dp = default_params(lib)
    sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = args.voxel_size, w, h, F
    sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
    det = VoFOD(lib, sp, dp)
    det.reserve(args.inflight)
    det.set_column_shift((7 * np.arange(h) - 40).astype(np.int32))  # a destaggered image
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    scene = synth.bench_scene()
    synth.warm_map(det, scene, args.sensor, args.map_warm_scans, pmap=pool.map)
    frames = synth.bench_frames(scene, args.sensor, F, 0, pmap=pool.map)
    pool.shutdown()
    tfs = np.stack([s.tf for s in frames]).astype(np.float32)
    dev = torch.device("cuda", 0)
    # a pose table per frame: a hovering vehicle's drift over one period, 1 rad/s and 3 m/s at the most
    tables = np.zeros((F, w, 3, 4), dtype=np.float32)
    rs = np.random.default_rng(0)
    for f in range(F):
        begin = np.eye(3, 4, dtype=np.float32)
        th = rs.uniform(-0.1, 0.1)
        begin[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        begin[:, 3] = rs.uniform(-0.3, 0.3, 3)
        tables[f] = column_poses(lib, begin, np.eye(3, 4, dtype=np.float32), np.eye(3, 4, dtype=np.float32), w)

    def legs_of(pinned):
        rng = torch.empty((F, n_pts), dtype=torch.int32)  # (the bits of the uint32 millimetres)
        for f, s in enumerate(frames):
            rng[f] = torch.from_numpy(s.range.view(np.int32))
        tab = torch.from_numpy(tables)
        rng, tab = (rng.pin_memory(), tab.pin_memory()) if pinned else (rng.to(dev), tab.to(dev))
        space = capi.MEM_HOST if pinned else capi.MEM_DEVICE
        plain = [ScanData.range_image(rng[f].data_ptr(), w, h, memspace=space) for f in range(F)]
        motion = [ScanData.range_image(rng[f].data_ptr(), w, h, memspace=space, col_tfs=tab[f].data_ptr()) for f in range(F)]
        return (rng, tab), plain, motion

    keep, legs = [], {}
    for pinned in (True, False):
        bufs, plain, motion = legs_of(pinned)
        keep.append(bufs)
        legs[("host" if pinned else "device") + "_plain"] = plain
        legs[("host" if pinned else "device") + "_motion"] = motion
    torch.cuda.synchronize()

    # ---- the kernels alone
    det.lib.profile_enable(det.h, 1)
    ms = {"k_range_decode": [], "k_range_decode_motion": []}
    for i in range(6):  # (the first pair warms up and is dropped)
        for leg, kern in (("device_plain", "k_range_decode"), ("device_motion", "k_range_decode_motion")):
            prof(det)
            det.process_batch(legs[leg], tfs)
            p = prof(det)
            t, calls = p.get(kern, (0.0, 0))
            other = "k_range_decode_motion" if kern == "k_range_decode" else "k_range_decode"
            assert calls == 1 and other not in p, p
            if i:
                ms[kern].append(t)
    det.lib.profile_enable(det.h, 0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratio = med["k_range_decode_motion"] / med["k_range_decode"]
    chunk = min(max(F // 16, 1), 8)
    n_chunks = (F + chunk - 1) // chunk
    model_bytes = 16.0 * n_pts * F + 24.0 * n_pts * n_chunks

    # ---- batches in flight
    def run(leg, k):
        infl, n_det = [], 0
        for _ in range(k):
            infl.append(det.batch_submit(legs[leg], tfs))
            if len(infl) == args.inflight:
                n_det += len(det.batch_collect(infl.pop(0))[0])
        while infl:
            n_det += len(det.batch_collect(infl.pop(0))[0])
        return n_det

    rates = {leg: [] for leg in legs}
    dets = {leg: run(leg, args.warmup) for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(leg, args.steps)
            torch.cuda.synchronize()
            rates[leg].append(F * args.steps / (time.perf_counter() - t0))

    def summary(v):
        return {"frames_per_s_mean": round(statistics.mean(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "rounds": [round(x, 1) for x in v]}

    out_legs = {leg: summary(v) for leg, v in rates.items()}
    print(json.dumps({
        "tool": "range_motion_bench", "frames": F, "sensor": args.sensor, "points_per_frame": n_pts, "voxel_size": args.voxel_size, "map_warm_scans": args.map_warm_scans,
        "batches_in_flight": args.inflight, "rounds": args.rounds, "steps_per_round": args.steps, "warmup_steps": args.warmup,
        "kernel": {"device_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "device_ms_median": {k: round(v, 4) for k, v in med.items()},
                   "motion_over_plain": round(ratio, 3), "condition": "<= 1.25", "pass": bool(ratio <= 1.25),
                   "bytes_model": model_bytes, "GBps_model": {k: round(model_bytes / (v * 1e-3) / 1e9, 1) for k, v in med.items()}},
        "legs": out_legs, "detections_in_warmup": dets,
        "host_motion_vs_host_plain": round(out_legs["host_motion"]["frames_per_s_mean"] / out_legs["host_plain"]["frames_per_s_mean"], 3),
        "device_motion_vs_device_plain": round(out_legs["device_motion"]["frames_per_s_mean"] / out_legs["device_plain"]["frames_per_s_mean"], 3),
    }))
    det.close()


if __name__ == "__main__":
    main()
