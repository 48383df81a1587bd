"""Range images (include/vofod.h: a vofod_scan with x == y == z == NULL) at the benchmark's shape: what handing over the sensor's
range column instead of points is worth on the host-fed path, and what the decode costs where the inputs are resident.
Prints one JSON line (recorded as profiles/r10_range_input.json).

256 x OS1-128 at 0.25 m, the warmed map and the submit / collect pipeline of bench.py with its number of batches in flight.
Four legs in ONE process, alternating, `--rounds` times each, so that every leg's spread is recorded beside its mean:
  1. host x | y | z columns at a constant pitch, pinned (12 B per point: today's best host layout)
  2. host range columns at a constant pitch, pinned (4 B per point), decoded on the device by k_range_decode
  3. device-resident x | y | z (what bench.py times)
  4. device-resident range
Pass condition: leg 2 is not slower than leg 1 beyond the spread of this same run (the larger of the two legs' max - min).
Leg 4 against leg 3 is the price of not fusing the decode into the frame kernel: recorded, no condition.
k_range_decode itself: device time from the library's HIP-event profiler on synchronous batches, bytes from the model 16 N per
frame (4 read, 12 written) + 24 N of LUT per chunk of frames (re-reads served by the L2 / Infinity Cache), share of the HBM peak."""
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
from vofod_amd.detector import ScanData, VoFOD, default_params  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, as bench.py
RD_CHUNK_MAX = 8       # range_decode.h


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
    ap.add_argument("--inflight", type=int, default=0, help="batches in flight; 0 = bench.py's choice (four from 128 frames on, eight below)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12, help="batches per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    F = args.frames
    inflight = args.inflight if args.inflight > 0 else (4 if F >= 128 else 8)
    lib = vofod_amd.library()
    h, w, vfov_deg, _ = synth.SENSORS[args.sensor]
    n_pts = h * w
    sp, dp = default_params(lib)
    sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = args.voxel_size, w, h, F
    sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
    det = VoFOD(lib, sp, dp)
    det.reserve(inflight)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    scene = synth.bench_scene()
    synth.warm_map(det, scene, args.sensor, args.map_warm_scans, pmap=pool.map)
    sets = [synth.bench_frames(scene, args.sensor, F, rank, pmap=pool.map) for rank in (0, 5000)]  # two sets, alternated (as bench.py)
    pool.shutdown()
    dev = torch.device("cuda", 0)

    def columns(frames, pinned):
        xyz = torch.empty((F, 3, n_pts), dtype=torch.float32)
        rng = torch.empty((F, n_pts), dtype=torch.int32)  # (the bits of the uint32 millimetres)
        for f, s in enumerate(frames):
            xyz[f, 0], xyz[f, 1], xyz[f, 2] = torch.from_numpy(s.x), torch.from_numpy(s.y), torch.from_numpy(s.z)
            rng[f] = torch.from_numpy(s.range.view(np.int32))
        xyz, rng = (xyz.pin_memory(), rng.pin_memory()) if pinned else (xyz.to(dev), rng.to(dev))
        space = capi.MEM_HOST if pinned else capi.MEM_DEVICE
        pts = [ScanData(x=xyz[f, 0].data_ptr(), y=xyz[f, 1].data_ptr(), z=xyz[f, 2].data_ptr(), width=w, height=h, memspace=space) for f in range(F)]
        rgs = [ScanData.range_image(rng[f].data_ptr(), w, h, memspace=space) for f in range(F)]
        return (xyz, rng), pts, rgs

    keep, legs = [], {"host_xyz": [], "host_range": [], "device_xyz": [], "device_range": []}
    for frames in sets:
        tfs = np.stack([s.tf for s in frames]).astype(np.float32)
        for pinned in (True, False):
            bufs, pts, rgs = columns(frames, pinned)
            keep.append(bufs)
            legs["host_xyz" if pinned else "device_xyz"].append((pts, tfs))
            legs["host_range" if pinned else "device_range"].append((rgs, tfs))
    torch.cuda.synchronize()

    def run(leg, k):
        infl, n_det = [], 0
        for i in range(k):
            sc, tfs = legs[leg][i & 1]
            infl.append(det.batch_submit(sc, tfs))
            if len(infl) == inflight:
                n_det += len(det.batch_collect(infl.pop(0))[0])
        while infl:
            n_det += len(det.batch_collect(infl.pop(0))[0])
        return n_det

    rates = {leg: [] for leg in legs}
    dets = {}
    for leg in legs:
        dets[leg] = run(leg, args.warmup)
    for _ in range(args.rounds):
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(leg, args.steps)
            torch.cuda.synchronize()
            rates[leg].append(F * args.steps / (time.perf_counter() - t0))

    def summary(v):
        return {"frames_per_s_mean": round(statistics.mean(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                "stdev": round(statistics.stdev(v), 1) if len(v) > 1 else None, "rounds": [round(x, 1) for x in v]}

    out_legs = {leg: summary(v) for leg, v in rates.items()}
    for leg, bpp in (("host_xyz", 12.0), ("host_range", 4.0)):
        out_legs[leg]["h2d_GBps_mean"] = round(bpp * n_pts * out_legs[leg]["frames_per_s_mean"] / 1e9, 2)
    spread = max(out_legs[k]["max"] - out_legs[k]["min"] for k in ("host_xyz", "host_range"))
    m1, m2 = out_legs["host_xyz"]["frames_per_s_mean"], out_legs["host_range"]["frames_per_s_mean"]
    m3, m4 = out_legs["device_xyz"]["frames_per_s_mean"], out_legs["device_range"]["frames_per_s_mean"]

    # k_range_decode alone: synchronous batches under the event profiler (every launch bracketed by two events on its stream)
    chunk = min(max(F // 16, 1), RD_CHUNK_MAX)
    n_chunks = (F + chunk - 1) // chunk
    model_bytes = 16.0 * n_pts * F + 24.0 * n_pts * n_chunks
    kernel = {}
    det.lib.profile_enable(det.h, 1)
    for leg in ("device_range", "host_range"):
        ms = []
        for i in range(5):
            sc, tfs = legs[leg][i & 1]
            prof(det)
            det.process_batch(sc, tfs)
            t, calls = prof(det).get("k_range_decode", (0.0, 0))
            assert calls == 1, calls
            ms.append(t)
        med = statistics.median(ms)
        kernel[leg] = {"device_ms": [round(x, 4) for x in ms], "device_ms_median": round(med, 4), "GBps_model": round(model_bytes / (med * 1e-3) / 1e9, 1),
                       "share_of_hbm_peak": round(model_bytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)}
    det.lib.profile_enable(det.h, 0)
    print(json.dumps({
        "tool": "range_input_bench", "frames": F, "sensor": args.sensor, "points_per_frame": n_pts, "voxel_size": args.voxel_size, "map_warm_scans": args.map_warm_scans,
        "batches_in_flight": inflight, "rounds": args.rounds, "steps_per_round": args.steps, "warmup_steps": args.warmup,
        "legs": out_legs, "detections_in_warmup": dets,
        "host_range_vs_host_xyz": {"ratio": round(m2 / m1, 3), "spread_frames_per_s": round(spread, 1), "pass": bool(m2 >= m1 - spread),
                                   "bytes_bound_on_the_ratio": 3.0},
        "device_range_vs_device_xyz": {"ratio": round(m4 / m3, 3), "extra_us_per_batch": round(1e6 * F * (1.0 / m4 - 1.0 / m3), 1)},
        "k_range_decode": {"frames_per_chunk": chunk, "chunks": n_chunks, "bytes_model": model_bytes,
                           "bytes_model_note": "16 N per frame (4 read, 12 written) + 24 N of LUT per chunk; the LUT term (3 MB table) is served by the L2 / Infinity Cache",
                           "hbm_peak_GBps": HBM_PEAK_GBS, **kernel},
    }))
    det.close()


if __name__ == "__main__":
    main()
