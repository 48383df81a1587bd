"""Motion-compensated point scans (include/vofod.h: a point scan with col_tfs under vofod_set_point_motion) at the benchmark's shape:
what k_point_deskew costs per batch, in both pose-fetch forms, and what the poses cost in the batch rate.  Prints one JSON line
(recorded in profiles/r21_point_motion.txt).

256 x OS1-128 at 0.25 m, the warmed map and the submit / collect pipeline of bench.py, ONE process, device events:
  kernel   k_point_deskew on device-resident packed columns and on device-resident 48-byte structs, each with 16-byte aligned pose
           tables (the wave's poses fetched through LDS: the span form) and with the same tables 4 bytes behind a 16-byte boundary
           (every lane loads its poses from the table with 4-byte loads: the direct form), against k_range_decode_motion and
           k_range_decode on the same scans handed over as range images: synchronous batches under the library's HIP-event profiler,
           the legs alternating, median of five.  Byte model of k_point_deskew: 24 B per pixel (three
           floats in, three out) plus 48 B x width per frame (the table).
  batches  a batch of point scans with poses against the same scans without (points deskewed by the caller: the only route before),
           device-resident and pinned-host packed columns, `--inflight` batches in flight, frames/s; legs alternating, `--rounds`
           times each, medians."""
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


DECODES = ("k_point_deskew", "k_range_decode_motion", "k_range_decode")


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
    det.set_point_motion(True)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    scene = synth.bench_scene()
    synth.warm_map(det, scene, args.sensor, args.map_warm_scans, pmap=pool.map)
    frames = synth.bench_frames(scene, args.sensor, F, 0, pmap=pool.map)
    pool.shutdown()
    tfs = np.stack([s.tf for s in frames]).astype(np.float32)
    dev = torch.device("cuda", 0)
    # a pose table per frame: a hovering vehicle's drift over one period (the tables of tools/range_motion_bench.py)
    tables = np.zeros((F, w, 3, 4), dtype=np.float32)
    rs = np.random.default_rng(0)
    for f in range(F):
        begin = np.eye(3, 4, dtype=np.float32)
        th = rs.uniform(-0.1, 0.1)
        begin[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        begin[:, 3] = rs.uniform(-0.3, 0.3, 3)
        tables[f] = column_poses(lib, begin, np.eye(3, 4, dtype=np.float32), np.eye(3, 4, dtype=np.float32), w)

    # the scans on the device: the sensor's ranges, their rigid points as packed columns (decoded by the library) and as 48-byte structs
    rng_d = torch.empty((F, n_pts), dtype=torch.int32)
    for f, s in enumerate(frames):
        rng_d[f] = torch.from_numpy(s.range.view(np.int32))
    rng_d = rng_d.to(dev)
    tab_d = torch.from_numpy(tables).to(dev)
    tab_d4 = torch.empty(tables.size + 4, dtype=torch.float32, device=dev)[1:1 + tables.size].view(F, w, 3, 4)  # the same tables at +4 bytes
    tab_d4.copy_(tab_d)
    assert tab_d[0].data_ptr() % 16 == 0 and tab_d4[0].data_ptr() % 16 == 4
    pts_d = torch.empty((F, 3, n_pts), dtype=torch.float32, device=dev)
    for f in range(F):
        det.range_to_points(ScanData.range_image(rng_d[f].data_ptr(), w, h, memspace=capi.MEM_DEVICE), out=[pts_d[f, a].data_ptr() for a in range(3)])
    aos_d = torch.zeros((F, n_pts, 12), dtype=torch.float32, device=dev)
    aos_d[:, :, :3] = pts_d.permute(0, 2, 1)
    pts_h, tab_h = pts_d.cpu().pin_memory(), torch.from_numpy(tables).pin_memory()
    torch.cuda.synchronize()

    def points(buf, space, tab=None):
        return [ScanData(x=buf[f, 0].data_ptr(), y=buf[f, 1].data_ptr(), z=buf[f, 2].data_ptr(), width=w, height=h, memspace=space, col_tfs=None if tab is None else tab[f].data_ptr()) for f in range(F)]

    def structs(tab=None):
        return [ScanData(x=aos_d[f].data_ptr(), y=aos_d[f].data_ptr() + 4, z=aos_d[f].data_ptr() + 8, width=w, height=h, stride_bytes=48, memspace=capi.MEM_DEVICE,
                         col_tfs=None if tab is None else tab[f].data_ptr()) for f in range(F)]

    legs = {
        "range_plain": [ScanData.range_image(rng_d[f].data_ptr(), w, h, memspace=capi.MEM_DEVICE) for f in range(F)],
        "range_motion": [ScanData.range_image(rng_d[f].data_ptr(), w, h, memspace=capi.MEM_DEVICE, col_tfs=tab_d[f].data_ptr()) for f in range(F)],
        "device_packed_motion": points(pts_d, capi.MEM_DEVICE, tab_d),
        "device_packed_plain": points(pts_d, capi.MEM_DEVICE),
        "device_aos48_motion": structs(tab_d),
        "device_packed_motion4": points(pts_d, capi.MEM_DEVICE, tab_d4),
        "device_aos48_motion4": structs(tab_d4),
        "host_packed_motion": points(pts_h, capi.MEM_HOST, tab_h),
        "host_packed_plain": points(pts_h, capi.MEM_HOST),
    }

    # ---- the kernels alone: (label, leg, kernel)
    kernel_legs = [("range_plain", "range_plain", "k_range_decode"), ("range_motion", "range_motion", "k_range_decode_motion"),
                   ("device_packed_motion/span", "device_packed_motion", "k_point_deskew"), ("device_packed_motion/direct4", "device_packed_motion4", "k_point_deskew"),
                   ("device_aos48_motion/span", "device_aos48_motion", "k_point_deskew"), ("device_aos48_motion/direct4", "device_aos48_motion4", "k_point_deskew")]
    det.lib.profile_enable(det.h, 1)
    ms = {label: [] for label, _, _ in kernel_legs}
    for i in range(6):  # (the first round warms up and is dropped)
        for label, leg, kern in kernel_legs:
            prof(det)
            det.process_batch(legs[leg], tfs)
            p = prof(det)
            t, calls = p.get(kern, (0.0, 0))
            assert calls == 1 and not [k for k in DECODES if k != kern and k in p], p
            if i:
                ms[label].append(t)
    det.lib.profile_enable(det.h, 0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    model_bytes = (24.0 * n_pts + 48.0 * w) * F

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

    rate_legs = ("device_packed_plain", "device_packed_motion", "host_packed_plain", "host_packed_motion")
    rates = {leg: [] for leg in rate_legs}
    dets = {leg: run(leg, args.warmup) for leg in rate_legs}
    for _ in range(args.rounds):
        for leg in rate_legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(leg, args.steps)
            torch.cuda.synchronize()
            rates[leg].append(F * args.steps / (time.perf_counter() - t0))

    def summary(v):
        return {"frames_per_s_median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "rounds": [round(x, 1) for x in v]}

    out_legs = {leg: summary(v) for leg, v in rates.items()}
    print(json.dumps({
        "tool": "point_motion_bench", "frames": F, "sensor": args.sensor, "points_per_frame": n_pts, "voxel_size": args.voxel_size, "map_warm_scans": args.map_warm_scans,
        "batches_in_flight": args.inflight, "rounds": args.rounds, "steps_per_round": args.steps, "warmup_steps": args.warmup,
        "kernel": {"device_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "device_ms_median": {k: round(v, 4) for k, v in med.items()},
                   "over_k_range_decode_motion": {k: round(v / med["range_motion"], 3) for k, v in med.items()},
                   "over_k_range_decode": {k: round(v / med["range_plain"], 3) for k, v in med.items()},
                   "k_point_deskew_bytes_model": model_bytes, "k_point_deskew_GBps_model": {k: round(model_bytes / (v * 1e-3) / 1e9, 1) for k, v in med.items() if "/" in k}},
        "legs": out_legs, "detections_in_warmup": dets,
        "device_motion_vs_device_plain": round(out_legs["device_packed_motion"]["frames_per_s_median"] / out_legs["device_packed_plain"]["frames_per_s_median"], 3),
        "host_motion_vs_host_plain": round(out_legs["host_packed_motion"]["frames_per_s_median"] / out_legs["host_packed_plain"]["frames_per_s_median"], 3),
    }))
    det.close()


if __name__ == "__main__":
    main()
