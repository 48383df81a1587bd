"""vofod_detection_points at the benchmark's loaded shape: what the member voxels and AABBs of a batch's detections cost, against
the only way to get them without it.  Prints one JSON line (recorded in profiles/r12_detection_points.txt).

The `loaded_tail` scene of bench.py: 256 x OS1-128 at 0.25 m, 12 floating targets, the warmed map, device-resident columns.
  (a) vofod_detection_points(ticket) after a collected batch (submit + collect outside the clock): wall time of the call pair
      the Python wrapper makes (size query + answer into host arrays), and k_det_points' device time from vofod_profile_read;
  (b) process_batch(debug=True, far_only=True) minus a plain process_batch on the same batch: the debug view is the one source of
      the same data that exists without the call (full emission, host tail, read-back of every frame's weighted cloud and labels).
Each figure is the median of `--rounds` repeats after `--warmup` untimed ones; (a) and (b) alternate in one process.  A report,
not a gate."""
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
    ap.add_argument("--targets", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--debug-rounds", type=int, default=3, help="repeats of leg (b): a debug batch of 256 frames takes seconds")
    args = ap.parse_args()
    import torch

    # (as bench.py: torch opens the device before the library's handle is created)
    if not torch.cuda.is_available():
        raise SystemExit("detection_points_bench.py needs a GPU: no timing without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    F = args.frames
    lib = vofod_amd.library()
    h, w, vfov_deg, _ = synth.SENSORS[args.sensor]
    n_pts = h * w
    sp, dp = default_params(lib)
    sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = args.voxel_size, w, h, F
    sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
    det = VoFOD(lib, sp, dp)
    det.reserve(1)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    synth.warm_map(det, synth.bench_scene(), args.sensor, args.map_warm_scans, pmap=pool.map)
    busy = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=args.targets)
    frames = synth.bench_frames(busy, args.sensor, F, 0, pmap=pool.map)
    pool.shutdown()
    xyz = torch.empty((F, 3, n_pts), dtype=torch.float32)
    for f, s in enumerate(frames):
        xyz[f, 0], xyz[f, 1], xyz[f, 2] = torch.from_numpy(s.x), torch.from_numpy(s.y), torch.from_numpy(s.z)
    xyz = xyz.to(dev)
    torch.cuda.synchronize()
    scans = [ScanData(x=xyz[f, 0].data_ptr(), y=xyz[f, 1].data_ptr(), z=xyz[f, 2].data_ptr(), width=w, height=h, memspace=capi.MEM_DEVICE) for f in range(F)]
    tfs = np.stack([s.tf for s in frames]).astype(np.float32)

    def leg_a(profiled):
        tk = det.batch_submit(scans, tfs)
        dets, _ = det.batch_collect(tk)
        if profiled:
            det.lib.profile_enable(det.h, 1)
        t0 = time.perf_counter()
        ext, pts, idx = det.detection_points(tk)  # (the call waits for its stream: the clock stops behind the device work)
        wall = time.perf_counter() - t0
        kern = None
        if profiled:
            kern = prof(det).get("k_det_points", (0.0, 0))
            det.lib.profile_enable(det.h, 0)
        assert len(ext) == len(dets) and int(ext["count"].sum()) == len(pts)
        return wall, kern, len(ext), len(pts)

    def plain():
        t0 = time.perf_counter()
        det.process_batch(scans, tfs)
        return time.perf_counter() - t0

    def debug():
        t0 = time.perf_counter()
        _, _, gs = det.process_batch(scans, tfs, debug=True, far_only=True, clusters_cap=4096)
        return time.perf_counter() - t0, sum(len(g["weighted"]) for g in gs)

    for _ in range(args.warmup):
        leg_a(False)
        plain()
    debug_error = None
    try:
        debug()
    except vofod_amd.VofodError as e:  # (leg (b) is the comparison, not the subject: its failure is recorded, leg (a) still reported)
        debug_error = str(e)
    walls, kerns, plains, debugs = [], [], [], []
    n_det = n_points = n_weighted = 0
    for r in range(args.rounds):
        wall, _, n_det, n_points = leg_a(False)
        walls.append(wall)
        _, kern, _, _ = leg_a(True)  # (the profiler brackets the launch with events: a run of its own)
        assert kern[1] == 1, kern
        kerns.append(kern[0])
        plains.append(plain())
        if r < args.debug_rounds and debug_error is None:
            t, n_weighted = debug()
            debugs.append(t)
    med = statistics.median
    if debug_error is not None:
        debugs = [float("nan")]
    out = {
        "tool": "detection_points_bench", "frames": F, "sensor": args.sensor, "voxel_size": args.voxel_size, "targets": args.targets, "rounds": args.rounds, "warmup": args.warmup,
        "detections_per_batch": n_det, "member_points_per_batch": n_points, "weighted_records_per_batch": n_weighted,
        "a_detection_points": {"wall_ms_median": round(1e3 * med(walls), 4), "wall_ms": [round(1e3 * x, 4) for x in walls],
                               "k_det_points_device_ms_median": round(med(kerns), 4), "k_det_points_device_ms": [round(x, 4) for x in kerns],
                               "bytes_returned": 40 * n_det + 20 * n_points},
        "b_debug_view_minus_plain": {"debug_far_only_ms_median": round(1e3 * med(debugs), 3), "debug_far_only_ms": [round(1e3 * x, 3) for x in debugs],
                                     "plain_ms_median": round(1e3 * med(plains), 3), "plain_ms": [round(1e3 * x, 3) for x in plains],
                                     "difference_ms": round(1e3 * (med(debugs) - med(plains)), 3), "bytes_returned": 20 * n_weighted},
    }
    out["b_debug_view_minus_plain"]["error"] = debug_error
    out["b_over_a"] = round(out["b_debug_view_minus_plain"]["difference_ms"] / out["a_detection_points"]["wall_ms_median"], 1)
    print(json.dumps(out))
    det.close()


if __name__ == "__main__":
    main()
