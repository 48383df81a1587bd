"""Exact raycast accumulation (include/vofod.h: vofod_set_raycast_exact) at the benchmark's sensor: what the fixed-point units cost or
save in the raycast role.  Prints one JSON line (recorded in profiles/r17_raycast_exact.txt).

One device-resident OS1-128 range image at 0.25 m on a map warmed by 32 scans, ONE process and ONE handle, the library's HIP-event
profiler.  A leg is a whole pass - vofod_raycast_begin, one vofod_process_scan of the same scan (a finish needs a detection iteration),
vofod_raycast_finish; the legs alternate between switch on and switch off, medians of ten after one warm-up pair:
  k_raycast_exact    against k_raycast    condition: ratio <= 1.00 (integer atomics on the same addresses were 0.81 x in a diagnostic build)
  k_ray_sweep_exact  against k_ray_sweep  condition: ratio <= 1.05 (the same bytes; the margin covers run-to-run spread)
Each pair is two instantiations of one template (k_raycast_t / k_ray_sweep_t in vofod_amd/csrc/kernels_raycast.h: the float and the
units accumulator), told apart by profiler name."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import statistics
import sys
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import vofod_amd  # noqa: E402
from vofod_amd import capi, synth  # noqa: E402
from vofod_amd.detector import ScanData, VoFOD, default_params  # noqa: E402

PAIRS = (("k_raycast", "k_raycast_exact", 1.00), ("k_ray_sweep", "k_ray_sweep_exact", 1.05))


def prof(det):
    names, ms, calls = (C.c_char * (64 * 128))(), (C.c_double * 128)(), (C.c_uint64 * 128)()
    n = det.lib.profile_read(det.h, names, ms, calls, 128)
    return {names[64 * i : 64 * i + 64].split(b"\0", 1)[0].decode(): (float(ms[i]), int(calls[i])) for i in range(n)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sensor", default="os1-128")
    ap.add_argument("--voxel-size", type=float, default=0.25)
    ap.add_argument("--map-warm-scans", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=10)
    args = ap.parse_args()
    import torch

    lib = vofod_amd.library()
    h, w, vfov_deg, _ = synth.SENSORS[args.sensor]
    sp, dp = default_params(lib)
    sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = args.voxel_size, w, h, 1
    sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
    det = VoFOD(lib, sp, dp)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    scene = synth.bench_scene()
    synth.warm_map(det, scene, args.sensor, args.map_warm_scans, pmap=pool.map)
    s = synth.bench_frames(scene, args.sensor, 1, 0, pmap=pool.map)[0]
    pool.shutdown()
    dev = torch.device("cuda", 0)
    d_rng = torch.from_numpy(s.range.view(np.int32)).to(dev)
    d_int = torch.from_numpy(np.ascontiguousarray(s.intensity, dtype=np.float32)).to(dev)
    torch.cuda.synchronize()
    scan = ScanData.range_image(d_rng.data_ptr(), w, h, intensity=d_int.data_ptr(), memspace=capi.MEM_DEVICE)

    def leg(exact):
        """({kernel: device ms}, voxels the pass touched, S or None) of one whole pass"""
        assert det.set_raycast_exact(exact) == capi.OK
        prof(det)
        assert det.raycast_begin(scan, s.tf) == capi.OK
        touched = int(np.count_nonzero(det.read_map(capi.MAP_RAYCAST)))
        log2_units = det.raycast_units()[1] if exact else None
        det.process_scan(scan, s.tf)
        assert det.raycast_finish() == capi.OK
        p = prof(det)
        mine, other = [k[1 if exact else 0] for k in PAIRS], [k[0 if exact else 1] for k in PAIRS]
        assert all(p.get(k, (0, 0))[1] == 1 for k in mine) and not any(k in p for k in other), p
        return {k: p[k][0] for k in mine}, touched, log2_units

    det.lib.profile_enable(det.h, 1)
    ms = {k: [] for pair in PAIRS for k in pair[:2]}
    touched, log2_units = {}, None
    for i in range(args.pairs + 1):  # (the first pair warms up and is dropped)
        for exact in (False, True):
            t, n_touched, s_leg = leg(exact)
            touched["exact" if exact else "float"] = n_touched
            log2_units = s_leg if exact else log2_units
            if i:
                for k, v in t.items():
                    ms[k].append(v)
    det.lib.profile_enable(det.h, 0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = {f"{e}_over_{f}": {"ratio": round(med[e] / med[f], 3), "condition": f"<= {lim:.2f}", "met": bool(med[e] / med[f] <= lim)} for f, e, lim in PAIRS}
    print(json.dumps({
        "tool": "raycast_exact_bench", "sensor": args.sensor, "rays": h * w, "voxel_size": args.voxel_size, "map_warm_scans": args.map_warm_scans, "pairs": args.pairs,
        "log2_units_per_m": log2_units, "voxels_touched": touched,
        "device_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "device_ms_median": {k: round(v, 4) for k, v in med.items()}, "ratios": ratios,
    }))
    det.close()


if __name__ == "__main__":
    main()
