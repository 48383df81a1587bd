"""Motion-compensated rays (include/vofod.h: vofod_set_raycast_motion) at the benchmark's sensor: what the pose per column costs in
the raycast role.  Prints one JSON line (recorded in profiles/r16_raycast_motion.txt).

One device-resident OS1-128 range image at 0.25 m on a warmed map, ONE process, the library's HIP-event profiler:
  kernel   k_raycast_motion (switch on, a rigid twist table of 1 rad/s and 3 m/s, 16-byte aligned, device-resident) against
           k_raycast (switch off) on the same scan: the legs alternate, medians of ten after one warm-up pair.  The new front
           adds one 48-byte pose and about 40 flops to a walk of hundreds of steps.  Expectation: at most 1.10 x k_raycast's time.
           Both are instantiations of one template (k_raycast_t in vofod_amd/csrc/kernels_raycast.h), told apart by profiler name.
  begin    the whole vofod_raycast_begin with a HOST scan (range, intensity and table staged by the call), wall clock, both legs."""
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


def twist_table(width, yaw_rate=1.0, v=(3.0, 0.0, 0.0), period=0.1):
    """a constant twist over one period, the last column the reference (tests/range_motion_cases.py: twist_col_tfs)"""
    out = np.zeros((width, 3, 4))
    for m in range(width):
        s = -(1.0 - m / (width - 1)) * period
        th = yaw_rate * s
        c, sn = np.cos(th), np.sin(th)
        out[m, :, :3] = [[c, -sn, 0], [sn, c, 0], [0, 0, 1]]
        a, b = (1.0, 0.0) if abs(th) < 1e-12 else (sn / th, (1 - c) / th)
        out[m, :, 3] = np.array([[a, -b, 0], [b, a, 0], [0, 0, 1]]) @ (np.asarray(v) * s)
    return out.astype(np.float32)


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
    det.set_column_shift((7 * np.arange(h) - 40).astype(np.int32))  # a destaggered image
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    scene = synth.bench_scene()
    synth.warm_map(det, scene, args.sensor, args.map_warm_scans, pmap=pool.map)
    s = synth.bench_frames(scene, args.sensor, 1, 0, pmap=pool.map)[0]
    pool.shutdown()
    table = twist_table(w)
    dev = torch.device("cuda", 0)
    d_rng = torch.from_numpy(s.range.view(np.int32)).to(dev)
    d_int = torch.from_numpy(np.ascontiguousarray(s.intensity, dtype=np.float32)).to(dev)
    d_tab = torch.from_numpy(table).to(dev)
    torch.cuda.synchronize()
    assert d_tab.data_ptr() % 16 == 0
    on_device = ScanData.range_image(d_rng.data_ptr(), w, h, intensity=d_int.data_ptr(), memspace=capi.MEM_DEVICE, col_tfs=d_tab.data_ptr())
    on_host = ScanData.range_image(s.range, w, h, intensity=np.ascontiguousarray(s.intensity, dtype=np.float32), col_tfs=table)

    def one(scan, on):
        """(device ms of the raycast kernel, wall ms of the call, voxels the pass touched)"""
        assert det.set_raycast_motion(on) == capi.OK
        prof(det)
        t0 = time.perf_counter()
        assert det.raycast_begin(scan, s.tf) == capi.OK
        wall = (time.perf_counter() - t0) * 1e3
        p = prof(det)
        kern, other = ("k_raycast_motion", "k_raycast") if on else ("k_raycast", "k_raycast_motion")
        assert p.get(kern, (0, 0))[1] == 1 and other not in p, p
        touched = int(np.count_nonzero(det.read_map(capi.MAP_RAYCAST)))
        det.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,))
        return p[kern][0], wall, touched

    det.lib.profile_enable(det.h, 1)
    ms = {"k_raycast": [], "k_raycast_motion": []}
    wall = {"rigid_host_begin": [], "motion_host_begin": []}
    touched = {}
    for i in range(args.pairs + 1):  # (the first pair warms up and is dropped)
        for on, kern in ((False, "k_raycast"), (True, "k_raycast_motion")):
            t, _, touched[kern] = one(on_device, on)
            if i:
                ms[kern].append(t)
    for i in range(args.pairs + 1):
        for on, leg in ((False, "rigid_host_begin"), (True, "motion_host_begin")):
            _, t, _ = one(on_host, on)
            if i:
                wall[leg].append(t)
    det.lib.profile_enable(det.h, 0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratio = med["k_raycast_motion"] / med["k_raycast"]
    print(json.dumps({
        "tool": "raycast_motion_bench", "sensor": args.sensor, "rays": h * w, "voxel_size": args.voxel_size, "map_warm_scans": args.map_warm_scans, "pairs": args.pairs,
        "kernel": {"device_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "device_ms_median": {k: round(v, 4) for k, v in med.items()},
                   "motion_over_rigid": round(ratio, 3), "expectation": "<= 1.10", "met": bool(ratio <= 1.10), "voxels_touched": touched},
        "begin_host_scan_wall_ms": {k: [round(x, 3) for x in v] for k, v in wall.items()},
        "begin_host_scan_wall_ms_median": {k: round(statistics.median(v), 3) for k, v in wall.items()},
    }))
    det.close()


if __name__ == "__main__":
    main()
