"""vofod_detection_pixels at the benchmark's shape: what the raw returns of a batch's detections cost, beside their byte model and
beside vofod_detection_points on the same batch.  Writes profiles/r26_detection_pixels.txt (first line: the summary DESIGN.md
quotes, then one JSON line per scene) - or to --out.

256 x OS1-128 at 0.25 m on the warmed map, device-resident columns, a collected ticket; the default scene of bench.py and the
12-target scene of its `loaded_tail` leg.  Per scene, the median of `--rounds` whole calls, each between two HIP events, outputs in
device memory (the sizes are asked for once, outside the clock: the sizing kernel's launch is reported on its own), and the device
times of k_det_pixel_sizes / k_det_pixels / k_det_points from vofod_profile_read in runs of their own.
Byte model: the frame's three columns read once per detection, plus the outputs (20 B per pixel, 16 B per detection).
A report, not a gate."""
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
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r26_detection_pixels.txt"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("detection_pixels_bench.py needs a GPU: no timing without one")
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
    scenes = {"default": synth.bench_scene(), f"targets_{args.targets}": synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=args.targets)}
    frames = {k: synth.bench_frames(sc, args.sensor, F, 0, pmap=pool.map) for k, sc in scenes.items()}
    pool.shutdown()
    med = statistics.median
    results = []
    for name, fr in frames.items():
        xyz = torch.empty((F, 3, n_pts), dtype=torch.float32)
        for f, s in enumerate(fr):
            xyz[f, 0], xyz[f, 1], xyz[f, 2] = torch.from_numpy(s.x), torch.from_numpy(s.y), torch.from_numpy(s.z)
        xyz = xyz.to(dev)
        torch.cuda.synchronize()
        scans = [ScanData(x=xyz[f, 0].data_ptr(), y=xyz[f, 1].data_ptr(), z=xyz[f, 2].data_ptr(), width=w, height=h, memspace=capi.MEM_DEVICE) for f in range(F)]
        tfs = np.stack([s.tf for s in fr]).astype(np.float32)
        tk = det.batch_submit(scans, tfs)
        dets, _ = det.batch_collect(tk)
        # sizes: the first query after the collect launches the sizing kernel
        det.lib.profile_enable(det.h, 1)
        n_span, n_px = C.c_size_t(0), C.c_size_t(0)
        assert det.lib.detection_pixels(det.h, tk, None, 0, C.byref(n_span), None, None, None, 0, C.byref(n_px), capi.MEM_HOST) == capi.OK
        sizing = prof(det).get("k_det_pixel_sizes", (0.0, 0))
        det.lib.profile_enable(det.h, 0)
        n_det, n_pix = n_span.value, n_px.value
        n_mem = int(dets["n_points"].sum())
        assert n_det == len(dets)
        d_px, d_member = torch.empty(max(n_pix, 1), dtype=torch.int32, device=dev), torch.empty(max(n_pix, 1), dtype=torch.int32, device=dev)
        d_xyz = torch.empty(max(3 * n_pix, 1), dtype=torch.float32, device=dev)
        d_pts, d_idx = torch.empty(max(4 * n_mem, 1), dtype=torch.float32, device=dev), torch.empty(max(n_mem, 1), dtype=torch.int32, device=dev)

        def pixels():
            return det.detection_pixels(tk, device_out=(d_px.data_ptr(), d_member.data_ptr(), d_xyz.data_ptr(), n_pix))

        def points():
            return det.detection_points(tk, device_out=(d_pts.data_ptr(), d_idx.data_ptr(), n_mem))

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()  # (waits for the workspace's stream itself: the second event is recorded behind the device work)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        def kernel_ms(call, kernel):
            det.lib.profile_enable(det.h, 1)
            call()
            k = prof(det).get(kernel, (0.0, 0))
            det.lib.profile_enable(det.h, 0)
            assert k[1] == 1, (kernel, k)
            return k[0]

        for _ in range(args.warmup):
            pixels(), points()
        t_px, t_pt, k_px, k_pt = [], [], [], []
        for _ in range(args.rounds):
            t_px.append(timed(pixels))
            t_pt.append(timed(points))
            k_px.append(kernel_ms(pixels, "k_det_pixels"))
            k_pt.append(kernel_ms(points, "k_det_points"))
        span = pixels()[0]
        assert int(span["count"].sum()) == n_pix
        model = 12 * n_pts * n_det + 20 * n_pix + 16 * n_det
        results.append({
            "scene": name, "frames": F, "sensor": args.sensor, "voxel_size": args.voxel_size, "detections": n_det, "member_voxels": n_mem, "pixels": n_pix,
            "detection_pixels": {"call_ms_median": round(med(t_px), 4), "call_ms": [round(x, 4) for x in t_px], "k_det_pixels_ms_median": round(med(k_px), 4),
                                 "k_det_pixel_sizes_ms": round(sizing[0], 4), "byte_model_bytes": model, "byte_model_ms_at_4_TBs": round(model / 4e12 * 1e3, 4),
                                 "kernel_GBps_on_model": round(model / (med(k_px) * 1e-3) / 1e9, 1) if med(k_px) > 0 else None},
            "detection_points": {"call_ms_median": round(med(t_pt), 4), "call_ms": [round(x, 4) for x in t_pt], "k_det_points_ms_median": round(med(k_pt), 4)},
        })
    det.close()
    parts = []
    for r in results:
        a, b = r["detection_pixels"], r["detection_points"]
        parts.append(f"{r['scene']} scene, {r['detections']} detections of {r['member_voxels']} voxels and {r['pixels']} returns per {r['frames']}-frame step: `vofod_detection_pixels` "
                     f"{a['call_ms_median']:.3f} ms per call (`k_det_pixels` {a['k_det_pixels_ms_median']:.3f} ms, the sizing kernel once per batch {a['k_det_pixel_sizes_ms']:.3f} ms) beside a byte model of "
                     f"{a['byte_model_bytes'] / 1e6:.1f} MB = {a['byte_model_ms_at_4_TBs']:.3f} ms at 4 TB/s ({a['kernel_GBps_on_model']} GB/s in the kernel); `vofod_detection_points` "
                     f"{b['call_ms_median']:.3f} ms (`k_det_points` {b['k_det_points_ms_median']:.3f} ms)")
    text = "measured: " + "; ".join(parts) + ".\n" + "".join(json.dumps(r) + "\n" for r in results)
    # (the lines of the file that other runs wrote - the bench.py comparison, the mutation record - stay)
    if Path(args.out).exists():
        text += "".join(l + "\n" for l in Path(args.out).read_text().splitlines() if l.startswith(("bench: ", "mutations: ", "suite: ")))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
