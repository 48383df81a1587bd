"""vofod_map_render at the benchmark's shape: the kernel's time for 1, 16 and 64 views and for bursts of K = 1, 2, 4, 8 steps, beside
k_raycast of the same scan.  Writes profiles/r27_map_render.txt (first line: the summary DESIGN.md quotes, then one JSON line per
configuration) - or to --out.

OS1-128 at 0.25 m on bench.py's warmed map, max_distance = raycast__max_distance, threshold = thresholds/new_obstacles, the poses
of the bench's first frames (view 0: the pose of frame 0, whose scan is the yardstick's).  Per (views, K): the median over --rounds
calls of k_map_render's device time from the library's profiler (vofod_profile_read), outputs in device memory, and - in calls of
their own with the profiler off - the time of the C call vofod_map_render itself (arguments marshalled beforehand) on the host clock,
which ends in the call's own synchronisation.
Yardstick: k_raycast of frame 0's scan through vofod_raycast_begin in the same process, from the same profiler.
rays x mean steps per second: the mean number of voxels looked at per ray is counted by a vectorised numpy walk of a sample of the
rays of the 64 views (the float32 expressions of include/vofod.h), which is also compared with the device's `what` for those rays.
Then the same at OS2-128 x 2048 / 0.1 m with one view (--big 0 leaves it out).  Not measured: PMC counters of the kernel.
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
from vofod_amd.detector import VoFOD, default_params  # noqa: E402

F = np.float32
BURSTS = (1, 2, 4, 8)
KEPT = 8  # vmr::MR_BURST of map_render.h


def prof(det):
    names, ms, calls = (C.c_char * (64 * 128))(), (C.c_double * 128)(), (C.c_uint64 * 128)()
    n = det.lib.profile_read(det.h, names, ms, calls, 128)
    return {names[64 * i : 64 * i + 64].split(b"\0", 1)[0].decode(): (float(ms[i]), int(calls[i])) for i in range(n)}


def count_steps(det, dirs, tfs, pick, m, thr, length):
    """voxels looked at per ray and `what`, for the rays `pick` = (view, pixel) pairs: the walk of include/vofod.h, all rays at once"""
    sx, sy, sz = det.map_size
    off, vs = np.asarray(det.map_offset, F), F(det.sp.voxel_size)
    size = np.array([sx, sy, sz])
    tf = tfs[pick[0]].reshape(-1, 3, 4).astype(F)
    d = dirs[pick[1]].astype(F)
    with np.errstate(all="ignore"):
        dir_ = np.stack([((tf[:, k, 0] * d[:, 0]) + (tf[:, k, 1] * d[:, 1])) + (tf[:, k, 2] * d[:, 2]) for k in range(3)], axis=1)
        start = tf[:, :, 3]  # (the simulated LUT has no offsets)
        cur = np.floor((start - off) * (F(1.0) / vs)).astype(np.int64)
        step = np.sign(dir_).astype(np.int64)
        last = np.where(step > 0, size - 1, 0)
        ad = np.abs(dir_)
        tdelta = (F(1.0) / ad) * vs
        ctr = ((cur.astype(F) + F(0.5)) * vs) + off
        tmax = ((vs / F(2.0)) + (step.astype(F) * (ctr - start))) / ad
        n = len(d)
        what = np.zeros(n, np.uint8)
        steps = np.zeros(n, np.int64)
        live = ((cur >= 0) & (cur < size)).all(axis=1)
        flat = m.reshape(-1)
        rows = np.arange(n)
        while live.any():
            a = np.where(tmax[:, 1] < tmax[:, 0], 1, 0)
            a = np.where(tmax[:, 2] < tmax[rows, a], 2, a)
            dist = tmax[rows, a]
            lin = (cur[:, 2] * sy + cur[:, 1]) * sx + cur[:, 0]
            steps += live
            hit = live & (flat[np.where(live, lin, 0)] > F(thr))
            end = live & ~hit & ~(dist < F(length))
            left = live & ~hit & ~end & (cur[rows, a] == last[rows, a])
            what[hit], what[end], what[left] = capi.RENDER_HIT, capi.RENDER_END, capi.RENDER_LEFT
            live = live & ~hit & ~end & ~left
            cur[rows[live], a[live]] += step[rows[live], a[live]]
            tmax[rows[live], a[live]] = tmax[rows[live], a[live]] + tdelta[rows[live], a[live]]
    return steps, what


def measure(args, sensor, voxel_size, warm_scans, view_counts, pool, torch, dev):
    lib = vofod_amd.library()
    h, w, vfov_deg, _ = synth.SENSORS[sensor]
    n = h * w
    sp, dp = default_params(lib)
    sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = voxel_size, w, h, 1
    sp.sensor_vfov = F(np.deg2rad(vfov_deg))
    det = VoFOD(lib, sp, dp)
    scene = synth.bench_scene()
    synth.warm_map(det, scene, sensor, warm_scans, pmap=pool.map)
    frames = synth.bench_frames(scene, sensor, max(view_counts), 0, pmap=pool.map)
    tfs = np.stack([s.tf for s in frames]).astype(F)
    thr, length = float(dp.voxel_map__thresholds__new_obstacles), float(dp.raycast__max_distance)
    med = statistics.median
    # ---- the yardstick: k_raycast of frame 0's scan (the pass is abandoned: no detection ran in between, the map stays)
    k_ray = []
    for r in range(args.warmup + args.rounds):
        det.lib.profile_enable(det.h, 1)
        det.raycast_begin(frames[0].scan, frames[0].tf)
        p = prof(det)
        det.lib.profile_enable(det.h, 0)
        det.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION, capi.ERR_RAYCAST_EMPTY))
        if r >= args.warmup:
            k_ray.append(p["k_raycast"][0])
    res = {"sensor": sensor, "voxel_size": voxel_size, "map": list(det.map_size), "map_MB": round(det.n_voxels * 4 / 1e6, 1), "warm_scans": warm_scans, "threshold": thr, "max_distance": length,
           "k_raycast_ms_median": round(med(k_ray), 4), "k_raycast_ms": [round(x, 4) for x in k_ray], "views": {}}
    total = max(view_counts) * n
    d_range, d_voxel = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev)
    d_what, d_tio = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(2 * total, dtype=torch.float32, device=dev)
    out = (d_range.data_ptr(), d_voxel.data_ptr(), d_what.data_ptr(), d_tio.data_ptr())
    for nv in view_counts:
        per = {}
        for K in BURSTS:
            os.environ["VOFOD_RENDER_BURST"] = str(K)
            # the C entry itself, its arguments marshalled once outside the clock (no numpy conversion, no Python wrapper in the time)
            tf_nv = np.ascontiguousarray(tfs[:nv]).reshape(-1)
            c_args = (det.h, capi.ptr(tf_nv), nv, C.c_float(thr), C.c_float(length), *(C.c_void_p(a) for a in out), C.c_int32(capi.MEM_DEVICE))
            fn = det.lib.map_render

            def call():
                assert fn(*c_args) == capi.OK

            kern, wall = [], []
            for r in range(args.warmup + args.rounds):
                det.lib.profile_enable(det.h, 1)
                call()
                p = prof(det)
                det.lib.profile_enable(det.h, 0)
                assert list(p) == ["k_map_render"] and p["k_map_render"][1] == 1, p
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                if r >= args.warmup:
                    kern.append(p["k_map_render"][0])
                    wall.append((t1 - t0) * 1e3)
            per[str(K)] = {"kernel_ms_median": round(med(kern), 4), "kernel_ms": [round(x, 4) for x in kern], "call_wall_ms_median": round(med(wall), 4)}
        res["views"][str(nv)] = per
    os.environ.pop("VOFOD_RENDER_BURST", None)
    # ---- what the views see, and the steps of a sample of their rays
    nv = max(view_counts)
    det.map_render(tfs[:nv], thr, length, out=out)
    what = d_what.cpu().numpy()[: nv * n].reshape(nv, n)
    res["what_counts"] = {k: int((what == v).sum()) for k, v in (("not_cast", 0), ("hit", 1), ("end", 2), ("left", 3))}
    rng = np.random.default_rng(0)
    pick = (rng.integers(0, nv, args.sample), rng.integers(0, n, args.sample))
    dirs = synth.sim_lut(w, h, float(F(np.deg2rad(vfov_deg))))
    steps, what_np = count_steps(det, dirs, tfs, pick, det.read_map(), thr, length)
    assert (what_np == what[pick]).all(), "the numpy walk and the device disagree on the sampled rays"
    res["mean_steps_sample"] = round(float(steps.mean()), 2)
    res["sample"] = args.sample
    best = min(BURSTS, key=lambda K: res["views"][str(nv)][str(K)]["kernel_ms_median"])
    res["ray_steps_per_s_at_max_views"] = {str(K): round(nv * n * steps.mean() / (res["views"][str(nv)][str(K)]["kernel_ms_median"] * 1e-3) / 1e9, 2) for K in BURSTS}  # G steps/s
    res["fastest_K_at_max_views"] = best
    det.close()
    return res


def summary(results):
    """the record's first line and the JSON lines; the call's time and the step rate are quoted at the burst length the library keeps"""
    parts = []
    for r in results:
        bits = []
        for nv, per in r["views"].items():
            bits.append(f"{nv} view{'s' if nv != '1' else ''}: " + " / ".join(f"{per[str(K)]['kernel_ms_median'] * 1e3:.1f}" for K in BURSTS) + " us for K = 1 / 2 / 4 / 8"
                        + f" (the C call on the host clock at K = {KEPT}: {per[str(KEPT)]['call_wall_ms_median'] * 1e3:.0f} us)")
        nvmax = max(r["views"], key=int)
        parts.append(f"{r['sensor']} at {r['voxel_size']} m ({r['map'][0]} x {r['map'][1]} x {r['map'][2]} voxels, {r['map_MB']} MB, warmed by {r['warm_scans']} scans), threshold {r['threshold']}, max_distance "
                     f"{r['max_distance']} m: `k_map_render` " + "; ".join(bits) + f"; `k_raycast` of the same scan {r['k_raycast_ms_median'] * 1e3:.1f} us; {r['mean_steps_sample']} voxels looked at per ray "
                     f"(sample of {r['sample']}), {r['ray_steps_per_s_at_max_views'][str(KEPT)]} G ray steps/s at {nvmax} view{'s' if nvmax != '1' else ''} and K = {KEPT}; pixels: "
                     + ", ".join(f"{v} {k}" for k, v in r["what_counts"].items()))
    return "measured: " + ". ".join(parts) + ".  Not measured: PMC counters of the kernel.\n" + "".join(json.dumps(r) + "\n" for r in results)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--map-warm-scans", type=int, default=96)
    ap.add_argument("--big", type=int, default=1, help="also OS2-128 x 2048 at 0.1 m, one view")
    ap.add_argument("--big-warm-scans", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=32768)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r27_map_render.txt"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("map_render_bench.py needs a GPU: no timing without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    results = [measure(args, "os1-128", 0.25, args.map_warm_scans, (1, 16, 64), pool, torch, dev)]
    if args.big:
        results.append(measure(args, "os2-128x2048", 0.1, args.big_warm_scans, (1,), pool, torch, dev))
    pool.shutdown()
    text = summary(results)
    if Path(args.out).exists():
        text += "".join(l + "\n" for l in Path(args.out).read_text().splitlines() if l.startswith(("resources: ", "bench: ", "mutations: ", "suite: ")))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
