"""vofod_map_render_scans at the shapes of tools/map_render_bench.py: k_map_render_scans with a pose table per view, without and with
the verdict and the counts, beside k_map_render of the same views - of this tree and, with --parent-lib, of a library built from the
parent commit.  Writes profiles/r30_map_render_scans.txt (first line: the summary DESIGN.md quotes, then one JSON line per shape) -
or to --out.

OS1-128 at 0.25 m on bench.py's warmed map with 1 / 16 / 64 views, then OS2-128 x 2048 at 0.1 m with one view (--big 0 leaves it
out); max_distance = raycast__max_distance, threshold = thresholds/new_obstacles, tolerance one voxel.  View v is the bench's frame
v: its pose, its measured range column (device memory, stride 4) and a table of `width` poses that moves the sensor from frame v's
pose to frame v + 1's while the scan is taken (vofod_column_poses, device memory, 16-byte aligned).  Per figure: the median over
--rounds calls of the kernel's device time from the library's profiler (vofod_profile_read), render outputs in device memory.  The
parent's library renders the same map (copied over with vofod_write_map) from the same poses; its spread over its calls
((max - min) / median) is the margin its figure gets.
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
from vofod_amd.detector import ScanData, VoFOD, column_poses, default_params  # noqa: E402

F = np.float32


def prof(det):
    names, ms, calls = (C.c_char * (64 * 128))(), (C.c_double * 128)(), (C.c_uint64 * 128)()
    n = det.lib.profile_read(det.h, names, ms, calls, 128)
    return {names[64 * i : 64 * i + 64].split(b"\0", 1)[0].decode(): (float(ms[i]), int(calls[i])) for i in range(n)}


def older_library(path):
    """a library that may lack the newest entry points (the parent commit's): bound as far as it goes"""
    lib = capi.Library.__new__(capi.Library)
    try:
        lib.__init__(path, "vofod_")
    except ImportError:
        pass
    return lib


def timed(det, name, call, args):
    ms = []
    for r in range(args.warmup + args.rounds):
        det.lib.profile_enable(det.h, 1)
        call()
        p = prof(det)
        det.lib.profile_enable(det.h, 0)
        assert list(p) == [name] and p[name][1] == 1, p
        if r >= args.warmup:
            ms.append(p[name][0])
    med = statistics.median(ms)
    return {"kernel_ms_median": round(med, 4), "kernel_ms": [round(x, 4) for x in ms], "spread": round((max(ms) - min(ms)) / med, 4)}


def measure(args, sensor, voxel_size, warm_scans, view_counts, pool, torch, dev, parent):
    lib = vofod_amd.library()
    h, w, vfov_deg, _ = synth.SENSORS[sensor]
    n = h * w

    def make(lb):
        sp, dp = default_params(lb)
        sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = voxel_size, w, h, 1
        sp.sensor_vfov = F(np.deg2rad(vfov_deg))
        return VoFOD(lb, sp, dp)

    det = make(lib)
    scene = synth.bench_scene()
    synth.warm_map(det, scene, sensor, warm_scans, pmap=pool.map)
    nmax = max(view_counts)
    frames = synth.bench_frames(scene, sensor, nmax + 1, 0, pmap=pool.map)
    tfs = np.stack([s.tf for s in frames]).astype(F)
    thr, length, tol = float(det.dp.voxel_map__thresholds__new_obstacles), float(det.dp.raycast__max_distance), float(voxel_size)
    old = None
    if parent is not None:
        old = make(parent)
        old.write_map(capi.MAP_VOXELS, det.read_map())
    total = nmax * n
    d_range, d_voxel = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev)
    d_what, d_tio, d_verdict = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(2 * total, dtype=torch.float32, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
    out4 = (d_range.data_ptr(), d_voxel.data_ptr(), d_what.data_ptr(), d_tio.data_ptr())
    keep, scans = [], []
    for v in range(nmax):
        rng = torch.from_numpy(np.ascontiguousarray(frames[v].scan.range, np.uint32).view(np.int32)).to(dev)
        tab = torch.from_numpy(column_poses(lib, tfs[v], tfs[v + 1], tfs[v], w).reshape(-1)).to(dev)
        assert tab.data_ptr() % 16 == 0
        keep += [rng, tab]
        scans.append(ScanData.range_image(rng.data_ptr(), w, h, memspace=capi.MEM_DEVICE, col_tfs=tab.data_ptr()))
    res = {"sensor": sensor, "voxel_size": voxel_size, "map": list(det.map_size), "map_MB": round(det.n_voxels * 4 / 1e6, 1), "warm_scans": warm_scans, "threshold": thr, "max_distance": length,
           "tolerance": tol, "views": {}}
    for nv in view_counts:
        arr = (capi.Scan * nv)(*[s.as_c() for s in scans[:nv]])
        tf_nv = np.ascontiguousarray(tfs[:nv]).reshape(-1)
        counts = np.zeros((nv, 8), np.uint32)
        head = (arr, capi.ptr(tf_nv), nv, C.c_float(thr), C.c_float(length), C.c_float(tol), *(C.c_void_p(a) for a in out4))
        rigid = (capi.ptr(tf_nv), nv, C.c_float(thr), C.c_float(length), *(C.c_void_p(a) for a in out4), C.c_int32(capi.MEM_DEVICE))

        def ok(st):
            assert st == capi.OK, st

        per = {"k_map_render": timed(det, "k_map_render", lambda: ok(lib.map_render(det.h, *rigid)), args)}
        if old is not None:
            per["k_map_render_parent"] = timed(old, "k_map_render", lambda: ok(parent.map_render(old.h, *rigid)), args)
        per["scans_tables"] = timed(det, "k_map_render_scans", lambda: ok(lib.map_render_scans(det.h, *head, None, None, C.c_int32(capi.MEM_DEVICE))), args)
        per["scans_tables_verdict_counts"] = timed(det, "k_map_render_scans", lambda: ok(lib.map_render_scans(det.h, *head, C.c_void_p(d_verdict.data_ptr()), capi.ptr(counts), C.c_int32(capi.MEM_DEVICE))), args)
        per["counts"] = counts.sum(axis=0).tolist()
        assert (counts.sum(axis=1) == n).all()
        res["views"][str(nv)] = per
    det.close()
    if old is not None:
        old.close()
    return res


def summary(results):
    parts = []
    for r in results:
        bits = []
        for nv, per in r["views"].items():
            ref = per.get("k_map_render_parent", per["k_map_render"])
            us = lambda k: per[k]["kernel_ms_median"] * 1e3
            ratio = lambda k: per[k]["kernel_ms_median"] / ref["kernel_ms_median"]
            bits.append(f"{nv} view{'s' if nv != '1' else ''}: `k_map_render` of the parent's library {ref['kernel_ms_median'] * 1e3:.1f} us (spread over its twelve calls {ref['spread'] * 100:.1f} %), of this "
                        f"tree {us('k_map_render'):.1f} us (x {ratio('k_map_render'):.3f}); `k_map_render_scans` with tables {us('scans_tables'):.1f} us (x {ratio('scans_tables'):.3f}), with tables, verdict and "
                        f"counts {us('scans_tables_verdict_counts'):.1f} us (x {ratio('scans_tables_verdict_counts'):.3f})")
        last = r["views"][max(r["views"], key=int)]["counts"]
        parts.append(f"{r['sensor']} at {r['voxel_size']} m ({r['map'][0]} x {r['map'][1]} x {r['map'][2]} voxels, {r['map_MB']} MB, warmed by {r['warm_scans']} scans), threshold {r['threshold']}, max_distance "
                     f"{r['max_distance']} m, tolerance {r['tolerance']} m: " + "; ".join(bits) + "; verdicts at the most views: " + ", ".join(f"{c} {k}" for k, c in zip(("none", "agree", "empty", "nearer", "through", "missing", "beyond"), last)))
    return "measured: " + ". ".join(parts) + ".\n" + "".join(json.dumps(r) + "\n" for r in results)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--map-warm-scans", type=int, default=96)
    ap.add_argument("--big", type=int, default=1, help="also OS2-128 x 2048 at 0.1 m, one view")
    ap.add_argument("--big-warm-scans", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libvofod_hip.so built from the parent commit: its k_map_render is the reference")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r30_map_render_scans.txt"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("map_render_scans_bench.py needs a GPU: no timing without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    parent = older_library(args.parent_lib) if args.parent_lib else None
    pool = ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn"))
    results = [measure(args, "os1-128", 0.25, args.map_warm_scans, (1, 16, 64), pool, torch, dev, parent)]
    if args.big:
        results.append(measure(args, "os2-128x2048", 0.1, args.big_warm_scans, (1,), pool, torch, dev, parent))
    pool.shutdown()
    text = summary(results)
    if Path(args.out).exists():
        text += "".join(l + "\n" for l in Path(args.out).read_text().splitlines() if l.startswith(("resources: ", "bench: ", "mutations: ", "suite: ")))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
