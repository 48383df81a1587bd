"""Map snapshots and deltas (include/vofod.h vofod_map_export / vofod_map_apply): times and effective bandwidth of the export and
apply paths at 0.25 m (OS1-128, configs[2]) and 0.1 m (OS2-128 x 2048, configs[4]), beside the dense read_map + write_map host
round trip.  Prints one JSON line (recorded as profiles/r06_map_sync.json).

Cases per configuration and maps mask (voxel map alone, all three maps): a full snapshot, a delta after one scan, a delta after
a raycast pass (the scan whose VOFOD_SCAN_AUTO_RAYCAST finishes the pass begun by the one before), each applied to a replica,
after an untimed warm-up that allocates the handles' shadows and staging buffers.
Device times come from the library's HIP-event profiler (vofod_profile_read), host times from the wall clock of the call.
Bytes model: count pass 8 M per map with a shadow (map + shadow), 4 M against init; emit pass 8 D plus the tiles it re-reads
(a full snapshot re-reads and copies the whole map: + 8 M); apply 8 D (+ 4 M of init fill for a full snapshot)."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import vofod_amd  # noqa: E402
from vofod_amd import capi, mapsync, synth  # noqa: E402
from vofod_amd.detector import VoFOD, default_params  # noqa: E402

TILE = 8192  # voxels per tile of the count pass (mapsync.h MS_TILE)


def make(lib, sensor, vs):
    h, w, vfov_deg, _ = synth.SENSORS[sensor]
    sp, dp = default_params(lib)
    sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = vs, w, h, 1
    sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
    return VoFOD(lib, sp, dp)


def prof(det):
    names, ms, calls = (C.c_char * (64 * 128))(), (C.c_double * 128)(), (C.c_uint64 * 128)()
    n = det.lib.profile_read(det.h, names, ms, calls, 128)
    return {names[64 * i : 64 * i + 64].split(b"\0", 1)[0].decode(): (float(ms[i]), int(calls[i])) for i in range(n)}


def timed(det, fn):
    prof(det)
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    return out, wall, prof(det)


def tbs(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e12, 3) if ms > 0 else None


def export_case(own, rep, maps, full, label, M):
    kind = capi.SNAPSHOT_FULL if full else capi.SNAPSHOT_DELTA
    n_maps = bin(maps).count("1")
    # count pass alone (size queries: nothing changes), five times
    cnt_ms = []
    for _ in range(5):
        n = C.c_size_t(0)
        _, _, p = timed(own, lambda: own.lib.map_export(own.h, maps, kind, None, 0, capi.MEM_HOST, C.byref(n)))
        cnt_ms.append(p.get("k_ms_count", (0.0, 0))[0])
    buf, wall, p = timed(own, lambda: own.export_map(maps, full))
    snap = mapsync.decode(buf)
    D = sum(len(r[0]) for r in snap.records.values())
    count_bytes = (4 if full else 8) * M * n_maps
    emit_ms = p.get("k_ms_emit", (0.0, 0))[0]
    tiles = 0
    for m, (idx, _) in snap.records.items():
        tiles += len(np.unique(idx // TILE)) if len(idx) else 0
    emit_bytes = 8 * D + (8 * M * n_maps if full else 8 * min(tiles * TILE, M))
    _, awall, ap = timed(rep, lambda: rep.apply_map(buf))
    apply_dev = sum(ap.get(k, (0.0, 0))[0] for k in ("k_ms_check", "k_ms_scatter", "k_fill", "k_ms_count"))
    apply_bytes = 8 * D + (4 * M * n_maps if full else 0)
    return {
        "case": label, "maps": maps, "kind": "full" if full else "delta", "records": D, "bytes": int(buf.size),
        "count_ms_median": round(statistics.median(cnt_ms), 4), "count_tbs": tbs(count_bytes, statistics.median(cnt_ms)),
        "count_bytes_model": count_bytes,
        "emit_ms": round(emit_ms, 4), "emit_tbs": tbs(emit_bytes, emit_ms), "emit_bytes_model": emit_bytes, "tiles_with_records": tiles,
        "export_wall_ms": round(wall, 3),
        "apply_device_ms": round(apply_dev, 4), "apply_tbs": tbs(apply_bytes, apply_dev), "apply_bytes_model": apply_bytes,
        "apply_wall_ms": round(awall, 3),
        "apply_kernels": {k: round(v[0], 4) for k, v in ap.items()},
    }


def run_config(lib, name, sensor, vs, warm):
    own, rep = make(lib, sensor, vs), make(lib, sensor, vs)
    M = own.n_voxels
    scans = warm(own, sensor, vs)
    for d in (own, rep):
        d.lib.profile_enable(d.h, 1)
    k = 0

    def settle():
        nonlocal k
        if own.status().raycast_pending:  # (a chain starts with no raycast pass pending)
            own.process_scan(scans[k].scan, scans[k].tf, flags=capi.SCAN_AUTO_RAYCAST)
            k += 1

    # warm-up, not recorded: the first exports and applies of a handle allocate its shadows and staging buffers (hipMalloc);
    # one pass of the all-maps sequence sizes them for the timed cases below
    settle()
    rep.apply_map(own.export_map(capi.MAPS_ALL, full=True))
    for _ in range(2):
        own.process_scan(scans[k].scan, scans[k].tf, flags=capi.SCAN_AUTO_RAYCAST)
        k += 1
        rep.apply_map(own.export_map(capi.MAPS_ALL, full=False))
    cases = []
    for maps in (1 << capi.MAP_VOXELS, capi.MAPS_ALL):
        lab = "voxels" if maps == 1 else "all"
        settle()
        cases.append(export_case(own, rep, maps, True, f"{lab}/full", M))
        own.process_scan(scans[k].scan, scans[k].tf, flags=capi.SCAN_AUTO_RAYCAST)  # begins a raycast pass
        k += 1
        cases.append(export_case(own, rep, maps, False, f"{lab}/delta_one_scan", M))
        own.process_scan(scans[k].scan, scans[k].tf, flags=capi.SCAN_AUTO_RAYCAST)  # finishes it: the sweep changes the map
        k += 1
        cases.append(export_case(own, rep, maps, False, f"{lab}/delta_after_raycast", M))
    # the dense host round trip of the same maps
    dense = {}
    for maps in (1, capi.MAPS_ALL):
        sel = [m for m in range(3) if (maps >> m) & 1]
        t0 = time.perf_counter()
        arrs = [own.read_map(m) for m in sel]
        t1 = time.perf_counter()
        for m, a in zip(sel, arrs):
            rep.write_map(m, a)
        t2 = time.perf_counter()
        dense["voxels" if maps == 1 else "all"] = {"read_ms": round((t1 - t0) * 1e3, 2), "write_ms": round((t2 - t1) * 1e3, 2), "total_ms": round((t2 - t0) * 1e3, 2),
                                                   "bytes": 4 * M * len(sel)}
        del arrs
    for c in cases:
        lab = c["case"].split("/")[0]
        total = c["export_wall_ms"] + c["apply_wall_ms"]
        c["speedup_vs_dense_round_trip"] = round(dense[lab]["total_ms"] / total, 1) if total > 0 else None
    own.close()
    rep.close()
    return {"config": name, "sensor": sensor, "voxel_size": vs, "M": M, "cases": cases, "dense_host_round_trip": dense}


def warm_025(det, sensor, vs):
    scene = synth.make_scene(21, n_targets=3)
    det.load_apriori(synth.apriori_points(scene, vs, n_voxels=1_000_000, solid_ground_to=-1.2))
    scans = synth.scan_sequence(scene, sensor, 18, seed0=300)
    for s in scans[:4]:
        det.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
    return scans[4:]


def warm_01(det, sensor, vs):
    gx, gy = np.meshgrid(np.arange(-20, 30, vs), np.arange(-20, 30, vs), indexing="ij")
    pts = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.01)], axis=1).astype(np.float32)
    det.load_apriori(pts[np.hypot(pts[:, 0], pts[:, 1]) < 30])
    scans = synth.scan_sequence(synth.bench_scene(), sensor, 14, seed0=1000)
    for s in scans[:2]:
        det.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
    return scans[2:]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=("025", "01"), default=None)
    args = ap.parse_args()
    lib = vofod_amd.library()
    out = {"tool": "map_sync_bench", "warmup": "one untimed full + two deltas of all maps per configuration (allocations)", "configs": []}
    if args.only in (None, "025"):
        out["configs"].append(run_config(lib, "configs[2]", "os1-128", 0.25, warm_025))
    if args.only in (None, "01"):
        out["configs"].append(run_config(lib, "configs[4]", "os2-128x2048", 0.1, warm_01))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
