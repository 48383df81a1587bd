"""Rolling operation area (include/vofod.h vofod_map_shift): device time of k_map_shift per map at 0.25 m (OS1-128 defaults) and
0.1 m (OS2-128 x 2048), beside a device-to-device hipMemcpyAsync of one map in the same process - the yardstick: it moves the same
4 M + 4 M bytes and is not the code under test - and the host round trip the call replaces (read_map x 3, numpy shift,
write_map x 3).  Writes <out>/r14_map_shift.json and a short <out>/r14_map_shift.txt (kept as profiles/r14_map_shift.*).

Per configuration, after an untimed shift that allocates the spare buffer: REPS shifts with s0 % 4 == 0 (every 16-byte load of the
kernel aligned) and REPS with s0 % 4 != 0 (4-byte aligned loads), there and back so that the offset does not wander.  Kernel times
come from the library's HIP-event profiler (vofod_profile_read: three launches per call, one per map), the copy is bracketed by
HIP events of the same kind, host times are the wall clock of the call.
PASS CONDITION: the aligned shift of one map takes no more than 1.2 x the device-to-device copy.  The unaligned case and the ratio
to the host round trip are recorded, not gated."""
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
from vofod_amd import capi, synth  # noqa: E402
from vofod_amd.detector import VoFOD, default_params  # noqa: E402

REPS = 5
GATE = 1.2
MAPS = (capi.MAP_VOXELS, capi.MAP_FLAGS, capi.MAP_RAYCAST)


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


def hip_runtime():
    """the HIP runtime the product library was loaded with (for the yardstick copy)"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    rt = C.CDLL(path)
    for name, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]), ("hipMemset", [C.c_void_p, C.c_int, C.c_size_t]),
                       ("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventDestroy", [C.c_void_p]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                       ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
                       ("hipMemcpyAsync", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]), ("hipDeviceSynchronize", [])):
        fn = getattr(rt, name)
        fn.argtypes, fn.restype = args, C.c_int
    return rt


def chk(st, what):
    if st != 0:
        raise RuntimeError(f"{what}: hipError {st}")


def copy_yardstick(rt, nbytes, reps):
    """ms of hipMemcpyAsync device-to-device of nbytes, between two HIP events, `reps` times after one untimed copy: the yardstick
    (one source, one destination, every time) and, recorded beside it, the same copy walking round four buffers as the maps and the
    spare of a shift do (at 0.25 m two buffers fit into the 256 MB of last-level cache, four do not)"""
    bufs = [C.c_void_p() for _ in range(4)]
    e0, e1 = C.c_void_p(), C.c_void_p()
    for b in bufs:
        chk(rt.hipMalloc(C.byref(b), nbytes), "hipMalloc")
        chk(rt.hipMemset(b, 0x5A, nbytes), "hipMemset")
    chk(rt.hipEventCreate(C.byref(e0)), "hipEventCreate")
    chk(rt.hipEventCreate(C.byref(e1)), "hipEventCreate")
    out = {"fixed": [], "rotating": []}
    try:
        for mode in ("fixed", "rotating"):
            for r in range(reps + 1):
                src, dst = (bufs[0], bufs[1]) if mode == "fixed" else (bufs[r % 4], bufs[(r + 1) % 4])
                chk(rt.hipEventRecord(e0, None), "hipEventRecord")
                chk(rt.hipMemcpyAsync(dst, src, nbytes, 3, None), "hipMemcpyAsync")  # 3 = hipMemcpyDeviceToDevice
                chk(rt.hipEventRecord(e1, None), "hipEventRecord")
                chk(rt.hipEventSynchronize(e1), "hipEventSynchronize")
                ms = C.c_float(0)
                chk(rt.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
                if r:
                    out[mode].append(float(ms.value))
    finally:
        rt.hipEventDestroy(e0)
        rt.hipEventDestroy(e1)
        for b in bufs:
            rt.hipFree(b)
    return out["fixed"], out["rotating"]


def np_shift(a, s, init):
    """the statement of vofod_map_shift on [sz, sy, sx] with slices"""
    out = np.full_like(a, init)
    dst, src = [], []
    for axis, sa in zip((2, 1, 0), s):
        n = a.shape[axis]
        lo, hi = max(0, -sa), min(n, n - sa)
        if hi <= lo:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo + sa, hi + sa))
    out[dst[2], dst[1], dst[0]] = a[src[2], src[1], src[0]]
    return out


def offset_of(base, k, vs):
    return tuple(float(np.float32(b + int(kk) * vs)) for b, kk in zip(base, k))


def shift_case(det, base, k, s, vs, reps):
    """`reps` times s and back; per call: (k_map_shift ms summed over the three maps, wall ms)"""
    dev, wall = [], []
    for r in range(2 * reps):
        step = s if r % 2 == 0 else tuple(-v for v in s)
        k += np.array(step)
        prof(det)
        t0 = time.perf_counter()
        det.map_shift(step, offset_of(base, k, vs))
        wall.append((time.perf_counter() - t0) * 1e3)
        p = prof(det)
        ms, calls = p.get("k_map_shift", (0.0, 0))
        assert calls == 3, p
        dev.append(ms)
    return dev, wall


def run_config(lib, rt, name, sensor, vs):
    det = make(lib, sensor, vs)
    M = det.n_voxels
    base = tuple(float(v) for v in det.sp.oparea_offset)
    det.load_apriori(synth.apriori_points(synth.bench_scene(), max(vs, 0.25)))  # (something in the map; the copy does not look at it)
    k = np.zeros(3, dtype=np.int64)
    # untimed: allocates the spare buffer
    for step in ((4, 0, 0), (-4, 0, 0)):
        k += np.array(step)
        det.map_shift(step, offset_of(base, k, vs))
    det.lib.profile_enable(det.h, 1)
    al_dev, al_wall = shift_case(det, base, k, (4, 0, 0), vs, REPS)
    un_dev, un_wall = shift_case(det, base, k, (1, 0, 0), vs, REPS)
    gen_dev, gen_wall = shift_case(det, base, k, (3, -2, 1), vs, REPS)
    det.lib.profile_enable(det.h, 0)
    copy_ms, copy_rot_ms = copy_yardstick(rt, 4 * M, REPS)
    # the round trip the call replaces, on the same handle (once: it is seconds at 0.1 m)
    t0 = time.perf_counter()
    arrs = [det.read_map(m) for m in MAPS]
    t1 = time.perf_counter()
    arrs = [np_shift(a, (4, 0, 0), np.float32(det.sp.score_init if m == capi.MAP_VOXELS else 0.0)) for m, a in zip(MAPS, arrs)]
    t2 = time.perf_counter()
    for m, a in zip(MAPS, arrs):
        det.write_map(m, a)
    t3 = time.perf_counter()
    del arrs
    det.close()
    med = statistics.median
    per_map = lambda dev: med(dev) / 3.0  # noqa: E731
    tbs = lambda ms: round(8 * M / (ms * 1e-3) / 1e12, 3)  # noqa: E731
    out = {
        "config": name, "sensor": sensor, "voxel_size": vs, "M": M, "bytes_moved_per_map": 8 * M, "reps": 2 * REPS,
        "aligned": {"shift": [4, 0, 0], "k_map_shift_ms_per_map": round(per_map(al_dev), 4), "tbs": tbs(per_map(al_dev)), "k_map_shift_ms_per_call": [round(v, 4) for v in al_dev],
                    "call_wall_ms_median": round(med(al_wall), 3)},
        "unaligned": {"shift": [1, 0, 0], "k_map_shift_ms_per_map": round(per_map(un_dev), 4), "tbs": tbs(per_map(un_dev)), "k_map_shift_ms_per_call": [round(v, 4) for v in un_dev],
                      "call_wall_ms_median": round(med(un_wall), 3)},
        "three_axes": {"shift": [3, -2, 1], "k_map_shift_ms_per_map": round(per_map(gen_dev), 4), "tbs": tbs(per_map(gen_dev)), "call_wall_ms_median": round(med(gen_wall), 3)},
        "memcpy_d2d_one_map": {"ms_median": round(med(copy_ms), 4), "tbs": tbs(med(copy_ms)), "ms": [round(v, 4) for v in copy_ms]},
        "memcpy_d2d_round_four_buffers": {"ms_median": round(med(copy_rot_ms), 4), "tbs": tbs(med(copy_rot_ms)), "ms": [round(v, 4) for v in copy_rot_ms]},
        "host_round_trip": {"read_ms": round((t1 - t0) * 1e3, 2), "numpy_shift_ms": round((t2 - t1) * 1e3, 2), "write_ms": round((t3 - t2) * 1e3, 2), "total_ms": round((t3 - t0) * 1e3, 2)},
    }
    out["aligned_over_memcpy"] = round(per_map(al_dev) / med(copy_ms), 3)
    out["unaligned_over_memcpy"] = round(per_map(un_dev) / med(copy_ms), 3)
    out["host_round_trip_over_call"] = round(out["host_round_trip"]["total_ms"] / med(al_wall), 1)
    out["pass"] = bool(out["aligned_over_memcpy"] <= GATE)
    return out


def text(res):
    lines = ["vofod_map_shift: k_map_shift per map against a device-to-device hipMemcpyAsync of one map (tools/map_shift_bench.py, one MI355X)",
             f"medians of {2 * REPS} calls (HIP events); the kernel and the copy both move 4 M + 4 M bytes per map", ""]
    for c in res["configs"]:
        a, u, g, y, h = c["aligned"], c["unaligned"], c["three_axes"], c["memcpy_d2d_one_map"], c["host_round_trip"]
        lines += [
            f"{c['config']}: {c['sensor']} @ {c['voxel_size']} m, M = {c['M']:,} voxels",
            f"  k_map_shift, s = (4, 0, 0), aligned loads     {a['k_map_shift_ms_per_map']:9.4f} ms per map  {a['tbs']:6.3f} TB/s",
            f"  k_map_shift, s = (1, 0, 0), 4-byte aligned    {u['k_map_shift_ms_per_map']:9.4f} ms per map  {u['tbs']:6.3f} TB/s",
            f"  k_map_shift, s = (3, -2, 1)                   {g['k_map_shift_ms_per_map']:9.4f} ms per map  {g['tbs']:6.3f} TB/s",
            f"  hipMemcpyAsync device to device, one map      {y['ms_median']:9.4f} ms           {y['tbs']:6.3f} TB/s   (the yardstick: one source, one destination)",
            f"  the same copy round four buffers              {c['memcpy_d2d_round_four_buffers']['ms_median']:9.4f} ms           {c['memcpy_d2d_round_four_buffers']['tbs']:6.3f} TB/s   (recorded: as the maps and the spare of a shift rotate)",
            f"  aligned / copy = {c['aligned_over_memcpy']:.3f} (gate: <= {GATE}): {'PASS' if c['pass'] else 'MISSED'};  unaligned / copy = {c['unaligned_over_memcpy']:.3f} (recorded, not gated)",
            f"  whole call, three maps, wall clock            {a['call_wall_ms_median']:9.3f} ms (aligned)  {u['call_wall_ms_median']:9.3f} ms (unaligned)",
            f"  host round trip it replaces                   {h['total_ms']:9.2f} ms = read {h['read_ms']} + numpy {h['numpy_shift_ms']} + write {h['write_ms']}: {c['host_round_trip_over_call']} x the call",
            "",
        ]
    lines.append("verdict on the 1.2 x condition: " + ("met at every configuration" if res["pass"] else "MISSED at " + ", ".join(c["config"] for c in res["configs"] if not c["pass"])))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=("025", "01"), default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles"), help="directory of r14_map_shift.json / .txt")
    args = ap.parse_args()
    lib = vofod_amd.library()
    rt = hip_runtime()
    res = {"tool": "map_shift_bench", "gate": GATE, "warmup": "one untimed shift there and back per configuration (allocates the spare buffer)", "configs": []}
    if args.only in (None, "025"):
        res["configs"].append(run_config(lib, rt, "0.25 m", "os1-128", 0.25))
    if args.only in (None, "01"):
        res["configs"].append(run_config(lib, rt, "0.1 m", "os2-128x2048", 0.1))
    res["pass"] = all(c["pass"] for c in res["configs"])
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "r14_map_shift.json").write_text(json.dumps(res) + "\n")
    (out / "r14_map_shift.txt").write_text(text(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
