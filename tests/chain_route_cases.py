"""Which kernels a call launches: the calls, the settings and the handles of tests/test_gpu_chain_routes.py, shared with
tools/record_chain_routes.py, which recorded tests/golden/chain_routes.json with them.  Public API only (vofod_amd.detector,
include/vofod.h): the module runs unchanged on any commit of the library.

One OS1-16 at 0.5 m (16 x 1024 points: the voxel capacity lies above FAR_MAX, so a single scan may cluster close first), a
fresh handle per setting with a warmed map, and a further handle whose map knows nothing - every voxel of its first scan is far,
more than the close-first path takes: CF_RETRY, the full clustering behind it, and the latch that keeps the next calls there.
At 0.5 m a 4x4x4 brick is no clique for the clustering tolerance: those handles cluster at voxel level.  A third handle of the
same sensor at 0.25 m, warmed the same way, takes the brick kernels, the LDS clustering and the frame kernel.
Every call is bracketed by the library's profiler; what a case yields is {profiler label: launches}.  Nothing is compared against
the oracle here: parity is the other tests' job."""
import ctypes as C
import os
import re
import shlex
from pathlib import Path

import numpy as np

from vofod_amd import capi, synth
from vofod_amd.detector import VoFOD, default_params

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "chain_routes.json"
SENSOR, VS = "os1-16", 0.5
VS_BRICKS = 0.25  # a voxel size at which the clustering runs on bricks
MAX_BATCH = 128
N_WARM = 4
N_FRAMES = 8  # distinct frames: the larger batches repeat them


def settings():
    """default, every entry of the fallback matrix's ALL list, and the two switches that change a kernel's work, not the route"""
    text = (ROOT / "tools" / "run_fallback_matrix.sh").read_text()
    entries = shlex.split(re.search(r"^ALL=\((.*)\)$", text, re.M).group(1))
    out = [e or "default" for e in entries]
    assert out[0] == "default" and len(out) == len(set(out)), out
    return out + ["VOFOD_LEAN_EMIT=0", "VOFOD_LDS_MAX_BRICKS=64"]


def setting_env(setting):
    """{variable: value} of a setting's name"""
    return {} if setting == "default" else dict(kv.split("=", 1) for kv in setting.split())


def outside_switches():
    """VOFOD_* variables of the environment other than the harness self-check's: set from outside, they move every route"""
    return sorted(k for k in os.environ if k.startswith("VOFOD_") and k != "VOFOD_TEST_HARNESS_SELFCHECK")


class Inputs:
    """scans and clouds of every case, built once: warm-up scans of the scene without targets, frames of the scene with them"""

    def __init__(self):
        self.warm_scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=0)
        self.scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=3)
        self.apriori = {vs: synth.apriori_points(self.warm_scene, vs) for vs in (VS, VS_BRICKS)}
        self.warm = synth.scan_sequence(self.warm_scene, SENSOR, N_WARM, seed0=synth.BENCH_WARM_SEED0)
        self.frames = synth.bench_frames(self.scene, SENSOR, N_FRAMES)
        self.stream = synth.scan_sequence(self.scene, SENSOR, 4, seed0=40)

    def batch(self, n):
        fr = [self.frames[f % N_FRAMES] for f in range(n)]
        return [s.scan for s in fr], np.stack([s.tf for s in fr])


def _handle(lib, vs=VS):
    h, w, vfov_deg, _ = synth.SENSORS[SENSOR]
    sp, dp = default_params(lib)
    sp.voxel_size = vs
    sp.sensor_hrays, sp.sensor_vrays = w, h
    sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
    sp.max_batch_frames = MAX_BATCH
    return VoFOD(lib, sp, dp)


def warmed_handle(lib, inp, vs=VS):
    """surveyed background (both latches), the ground below the sensor, N_WARM map-updating scans, and the voxels they left
    unknown declared free (the stand-in for a long raycast history): targets that appear afterwards are far, and few"""
    det = _handle(lib, vs)
    det.load_apriori(inp.apriori[vs])
    synth.seed_ground(det)
    for s in inp.warm:
        det.process_scan(s.scan, s.tf)
    m = det.read_map(capi.MAP_VOXELS)
    m[m == np.float32(det.sp.score_init)] = np.float32(det.dp.voxel_map__thresholds__frontiers)
    det.write_map(capi.MAP_VOXELS, m)
    return det


def brick_handle(lib, inp):
    return warmed_handle(lib, inp, VS_BRICKS)


def cold_handle(lib, inp):
    """a map without any background, at 0.25 m: nothing is close, a scan's far voxels can outnumber FAR_MAX"""
    return _handle(lib, VS_BRICKS)


def _scan(det, inp, k, **kw):
    s = inp.stream[k]
    return det.process_scan(s.scan, s.tf, **kw)


def _submitted(det, inp, n):
    scans, tfs = inp.batch(n)
    return det.batch_collect(det.batch_submit(scans, tfs))


def _grid_cloud(inp):
    s = inp.frames[0]
    keep = (s.x != 0) | (s.y != 0) | (s.z != 0)
    return s.x[keep], s.y[keep], s.z[keep]


def _cluster(det, inp):
    pts, keys, grid, _ = det.voxel_grid_weighted(*_grid_cloud(inp), VS)
    return det.cluster(pts, keys, grid, 2.0 * VS)


def _sepclusters(det, inp):
    st, sure = det.sepclusters_begin(allow=(capi.ERR_EMPTY,))
    if st == capi.OK and sure:
        det.sepclusters_finish()


# (name, call) in the order they run on the warmed handle of a setting
WARM_CALLS = [
    ("scan", lambda d, i: _scan(d, i, 0)),
    ("scan_debug", lambda d, i: _scan(d, i, 1, debug=True)),
    ("scan_auto_raycast", lambda d, i: _scan(d, i, 2, flags=capi.SCAN_AUTO_RAYCAST)),
    ("batch_3", lambda d, i: d.process_batch(*i.batch(3))),
    ("batch_4", lambda d, i: d.process_batch(*i.batch(4))),
    ("batch_7", lambda d, i: d.process_batch(*i.batch(7))),
    ("batch_8", lambda d, i: d.process_batch(*i.batch(8))),
    ("batch_4_debug", lambda d, i: d.process_batch(*i.batch(4), debug=True)),
    ("batch_4_far_only", lambda d, i: d.process_batch(*i.batch(4), debug=True, far_only=True)),
    ("submit_4", lambda d, i: _submitted(d, i, 4)),
    ("submit_128", lambda d, i: _submitted(d, i, 128)),
    ("voxel_grid_weighted", lambda d, i: d.voxel_grid_weighted(*_grid_cloud(i), VS)),
    ("voxel_grid_counted", lambda d, i: d.voxel_grid_counted(*_grid_cloud(i), np.ones(len(_grid_cloud(i)[0]), np.float32), VS, 0.5)),
    ("cluster", _cluster),
    ("sepclusters_begin", _sepclusters),
]
# ... and on the cold one.  As recorded: the first scan still fits the close-first path, the SECOND one raises CF_RETRY - both chains show in its launches, kernels_far.h and then the brick kernels - and
# sets the latch, under which the batch takes k_frame_lds_full.  (The names say what the calls were meant to meet.)
COLD_CALLS = [
    ("cold_scan_retry", lambda d, i: _scan(d, i, 0)),
    ("cold_scan_latched", lambda d, i: _scan(d, i, 1)),
    ("cold_batch_4_latched", lambda d, i: d.process_batch(*i.batch(4))),
]


# ... and on the warmed handle at 0.25 m
BRICK_CALLS = [
    ("bricks_scan", lambda d, i: _scan(d, i, 0)),
    ("bricks_scan_debug", lambda d, i: _scan(d, i, 1, debug=True)),
    ("bricks_batch_3", lambda d, i: d.process_batch(*i.batch(3))),
    ("bricks_batch_4", lambda d, i: d.process_batch(*i.batch(4))),
    ("bricks_batch_8", lambda d, i: d.process_batch(*i.batch(8))),
    ("bricks_batch_4_debug", lambda d, i: d.process_batch(*i.batch(4), debug=True)),
    ("bricks_batch_4_far_only", lambda d, i: d.process_batch(*i.batch(4), debug=True, far_only=True)),
    ("bricks_submit_4", lambda d, i: _submitted(d, i, 4)),
    ("bricks_submit_128", lambda d, i: _submitted(d, i, 128)),
]


def profiled(det, call):
    """{profiler label: launches} of one call (vofod_profile_read drains the list)"""
    lib = det.lib
    names, ms, calls = (C.c_char * (64 * 128))(), (C.c_double * 128)(), (C.c_uint64 * 128)()
    lib.profile_enable(det.h, 1)
    try:
        lib.profile_read(det.h, names, ms, calls, 128)  # (whatever an earlier call left)
        call()
        n = lib.profile_read(det.h, names, ms, calls, 128)
    finally:
        lib.profile_enable(det.h, 0)
    return {names[64 * i : 64 * i + 64].split(b"\0", 1)[0].decode(): int(calls[i]) for i in range(n)}


def routes_of_setting(lib, inp):
    """{call: {label: launches}} of every case under the switches the environment holds now: the handles are created, warmed and
    used under them"""
    out = {}
    for make, calls in ((warmed_handle, WARM_CALLS), (cold_handle, COLD_CALLS), (brick_handle, BRICK_CALLS)):
        det = make(lib, inp)
        try:
            for name, call in calls:
                out[name] = profiled(det, lambda: call(det, inp))
        finally:
            det.close()
    return out
