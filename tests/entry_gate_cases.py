"""Which call is admitted in which handle state: the states, the calls and the handle of tests/test_gpu_entry_gate.py, shared with
tools/record_entry_refusals.py, which recorded tests/golden/entry_refusals.json with them.  Public API only (include/vofod.h
through vofod_amd.capi): the module runs unchanged on any commit of the library.

The smallest handle the library accepts comfortably: a 16 x 8 sensor, 0.5 m voxels, an operation area of 4 m (9 x 9 x 9 voxels),
max_batch_frames 1.  The handle is put into a state, then every entry point that takes a handle is called with valid minimal
arguments; what a call yields is (status, last error string or None when the status is OK).  A refused call leaves the handle
as it was, so the handle is kept: the statuses of REFUSALS are answered in front of anything that changes the handle, and the
entries of READS change nothing whatever they answer.  After every other answer the state is rebuilt on a fresh handle.  (The
error string of a status that sets none is the one the handle held before: the order of CALLS is part of the record.)
vofod_broadcast_map is left out: it needs a communicator, and its local refusal is the one of vofod_map_apply."""
import ctypes as C
import os
import tempfile
from pathlib import Path

import numpy as np

from vofod_amd import capi

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "entry_refusals.json"
W, H = 16, 8
VS = 0.5
AREA = 4.0
N_PX = W * H
IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)

STATES = ["idle", "ticket_0_in_flight", "only_ticket_1_in_flight", "raycast_rigid_pending", "raycast_exact_pending", "sepclusters_pending", "world_enabled"]


def params(lib):
    sp, dp = capi.StaticParams(), capi.DynParams()
    lib.default_params(C.byref(sp), C.byref(dp))
    sp.voxel_size = VS
    for a in range(3):
        sp.oparea_size[a] = AREA
        sp.oparea_offset[a] = 0.0
        sp.exclude_offset[a] = 0.0
        sp.exclude_size[a] = 0.5
    sp.oparea_offset[2] = -AREA / 2  # (the z offset is the area's floor: the map is centred on the origin)
    sp.sensor_hrays, sp.sensor_vrays = W, H
    sp.sensor_vfov = np.float32(np.deg2rad(30.0))
    sp.max_batch_frames = 1
    dp.sepclusters__min_sure_points = 1
    return sp, dp


class Inputs:
    """every argument of every call, built once and kept alive (a submitted batch reads its scans until it is collected)"""

    def __init__(self, lib):
        self.sp, self.dp = params(lib)
        dirs = np.zeros((N_PX, 3), np.float32)
        assert lib.sim_lut(W, H, self.sp.sensor_vfov, capi.ptr(dirs)) == capi.OK
        self.range_mm = np.full(N_PX, 1500, np.uint32)
        self.xyz = [np.ascontiguousarray(dirs[:, a] * np.float32(1.5)) for a in range(3)]
        self.intensity = np.full(N_PX, 100.0, np.float32)
        self.col_tfs = np.ascontiguousarray(np.tile(IDENT, (W, 1)))
        self.points = self._scan(points=True)
        self.ranges = self._scan(points=False)
        self.moving = self._scan(points=True, col_tfs=True)
        self.tf = IDENT.copy()
        self.n_vox = (int(np.ceil(AREA / VS)) + 1) ** 3
        self.map = np.full(self.n_vox, self.sp.score_init, np.float32)
        self.units = np.zeros(self.n_vox, np.uint32)
        self.background = self.map.copy().reshape(9, 9, 9)
        self.background[3:6, 3:6, 3:6] = 0.0  # 27 sure voxels: one cluster for a sepclusters pass
        self.background = self.background.reshape(-1)
        self.apriori = np.array([[0.6, 0.6, 0.6], [-0.6, 0.6, 0.1]], np.float32)
        self.view = capi.CloudView()
        self.view.x, self.view.y, self.view.z = (capi.ptr(a) for a in self.xyz)
        self.view.intensity = capi.ptr(self.intensity)
        self.view.stride_bytes, self.view.n, self.view.memspace = 4, N_PX, capi.MEM_HOST
        self.grid_out = np.zeros(N_PX, capi.POINT_XYZR)
        self.grid_keys = np.zeros(N_PX, np.uint32)
        self.grid = capi.GridDesc()
        self.cl_grid = capi.GridDesc()
        for a in range(3):
            self.cl_grid.leaf[a], self.cl_grid.offset[a], self.cl_grid.min_b[a], self.cl_grid.div_b[a] = VS, 0.0, 0, 2
        self.cl_pts = np.zeros(2, capi.POINT_XYZR)
        self.cl_pts["x"] = [0.25, 0.75]
        self.cl_pts["y"] = [0.25, 0.75]
        self.cl_pts["z"] = [0.25, 0.75]
        self.cl_keys = np.array([0, 7], np.uint32)
        self.cl_labels = np.zeros(2, np.uint32)
        self.dets = np.zeros(64, capi.DETECTION)
        self.per = np.zeros(1, np.uint32)
        self.pc = np.zeros((self.n_vox, 4), np.float32)
        self.out3 = [np.zeros(N_PX, np.float32) for _ in range(3)]
        self.wire = np.zeros(4096 + 24 * self.n_vox, np.uint8)
        self.world = np.zeros(8, np.float32)
        self.names, self.ms, self.calls = (C.c_char * (64 * 8))(), (C.c_double * 8)(), (C.c_uint64 * 8)()
        fd, self.cloud_file = tempfile.mkstemp(suffix=".xyz")
        with os.fdopen(fd, "w") as f:
            f.write("0.6 0.6 0.6\n-0.6 0.6 0.1\n")
        # a full snapshot of an idle handle of this geometry, for vofod_map_apply
        self.snapshot = None
        if hasattr(lib, "map_export"):
            h = create(lib, self)
            n = C.c_size_t(0)
            assert lib.map_export(h, capi.MAPS_ALL, capi.SNAPSHOT_FULL, capi.ptr(self.wire), self.wire.size, capi.MEM_HOST, C.byref(n)) == capi.OK
            self.snapshot = self.wire[: n.value].copy()
            lib.destroy(h)

    def _scan(self, points, col_tfs=False):
        s = capi.Scan()
        if points:
            s.x, s.y, s.z = (capi.ptr(a) for a in self.xyz)
        s.intensity, s.range = capi.ptr(self.intensity), capi.ptr(self.range_mm)
        s.stride_bytes, s.width, s.height, s.memspace = 4, W, H, capi.MEM_HOST
        if col_tfs:
            s.col_tfs = capi.ptr(self.col_tfs)
        return s

    def close(self):
        os.unlink(self.cloud_file)


def create(lib, inp):
    h = C.c_void_p()
    st = lib.create(C.byref(inp.sp), C.byref(inp.dp), C.byref(h))
    assert st == capi.OK, st
    return h


def _ok(st, what):
    assert st == capi.OK, f"{what}: status {st} while building a state"


def _submit(lib, inp, h):
    t = C.c_int(-1)
    _ok(lib.batch_submit(h, C.byref(inp.points), capi.ptr(inp.tf), 1, C.byref(t)), "batch_submit")
    return t.value


def _collect(lib, inp, h, ticket):
    n = C.c_size_t(0)
    return lib.batch_collect(h, ticket, capi.ptr(inp.dets), inp.dets.size, capi.ptr(inp.per), C.byref(n))


def enter(lib, inp, state):
    """a fresh handle in `state`"""
    h = create(lib, inp)
    if state == "ticket_0_in_flight":
        assert _submit(lib, inp, h) == 0
    elif state == "only_ticket_1_in_flight":
        assert (_submit(lib, inp, h), _submit(lib, inp, h)) == (0, 1)
        _ok(_collect(lib, inp, h, 0), "batch_collect")
    elif state in ("raycast_rigid_pending", "raycast_exact_pending"):
        if state == "raycast_exact_pending":
            _ok(lib.set_raycast_exact(h, 1), "set_raycast_exact")
        _ok(lib.raycast_begin(h, C.byref(inp.points), capi.ptr(inp.tf)), "raycast_begin")
    elif state == "sepclusters_pending":
        _ok(lib.write_map(h, capi.MAP_VOXELS, capi.ptr(inp.background), inp.n_vox), "write_map")
        sure = C.c_int(0)
        _ok(lib.sepclusters_begin(h, C.byref(sure)), "sepclusters_begin")
        assert sure.value == 1, "the sepclusters pass is not pending"
    elif state == "world_enabled":
        m = np.full(3, 8, np.int32)
        _ok(lib.world_enable(h, capi.ptr(m), capi.ptr(m), 64), "world_enable")
    else:
        assert state == "idle", state
    return h


def leave(lib, inp, h):
    """nothing of the handle is in flight when it is destroyed"""
    for t in range(8):
        _collect(lib, inp, h, t)
    lib.destroy(h)


def _export(lib, inp, h):
    n = C.c_size_t(0)
    return lib.map_export(h, capi.MAPS_ALL, capi.SNAPSHOT_FULL, capi.ptr(inp.wire), inp.wire.size, capi.MEM_HOST, C.byref(n))


def _shift(lib, inp, h):
    s = np.array([1, 0, 0], np.int32)
    o = np.array([VS, 0.0, -AREA / 2], np.float32)
    return lib.map_shift(h, capi.ptr(s), capi.ptr(o))


def _world_enable(lib, inp, h):
    m = np.full(3, 8, np.int32)
    return lib.world_enable(h, capi.ptr(m), capi.ptr(m), 64)


def _world_read(lib, inp, h):
    lo, size = np.zeros(3, np.int32), np.full(3, 2, np.int32)
    return lib.world_read(h, capi.ptr(lo), capi.ptr(size), capi.ptr(inp.world), 8)


def _n():
    return C.byref(C.c_size_t(0))


# (name, call(lib, inputs, handle) -> status), in the order they run in every state; a name is the entry point's, a suffix
# tells the map or the input it names
CALLS = [
    ("get_status", lambda l, i, h: l.get_status(h, C.byref(capi.StatusInfo()))),
    ("set_dynamic_params", lambda l, i, h: l.set_dynamic_params(h, C.byref(i.dp))),
    ("world_status", lambda l, i, h: l.world_status(h, C.byref(capi.WorldInfo()))),
    ("profile_enable", lambda l, i, h: l.profile_enable(h, 0)),
    ("profile_read", lambda l, i, h: 0 * l.profile_read(h, i.names, i.ms, i.calls, 8)),
    ("read_map:voxels", lambda l, i, h: l.read_map(h, capi.MAP_VOXELS, capi.ptr(i.map.copy()), i.n_vox)),
    ("read_map:raycast", lambda l, i, h: l.read_map(h, capi.MAP_RAYCAST, capi.ptr(i.map.copy()), i.n_vox)),
    ("voxels_as_pc:voxels", lambda l, i, h: l.voxels_as_pc(h, capi.MAP_VOXELS, -300.0, 1, capi.ptr(i.pc), i.n_vox, _n())),
    ("voxels_as_pc:raycast", lambda l, i, h: l.voxels_as_pc(h, capi.MAP_RAYCAST, 0.0, 1, capi.ptr(i.pc), i.n_vox, _n())),
    ("raycast_units", lambda l, i, h: l.raycast_units(h, capi.ptr(i.units), i.n_vox, C.byref(C.c_int32(0)))),
    ("world_read", _world_read),
    ("map_export", _export),
    ("detection_points", lambda l, i, h: l.detection_points(h, capi.POINTS_SYNC, None, 0, _n(), None, None, 0, _n(), capi.MEM_HOST)),
    ("reserve", lambda l, i, h: l.reserve(h, 2)),
    ("set_point_motion", lambda l, i, h: l.set_point_motion(h, 1)),
    ("set_raycast_motion", lambda l, i, h: l.set_raycast_motion(h, 1)),
    ("set_raycast_exact", lambda l, i, h: l.set_raycast_exact(h, 1)),
    ("set_column_shift", lambda l, i, h: l.set_column_shift(h, None)),
    ("write_map:voxels", lambda l, i, h: l.write_map(h, capi.MAP_VOXELS, capi.ptr(i.map), i.n_vox)),
    ("write_map:raycast", lambda l, i, h: l.write_map(h, capi.MAP_RAYCAST, capi.ptr(np.zeros(i.n_vox, np.float32)), i.n_vox)),
    ("write_map:raycast_short", lambda l, i, h: l.write_map(h, capi.MAP_RAYCAST, capi.ptr(np.zeros(i.n_vox, np.float32)), i.n_vox - 1)),
    ("update_ground", lambda l, i, h: l.update_ground(h, 1.0, 0.0, 100.0, capi.ptr(i.tf))),
    ("load_apriori", lambda l, i, h: l.load_apriori(h, capi.ptr(i.apriori), 2)),
    ("ingest_apriori", lambda l, i, h: l.ingest_apriori(h, i.cloud_file.encode(), capi.ptr(np.zeros(3, np.float32)), 0.0, capi.ptr(np.zeros(3, np.float32)), _n(), _n())),
    ("map_apply", lambda l, i, h: l.map_apply(h, capi.ptr(i.snapshot), i.snapshot.size, capi.MEM_HOST)),
    ("map_shift", _shift),
    ("world_enable", _world_enable),
    ("world_disable", lambda l, i, h: l.world_disable(h)),
    ("process_scan", lambda l, i, h: l.process_scan(h, C.byref(i.points), capi.ptr(i.tf), capi.SCAN_DEFAULT, capi.ptr(i.dets), i.dets.size, _n(), None)),
    ("process_scan:no_map_update", lambda l, i, h: l.process_scan(h, C.byref(i.points), capi.ptr(i.tf), capi.SCAN_NO_MAP_UPDATE, capi.ptr(i.dets), i.dets.size, _n(), None)),
    ("process_batch", lambda l, i, h: l.process_batch(h, C.byref(i.points), capi.ptr(i.tf), 1, capi.ptr(i.dets), i.dets.size, capi.ptr(i.per), _n(), None)),
    ("batch_submit", lambda l, i, h: l.batch_submit(h, C.byref(i.points), capi.ptr(i.tf), 1, C.byref(C.c_int(-1)))),
    ("batch_collect:0", lambda l, i, h: _collect(l, i, h, 0)),
    ("batch_collect:1", lambda l, i, h: _collect(l, i, h, 1)),
    ("range_to_points", lambda l, i, h: l.range_to_points(h, C.byref(i.ranges), *(capi.ptr(a) for a in i.out3), capi.MEM_HOST)),
    ("range_to_points:wrong_size", lambda l, i, h: l.range_to_points(h, C.byref(_narrow(i.ranges)), *(capi.ptr(a) for a in i.out3), capi.MEM_HOST)),
    ("deskew_points", lambda l, i, h: l.deskew_points(h, C.byref(i.moving), *(capi.ptr(a) for a in i.out3), capi.MEM_HOST)),
    ("raycast_begin", lambda l, i, h: l.raycast_begin(h, C.byref(i.points), capi.ptr(i.tf))),
    ("raycast_finish", lambda l, i, h: l.raycast_finish(h)),
    ("sepclusters_begin", lambda l, i, h: l.sepclusters_begin(h, C.byref(C.c_int(0)))),
    ("sepclusters_finish", lambda l, i, h: l.sepclusters_finish(h)),
    ("voxel_grid_weighted", lambda l, i, h: l.voxel_grid_weighted(h, C.byref(i.view), VS, 0, None, capi.ptr(i.grid_out), capi.ptr(i.grid_keys), N_PX, _n(), C.byref(i.grid))),
    ("voxel_grid_counted", lambda l, i, h: l.voxel_grid_counted(h, C.byref(i.view), VS, 50.0, capi.ptr(i.grid_out), capi.ptr(i.grid_keys), N_PX, _n(), C.byref(i.grid))),
    ("cluster", lambda l, i, h: l.cluster(h, capi.ptr(i.cl_pts), capi.ptr(i.cl_keys), C.byref(i.cl_grid), 2, 2 * VS, capi.ptr(i.cl_labels), _n())),
    ("reset", lambda l, i, h: l.reset(h)),
]


# answers that leave the handle as it was: every entry gives them in front of its first change of the handle
REFUSALS = (capi.ERR_BUSY, capi.ERR_NOT_PENDING, capi.ERR_SIZE_MISMATCH, capi.ERR_INVALID_ARG)
# entries that read the handle (set_dynamic_params: the parameters it holds already; profile_enable: off stays off)
READS = ("get_status", "set_dynamic_params", "world_status", "profile_enable", "profile_read", "read_map", "voxels_as_pc", "raycast_units", "world_read", "detection_points")


def _narrow(scan):
    """the scan with one column less: the size test of an entry that runs it in front of its busy test"""
    s = capi.Scan()
    C.memmove(C.byref(s), C.byref(scan), C.sizeof(capi.Scan))
    s.width = W - 1
    return s


def entry_of(call_name):
    return call_name.split(":", 1)[0]


def rows_of_state(lib, inp, state):
    """{call: [status, error string or None]} of one state; calls the library does not export are left out"""
    rows = {}
    h = enter(lib, inp, state)
    try:
        for name, call in CALLS:
            if not hasattr(lib, entry_of(name)):
                continue
            st = int(call(lib, inp, h))
            msg = lib.last_error_string(h)
            rows[name] = [st, None if st == capi.OK else (msg.decode() if msg else "")]
            if st not in REFUSALS and entry_of(name) not in READS:
                leave(lib, inp, h)
                h = None
                h = enter(lib, inp, state)
    finally:
        if h is not None:
            leave(lib, inp, h)
    return rows


def table(lib, inp):
    """{state: rows_of_state}"""
    return {state: rows_of_state(lib, inp, state) for state in STATES}
