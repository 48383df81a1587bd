"""Host-side mirror of the vofod::VoFOD nodelet interface for the per-scan hot path.

`VoFOD` wraps one `vofod_handle` of a `capi.Library` and exposes the same call
order the nodelet uses (vofod_nodelet.cpp:882-989): `process_scan` (= the body of
processMsg), `raycast_begin/finish` (= raycast_cloud :1397), `sepclusters_begin/
finish` (= updateSeparatedBGClusters :1126), `reset` (:1610), `load_apriori`
(:339-345).  Parameter names are those of config/detection_params.yaml.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from . import capi


class VofodError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str = ""):
        super().__init__(f"{what} failed with status {status}" + (f": {detail}" if detail else ""))
        self.status = status


@dataclass
class ScanData:
    """One organised scan.  Arrays are float32/uint32 of w*h elements (host numpy),
    or integer device addresses with `memspace=capi.MEM_DEVICE`."""

    x: object
    y: object
    z: object
    width: int
    height: int
    intensity: object = None
    range: object = None
    stride_bytes: int = 4
    memspace: int = capi.MEM_HOST
    stamp: float = 0.0
    col_tfs: object = None  # range images, and point scans under VoFOD.set_point_motion: float32 [width, 3, 4] (or a device address), a pose per measurement column

    @classmethod
    def range_image(cls, range, width: int, height: int, intensity=None, stride_bytes: int = 4, memspace: int = capi.MEM_HOST, stamp: float = 0.0, col_tfs=None) -> "ScanData":
        """A range image (include/vofod.h): no point columns, only the sensor's uint32 millimetres (`width * height` of them at
        `stride_bytes`, pixel order of the handle's LUT); the product library rebuilds the points on the device.  `col_tfs`: a
        C-contiguous float32 array of `width` row-major 3x4 poses in the scan's memspace (or a device address) - the scan is
        motion-compensated column by column (include/vofod.h, MOTION COMPENSATION)."""
        if isinstance(col_tfs, np.ndarray):
            assert col_tfs.dtype == np.float32 and col_tfs.flags["C_CONTIGUOUS"] and col_tfs.size == 12 * width, "col_tfs: float32, C order, width * 12 values"
        return cls(x=None, y=None, z=None, width=width, height=height, intensity=intensity, range=range, stride_bytes=stride_bytes, memspace=memspace, stamp=stamp, col_tfs=col_tfs)

    def as_c(self) -> capi.Scan:
        def p(a):
            if a is None:
                return None
            if isinstance(a, np.ndarray):
                return a.ctypes.data_as(C.c_void_p)
            return C.c_void_p(int(a))

        s = capi.Scan()
        s.x, s.y, s.z = p(self.x), p(self.y), p(self.z)
        s.intensity, s.range = p(self.intensity), p(self.range)
        s.stride_bytes = self.stride_bytes
        s.width, s.height = self.width, self.height
        s.memspace = self.memspace
        s.stamp = self.stamp
        s.col_tfs = p(self.col_tfs)
        return s


def default_params(lib: capi.Library) -> tuple[capi.StaticParams, capi.DynParams]:
    sp, dp = capi.StaticParams(), capi.DynParams()
    lib.default_params(C.byref(sp), C.byref(dp))
    return sp, dp


class VoFOD:
    def __init__(self, lib: capi.Library, sp: capi.StaticParams | None = None, dp: capi.DynParams | None = None,
                 lut_directions: np.ndarray | None = None, lut_offsets: np.ndarray | None = None, mask: np.ndarray | None = None):
        self.lib = lib
        dsp, ddp = default_params(lib)
        self.sp = sp if sp is not None else dsp
        self.dp = dp if dp is not None else ddp
        self._keep = []
        n = self.sp.sensor_hrays * self.sp.sensor_vrays
        for name, arr, dt, cnt in (("lut_directions", lut_directions, np.float32, 3 * n), ("lut_offsets", lut_offsets, np.float32, 3 * n), ("mask", mask, np.uint8, n)):
            if arr is not None:
                a = np.ascontiguousarray(arr, dtype=dt).reshape(-1)
                assert a.size == cnt, f"{name}: expected {cnt} elements, got {a.size}"
                self._keep.append(a)
                setattr(self.sp, name, a.ctypes.data_as(C.c_void_p))
        self._scan_arrays = {}
        self._pending = {}
        self._collect_bufs = {}
        self.h = C.c_void_p()
        st = lib.create(C.byref(self.sp), C.byref(self.dp), C.byref(self.h))
        if st != capi.OK:
            raise VofodError(st, "vofod_create")
        info = self.status()
        self.map_size = tuple(info.map_size)  # (sx, sy, sz)
        self.map_offset = tuple(info.map_offset)
        self.n_voxels = int(np.prod(self.map_size))

    # ------------------------------------------------------------ lifecycle
    def close(self):
        if self.h:
            self.lib.destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int, what: str, allow: Sequence[int] = ()):
        if st != capi.OK and st not in allow:
            msg = self.lib.last_error_string(self.h)
            raise VofodError(st, what, msg.decode() if msg else "")
        return st

    def reset(self):
        self._check(self.lib.reset(self.h), "vofod_reset")

    def set_dynamic_params(self, **kv):
        for k, v in kv.items():
            if not hasattr(self.dp, k):
                raise KeyError(k)
            setattr(self.dp, k, v)
        self._check(self.lib.set_dynamic_params(self.h, C.byref(self.dp)), "vofod_set_dynamic_params")

    def status(self) -> capi.StatusInfo:
        s = capi.StatusInfo()
        self._check(self.lib.get_status(self.h, C.byref(s)), "vofod_get_status")
        return s

    def load_apriori(self, xyz: np.ndarray, allow: Sequence[int] = ()):
        a = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        return self._check(self.lib.load_apriori(self.h, capi.ptr(a), a.shape[0]), "vofod_load_apriori", allow)

    def ingest_apriori(self, filename: str, tf_xyz=(0.0, 0.0, 0.0), yaw_deg: float = 0.0, sim_correction=(0.0, 0.0, 0.0)):
        """initialize_apriori_map from a .pts/.xyz file (apriori_map/tf/* of sim.yaml); returns (points loaded, voxels set)"""
        t = np.ascontiguousarray(tf_xyz, dtype=np.float32)
        c = np.ascontiguousarray(sim_correction, dtype=np.float32)
        nl, nv = C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.ingest_apriori(self.h, filename.encode(), capi.ptr(t), float(yaw_deg), capi.ptr(c), C.byref(nl), C.byref(nv)), "vofod_ingest_apriori")
        return nl.value, nv.value

    def update_ground(self, range_m: float, tf, min_range: float = 0.0, max_range: float = 100.0, allow=()):
        """height range-finder message (vofod_nodelet.cpp:581-613); returns the status (MAP_RANGE may be allowed)"""
        t = np.ascontiguousarray(tf, dtype=np.float32).reshape(12)
        st = self.lib.update_ground(self.h, float(range_m), float(min_range), float(max_range), capi.ptr(t))
        if st != capi.OK and st not in allow:
            self._check(st, "vofod_update_ground")
        return st

    def read_map(self, which: int = capi.MAP_VOXELS) -> np.ndarray:
        """Returns the map as [sz, sy, sx] (x fastest: voxel_map.cpp:81)."""
        out = np.empty(self.n_voxels, dtype=np.float32)
        self._check(self.lib.read_map(self.h, which, capi.ptr(out), out.size), "vofod_read_map")
        sx, sy, sz = self.map_size
        return out.reshape(sz, sy, sx)

    def voxels_as_pc(self, threshold: float, greater_than: bool = True, which: int = capi.MAP_VOXELS) -> np.ndarray:
        """VoxelMap::voxelsAsPC (voxel_map.cpp:157-183): [n, 4] float32 world centres + map value, x outer / y / z inner"""
        n = C.c_size_t(0)
        st = self.lib.voxels_as_pc(self.h, which, float(threshold), int(bool(greater_than)), None, 0, C.byref(n))
        if st not in (capi.OK, capi.ERR_CAPACITY):
            self._check(st, "vofod_voxels_as_pc")
        out = np.zeros((n.value, 4), dtype=np.float32)
        if n.value:
            self._check(self.lib.voxels_as_pc(self.h, which, float(threshold), int(bool(greater_than)), capi.ptr(out), n.value, C.byref(n)), "vofod_voxels_as_pc")
        return out

    def write_map(self, which: int, arr: np.ndarray):
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        self._check(self.lib.write_map(self.h, which, capi.ptr(a), a.size), "vofod_write_map")

    def map_shift(self, shift_voxels, new_oparea_offset, allow: Sequence[int] = ()):
        """Move the operation area by whole voxels (vofod_map_shift): new[ix, iy, iz] = old[ix + s0, iy + s1, iz + s2] inside the
        overlap, the maps' init values elsewhere; afterwards the handle is one created at `new_oparea_offset`.  Returns the status
        (one in `allow` leaves the handle as it was)."""
        s = np.ascontiguousarray(shift_voxels, dtype=np.int32).reshape(3)
        o = np.ascontiguousarray(new_oparea_offset, dtype=np.float32).reshape(3)
        st = self._check(self.lib.map_shift(self.h, capi.ptr(s), capi.ptr(o)), "vofod_map_shift", allow)
        if st == capi.OK:
            for a in range(3):
                self.sp.oparea_offset[a] = o[a]
            self.map_offset = tuple(self.status().map_offset)
        return st

    def map_render(self, tfs, threshold: float, max_distance: float, out=None, allow: Sequence[int] = ()):
        """The voxel map as the sensor would see it from each pose of `tfs` ([views, 3, 4] or one [3, 4]; vofod_map_render): returns
        (range, voxel, what, t_in_out) - uint32 millimetres (0: no hit), the hit voxel's linear index (capi.RENDER_NO_VOXEL: none),
        capi.RENDER_* as uint8, each [views, h, w], and the ray's piece inside the last voxel looked at as float32 [views, h, w, 2].
        `out` = (range, voxel, what, t_in_out) device addresses on the handle's device, None for an output left out: they are
        written in place and None comes back.  A status in `allow` is returned in place of the result."""
        t = np.ascontiguousarray(tfs, dtype=np.float32).reshape(-1, 12)
        nv, hh, ww = t.shape[0], int(self.sp.sensor_vrays), int(self.sp.sensor_hrays)
        if out is not None:
            ptrs = [None if a is None else C.c_void_p(int(a)) for a in out]
            st = self._check(self.lib.map_render(self.h, capi.ptr(t), nv, float(threshold), float(max_distance), *ptrs, capi.MEM_DEVICE), "vofod_map_render", allow)
            return None if st == capi.OK else st
        rng = np.zeros((nv, hh, ww), dtype=np.uint32)
        vox = np.zeros((nv, hh, ww), dtype=np.uint32)
        what = np.zeros((nv, hh, ww), dtype=np.uint8)
        tio = np.zeros((nv, hh, ww, 2), dtype=np.float32)
        st = self._check(self.lib.map_render(self.h, capi.ptr(t), nv, float(threshold), float(max_distance), capi.ptr(rng), capi.ptr(vox), capi.ptr(what), capi.ptr(tio), capi.MEM_HOST),
                         "vofod_map_render", allow)
        return (rng, vox, what, tio) if st == capi.OK else st

    def map_render_scans(self, scans, tfs, threshold: float, max_distance: float, tolerance: float = 0.0, out=None, allow: Sequence[int] = ()):
        """Scans against the map (vofod_map_render_scans): view v is `scans[v]` (ScanData; one with `col_tfs` is cast from a pose per
        measurement column) under `tfs[v]`.  Returns a namespace of range, voxel, what, t_in_out - shaped like map_render's - and
        verdict (capi.VERDICT_* as uint8 [views, h, w]) and counts (uint32 [views, 8]: the pixels of each verdict).  `out` =
        (range, voxel, what, t_in_out, verdict) device addresses on the handle's device, None for an output left out: they are
        written in place and come back as None; counts is host memory always.  Where a scan has no `range`, verdict and counts are None.  A status in `allow` is returned in place of the result."""
        from types import SimpleNamespace

        scans = [scans] if isinstance(scans, ScanData) else list(scans)
        t = np.ascontiguousarray(tfs, dtype=np.float32).reshape(-1, 12)
        nv, hh, ww = len(scans), int(self.sp.sensor_vrays), int(self.sp.sensor_hrays)
        assert t.shape[0] == nv, "one tf per scan"
        arr = (capi.Scan * nv)(*[s.as_c() for s in scans])
        compare = all(s.range is not None for s in scans)  # (scans without a range: the render alone, verdict and counts None)
        counts = np.zeros((nv, 8), dtype=np.uint32) if compare else None
        if out is not None:
            ptrs = [None if a is None else C.c_void_p(int(a)) for a in out]
            st = self._check(self.lib.map_render_scans(self.h, arr, capi.ptr(t), nv, float(threshold), float(max_distance), float(tolerance), *ptrs, capi.ptr(counts), capi.MEM_DEVICE),
                             "vofod_map_render_scans", allow)
            return SimpleNamespace(range=None, voxel=None, what=None, t_in_out=None, verdict=None, counts=counts) if st == capi.OK else st
        r = SimpleNamespace(range=np.zeros((nv, hh, ww), dtype=np.uint32), voxel=np.zeros((nv, hh, ww), dtype=np.uint32), what=np.zeros((nv, hh, ww), dtype=np.uint8),
                            t_in_out=np.zeros((nv, hh, ww, 2), dtype=np.float32), verdict=np.zeros((nv, hh, ww), dtype=np.uint8) if compare else None, counts=counts)
        st = self._check(self.lib.map_render_scans(self.h, arr, capi.ptr(t), nv, float(threshold), float(max_distance), float(tolerance), capi.ptr(r.range), capi.ptr(r.voxel),
                                                   capi.ptr(r.what), capi.ptr(r.t_in_out), capi.ptr(r.verdict), capi.ptr(r.counts), capi.MEM_HOST), "vofod_map_render_scans", allow)
        return r if st == capi.OK else st

    def map_match(self, scan: ScanData, tfs, threshold: float, allow: Sequence[int] = ()):
        """Candidate poses scored against the map (vofod_map_match): `scan` (a range image, with or without `col_tfs`, or a point
        scan) under every pose of `tfs` ([K, 3, 4] or one [3, 4]).  Returns a namespace of counts (uint32 [K, 4]: the pixels of each
        capi.MATCH_* class per candidate) and best (the smallest k with the most OCCUPIED pixels).  A status in `allow` is returned in
        place of the result."""
        from types import SimpleNamespace

        t = np.ascontiguousarray(tfs, dtype=np.float32).reshape(-1, 12)
        cs = scan.as_c()
        counts = np.zeros((t.shape[0], 4), dtype=np.uint32)
        best = C.c_int32(-1)
        st = self._check(self.lib.map_match(self.h, C.byref(cs), capi.ptr(t), t.shape[0], float(threshold), capi.ptr(counts), C.byref(best)), "vofod_map_match", allow)
        return SimpleNamespace(counts=counts, best=int(best.value)) if st == capi.OK else st

    def map_distance(self, threshold: float, radius: int, device=False, allow: Sequence[int] = ()):
        """The squared distance, in voxels, from every voxel to the nearest one above `threshold`, clamped at radius * radius
        (vofod_map_distance): uint16 [sz, sy, sx].  `device` = a device address on the handle's device (2-byte aligned, n_voxels
        uint16): the field is written in place and None comes back.  A status in `allow` is returned in place of the result."""
        if device is not False and device is not None:
            st = self._check(self.lib.map_distance(self.h, float(threshold), int(radius), C.c_void_p(int(device)), self.n_voxels, capi.MEM_DEVICE), "vofod_map_distance", allow)
            return None if st == capi.OK else st
        out = np.zeros(self.n_voxels, dtype=np.uint16)
        st = self._check(self.lib.map_distance(self.h, float(threshold), int(radius), capi.ptr(out), out.size, capi.MEM_HOST), "vofod_map_distance", allow)
        sx, sy, sz = self.map_size
        return out.reshape(sz, sy, sx) if st == capi.OK else st

    def map_match_field(self, scan: ScanData, tfs, d2, near2: int = 0, outside_cost: int = 0, allow: Sequence[int] = ()):
        """Candidate poses scored by a distance field (vofod_map_match_field): `scan` and `tfs` as for map_match; `d2` is a uint16
        array of n_voxels values (what map_distance returned, or any other field) or a device address of one.  Returns a namespace
        of counts (uint32 [K, 4]: the pixels of each capi.FIELD_* class per candidate), cost (uint64 [K]: the sum of d2 over the
        inside pixels plus outside_cost per OUTSIDE pixel) and best (the smallest k with the smallest cost).  A status in `allow` is
        returned in place of the result."""
        from types import SimpleNamespace

        t = np.ascontiguousarray(tfs, dtype=np.float32).reshape(-1, 12)
        cs = scan.as_c()
        counts = np.zeros((t.shape[0], 4), dtype=np.uint32)
        cost = np.zeros(t.shape[0], dtype=np.uint64)
        best = C.c_int32(-1)
        if isinstance(d2, np.ndarray):
            field = np.ascontiguousarray(d2, dtype=np.uint16).reshape(-1)
            f_ptr, f_n, f_mem = capi.ptr(field), field.size, capi.MEM_HOST
        else:
            f_ptr, f_n, f_mem = C.c_void_p(int(d2)), self.n_voxels, capi.MEM_DEVICE
        st = self._check(self.lib.map_match_field(self.h, C.byref(cs), capi.ptr(t), t.shape[0], f_ptr, f_n, f_mem, int(near2), int(outside_cost), capi.ptr(counts), capi.ptr(cost),
                                                  C.byref(best)), "vofod_map_match_field", allow)
        return SimpleNamespace(counts=counts, cost=cost, best=int(best.value)) if st == capi.OK else st

    # ---- world store (include/vofod.h, WORLD STORE): the voxel map as a window onto a sparse map of a larger box
    def world_enable(self, margin_lo, margin_hi, max_tiles: int, allow: Sequence[int] = ()):
        """The box is [-margin_lo, map_size + margin_hi) in world indices (voxels, the window's origin K = 0 now); the pool holds
        max_tiles tiles of 8 x 8 x 8 voxels (2 KiB each).  From here on map_shift writes what leaves into the store and reads what
        enters from it, and load_apriori stamps the points beyond the window."""
        lo = np.ascontiguousarray(margin_lo, dtype=np.int32).reshape(3)
        hi = np.ascontiguousarray(margin_hi, dtype=np.int32).reshape(3)
        return self._check(self.lib.world_enable(self.h, capi.ptr(lo), capi.ptr(hi), int(max_tiles)), "vofod_world_enable", allow)

    def world_disable(self, allow: Sequence[int] = ()):
        return self._check(self.lib.world_disable(self.h), "vofod_world_disable", allow)

    def world_info(self) -> capi.WorldInfo:
        out = capi.WorldInfo()
        self._check(self.lib.world_status(self.h, C.byref(out)), "vofod_world_status")
        return out

    def world_read(self, lo, size) -> np.ndarray:
        """W over the box of world indices [lo, lo + size) as float32 [size2, size1, size0] (x fastest)"""
        lo = np.ascontiguousarray(lo, dtype=np.int32).reshape(3)
        size = np.ascontiguousarray(size, dtype=np.int32).reshape(3)
        out = np.empty((int(size[2]), int(size[1]), int(size[0])), dtype=np.float32)
        self._check(self.lib.world_read(self.h, capi.ptr(lo), capi.ptr(size), capi.ptr(out), out.size), "vofod_world_read")
        return out

    def set_column_shift(self, shift_by_row=None, allow: Sequence[int] = ()):
        """vofod_set_column_shift: pixel (row, col) was measured in column (col + shift_by_row[row]) mod width; None = zeros"""
        sh = None if shift_by_row is None else np.ascontiguousarray(shift_by_row, dtype=np.int32).reshape(self.sp.sensor_vrays)
        return self._check(self.lib.set_column_shift(self.h, capi.ptr(sh)), "vofod_set_column_shift", allow)

    def set_raycast_motion(self, on: bool = True, allow: Sequence[int] = ()):
        """vofod_set_raycast_motion: with it on, raycast_begin and the raycast half of SCAN_AUTO_RAYCAST cast a scan that carries
        `col_tfs` ray by ray from the columns' poses; off (the state after creation) they cast the rigid rays"""
        return self._check(self.lib.set_raycast_motion(self.h, int(bool(on))), "vofod_set_raycast_motion", allow)

    def set_point_motion(self, on: bool = True, allow: Sequence[int] = ()):
        """vofod_set_point_motion: with it on, process_scan, process_batch and batch_submit accept a point scan that carries `col_tfs`
        and apply the columns' poses on the device (k_point_deskew); off (the state after creation) such a scan is refused"""
        return self._check(self.lib.set_point_motion(self.h, int(bool(on))), "vofod_set_point_motion", allow)

    def set_raycast_exact(self, on: bool = True, allow: Sequence[int] = ()):
        """vofod_set_raycast_exact: with it on, the raycast passes begun from now on sum fixed-point units in uint32 (order
        independent, bit-identical between handles fed the same scans); off (the state after creation) they sum floats"""
        return self._check(self.lib.set_raycast_exact(self.h, int(bool(on))), "vofod_set_raycast_exact", allow)

    def raycast_units(self, allow: Sequence[int] = ()):
        """vofod_raycast_units: (U as uint32 [sz, sy, sx], S) of the pending exact pass - a voxel holds U * 2**-S metres; with a
        status in `allow` returned by the call: (None, status)"""
        out = np.empty(self.n_voxels, dtype=np.uint32)
        s = C.c_int32(-1)
        st = self._check(self.lib.raycast_units(self.h, capi.ptr(out), out.size, C.byref(s)), "vofod_raycast_units", allow)
        if st != capi.OK:
            return None, st
        sx, sy, sz = self.map_size
        return out.reshape(sz, sy, sx), int(s.value)

    # ------------------------------------------------- snapshots and deltas
    def export_map(self, maps: int = capi.MAPS_ALL, full: bool = True) -> np.ndarray:
        """A full snapshot or a delta of the maps in `maps` (bitmask of 1 << capi.MAP_*) in the wire format of
        vofod_amd.mapsync (uint8).  A delta follows the last export of the same mask (VofodError ERR_DELTA_BASE without one)."""
        kind = capi.SNAPSHOT_FULL if full else capi.SNAPSHOT_DELTA
        n = C.c_size_t(0)
        self._check(self.lib.map_export(self.h, int(maps), kind, None, 0, capi.MEM_HOST, C.byref(n)), "vofod_map_export")
        while True:
            buf = np.empty(n.value, dtype=np.uint8)
            st = self.lib.map_export(self.h, int(maps), kind, capi.ptr(buf), buf.size, capi.MEM_HOST, C.byref(n))
            if st == capi.ERR_CAPACITY and n.value > buf.size:
                continue  # (the map changed between the size query and the export: another thread's scan)
            self._check(st, "vofod_map_export")
            return buf[: n.value]

    def apply_map(self, buf) -> None:
        """apply a snapshot or delta (bytes / uint8 array from export_map, a file or another process)"""
        b = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else buf, dtype=np.uint8).reshape(-1)
        self._check(self.lib.map_apply(self.h, capi.ptr(b), b.size, capi.MEM_HOST), "vofod_map_apply")

    def world_export(self, kind: int = capi.SNAPSHOT_FULL, device=False, allow: Sequence[int] = ()):
        """A full snapshot (capi.SNAPSHOT_FULL) or a delta (capi.SNAPSHOT_DELTA) of the world store in the wire format of
        vofod_amd.mapsync.decode_world, as a uint8 array.  `device` = (address, capacity in bytes) on the handle's device, 16-byte
        aligned: the record is written there - for a collective of the caller's - and its size in bytes comes back.  A delta follows
        this handle's last export (ERR_DELTA_BASE without one).  A status in `allow` is returned in place of the result.  Without
        `device` the library is asked twice - the size query, then the export - and each runs the select pass (for a delta: the
        compare of every allocated tile with the shadow); a caller who minds passes a device buffer large enough."""
        n = C.c_size_t(0)
        if device:
            addr, cap = device
            st = self.lib.world_export(self.h, int(kind), C.c_void_p(int(addr)), int(cap), capi.MEM_DEVICE, C.byref(n))
            return n.value if st == capi.OK else self._check(st, "vofod_world_export", allow)
        st = self.lib.world_export(self.h, int(kind), None, 0, capi.MEM_HOST, C.byref(n))
        if st != capi.OK:
            return self._check(st, "vofod_world_export", allow)
        buf = np.empty(n.value, dtype=np.uint8)
        st = self.lib.world_export(self.h, int(kind), capi.ptr(buf), buf.size, capi.MEM_HOST, C.byref(n))
        if st != capi.OK:
            return self._check(st, "vofod_world_export", allow)
        return buf[: n.value]

    def world_apply(self, buf, allow: Sequence[int] = ()):
        """apply a world snapshot or delta: bytes / a uint8 array (world_export, a file, another process), or a pair (address, size in
        bytes) in the handle's device memory.  Returns the status (one in `allow` leaves the handle as it was)."""
        if isinstance(buf, tuple):
            addr, n = buf
            return self._check(self.lib.world_apply(self.h, C.c_void_p(int(addr)), int(n), capi.MEM_DEVICE), "vofod_world_apply", allow)
        b = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else buf).view(np.uint8).reshape(-1)
        return self._check(self.lib.world_apply(self.h, capi.ptr(b), b.size, capi.MEM_HOST), "vofod_world_apply", allow)

    def save_map(self, path, maps: int = capi.MAPS_ALL, full: bool = True) -> int:
        """checkpoint: export_map written to `path`; returns its size in bytes"""
        buf = self.export_map(maps, full)
        with open(path, "wb") as f:
            f.write(buf.tobytes())
        return buf.size

    def load_map(self, path) -> None:
        """restore a checkpoint written by save_map (a full snapshot, or the next delta of the chain applied last)"""
        with open(path, "rb") as f:
            self.apply_map(f.read())

    # ------------------------------------------------------------- hot path
    def _mk_dbg(self, n_points: int, clusters_cap: int | None = None):
        """debug buffers of one frame; `clusters_cap` bounds the cluster table (default: one per point, the worst case)"""
        n_cl = n_points if clusters_cap is None else clusters_cap
        w = np.zeros(n_points, dtype=capi.POINT_XYZR)
        lab = np.zeros(n_points, dtype=np.uint32)
        cl = np.zeros(n_cl, dtype=capi.CLUSTER_INFO)
        d = capi.ScanDebug()
        d.weighted, d.labels, d.weighted_cap = capi.ptr(w), capi.ptr(lab), n_points
        d.clusters, d.clusters_cap = capi.ptr(cl), n_cl
        return d, (w, lab, cl)

    @staticmethod
    def _dbg_dict(d: capi.ScanDebug, bufs):
        w, lab, cl = bufs
        return {
            "weighted": w[: d.n_weighted].copy(),
            "labels": lab[: d.n_weighted].copy(),
            "clusters": cl[: d.n_clusters].copy(),
            "n_input_after_crop": int(d.n_input_after_crop),
            "n_bg_voxels": int(d.n_bg_voxels),
            "background_pts_sufficient": bool(d.background_pts_sufficient),
            "sure_background_sufficient": bool(d.sure_background_sufficient),
            "stage_ms": list(d.stage_ms),
        }

    def process_scan(self, scan: ScanData, tf: np.ndarray, flags: int = capi.SCAN_DEFAULT, debug: bool = False, det_cap: int = 256,
                     allow: Sequence[int] = ()):
        tfa = np.ascontiguousarray(tf, dtype=np.float32).reshape(12)
        dets = np.zeros(det_cap, dtype=capi.DETECTION)
        n_out = C.c_size_t(0)
        cs = scan.as_c()
        dbg, bufs = (self._mk_dbg(scan.width * scan.height) if debug else (None, None))
        st = self.lib.process_scan(self.h, C.byref(cs), capi.ptr(tfa), flags, capi.ptr(dets), det_cap, C.byref(n_out), C.byref(dbg) if debug else None)
        self._check(st, "vofod_process_scan", allow)
        out = dets[: n_out.value].copy()
        return (out, self._dbg_dict(dbg, bufs)) if debug else out

    def process_batch(self, scans: Sequence[ScanData], tfs: np.ndarray, debug: bool = False, det_cap: int = 4096, clusters_cap: int | None = None, far_only: bool = False):
        """`far_only` (with `debug`): the view of the production path of read-only batches, which clusters close first - the
        cluster table lists the far clusters only, labels are capi.LABEL_NONE outside them (include/vofod.h)."""
        n = len(scans)
        arr = (capi.Scan * n)(*[s.as_c() for s in scans])
        tfa = np.ascontiguousarray(tfs, dtype=np.float32).reshape(n, 12)
        dets = np.zeros(det_cap, dtype=capi.DETECTION)
        per = np.zeros(n, dtype=np.uint32)
        n_out = C.c_size_t(0)
        dbgs = None
        bufs = []
        if debug:
            dbgs = (capi.ScanDebug * n)()
            for f in range(n):
                d, b = self._mk_dbg(scans[f].width * scans[f].height, clusters_cap)
                d.far_only = 1 if far_only else 0
                dbgs[f] = d
                bufs.append(b)
        st = self.lib.process_batch(self.h, arr, capi.ptr(tfa), n, capi.ptr(dets), det_cap, capi.ptr(per), C.byref(n_out), dbgs)
        self._check(st, "vofod_process_batch")
        out = dets[: n_out.value].copy()
        if debug:
            return out, per, [self._dbg_dict(dbgs[f], bufs[f]) for f in range(n)]
        return out, per

    def reserve(self, tickets: int):
        """allocate the workspaces of `tickets` batches in flight now instead of inside the first submits"""
        self._check(self.lib.reserve(self.h, int(tickets)), "vofod_reserve")

    def batch_submit(self, scans: Sequence[ScanData], tfs: np.ndarray) -> int:
        """Enqueue a batch (read-only map); returns the ticket for `batch_collect`.  At most eight in flight."""
        n = len(scans)
        key = id(scans)
        cached = self._scan_arrays.get(key)
        if cached is None or cached[0] != n:
            cached = (n, (capi.Scan * n)(*[s.as_c() for s in scans]), scans)  # keeps `scans` alive: the key is its id
            self._scan_arrays[key] = cached
        tfa = np.ascontiguousarray(tfs, dtype=np.float32).reshape(n, 12)
        ticket = C.c_int(-1)
        self._check(self.lib.batch_submit(self.h, cached[1], capi.ptr(tfa), n, C.byref(ticket)), "vofod_batch_submit")
        self._pending[ticket.value] = n
        return ticket.value

    def batch_collect(self, ticket: int, det_cap: int = 4096):
        n = self._pending.pop(ticket)
        for attempt in (0, 1):
            buf = self._collect_bufs.get((det_cap, n))  # reused between calls: the results are copied out below
            if buf is None:
                buf = (np.zeros(det_cap, dtype=capi.DETECTION), np.zeros(n, dtype=np.uint32))
                self._collect_bufs[(det_cap, n)] = buf
            dets, per = buf
            n_out = C.c_size_t(0)
            st = self.lib.batch_collect(self.h, ticket, capi.ptr(dets), det_cap, capi.ptr(per), C.byref(n_out))
            if st == capi.ERR_CAPACITY and attempt == 0 and n_out.value > det_cap:
                # device-tail batches stay pending when the array was too small (include/vofod.h): come back with the
                # size the library asked for.  (A batch that went through the host tail is consumed: the retry then
                # reports NOT_PENDING and the capacity error is raised.)
                msg = self.lib.last_error_string(self.h)
                det_cap = int(n_out.value)
                continue
            if st == capi.ERR_NOT_PENDING and attempt == 1:
                raise VofodError(capi.ERR_CAPACITY, "vofod_batch_collect", f"more than det_cap detections ({msg.decode() if msg else ''})")
            self._check(st, "vofod_batch_collect")
            return dets[: n_out.value].copy(), per.copy()

    def raycast_begin(self, scan: ScanData, tf: np.ndarray, allow: Sequence[int] = ()):
        tfa = np.ascontiguousarray(tf, dtype=np.float32).reshape(12)
        cs = scan.as_c()
        return self._check(self.lib.raycast_begin(self.h, C.byref(cs), capi.ptr(tfa)), "vofod_raycast_begin", allow)

    def raycast_finish(self, allow: Sequence[int] = ()):
        return self._check(self.lib.raycast_finish(self.h), "vofod_raycast_finish", allow)

    def sepclusters_begin(self, allow: Sequence[int] = ()):
        sure = C.c_int(0)
        st = self._check(self.lib.sepclusters_begin(self.h, C.byref(sure)), "vofod_sepclusters_begin", allow)
        return st, bool(sure.value)

    def sepclusters_finish(self, allow: Sequence[int] = ()):
        return self._check(self.lib.sepclusters_finish(self.h), "vofod_sepclusters_finish", allow)

    def range_to_points(self, scan: ScanData, out=None, allow: Sequence[int] = ()):
        """The points of a range image as the hot path decodes them (vofod_range_to_points): three float32 arrays of w*h values,
        or - with `out` = three device addresses - written to device memory (returns None)."""
        cs = scan.as_c()
        n = scan.width * scan.height
        if out is not None:
            self._check(self.lib.range_to_points(self.h, C.byref(cs), *(C.c_void_p(int(a)) for a in out), capi.MEM_DEVICE), "vofod_range_to_points", allow)
            return None
        xyz = [np.full(n, np.nan, dtype=np.float32) for _ in range(3)]
        self._check(self.lib.range_to_points(self.h, C.byref(cs), *(capi.ptr(a) for a in xyz), capi.MEM_HOST), "vofod_range_to_points", allow)
        return tuple(xyz)

    def deskew_points(self, scan: ScanData, out=None, allow: Sequence[int] = ()):
        """The compensated cloud of a point scan with `col_tfs` as the hot path sees it (vofod_deskew_points): three float32 arrays of
        w*h values, or - with `out` = three device addresses - written to device memory (returns None).  With a status in `allow`
        returned by the call: that status."""
        cs = scan.as_c()
        n = scan.width * scan.height
        if out is not None:
            st = self._check(self.lib.deskew_points(self.h, C.byref(cs), *(C.c_void_p(int(a)) for a in out), capi.MEM_DEVICE), "vofod_deskew_points", allow)
            return None if st == capi.OK else st
        xyz = [np.full(n, np.nan, dtype=np.float32) for _ in range(3)]
        st = self._check(self.lib.deskew_points(self.h, C.byref(cs), *(capi.ptr(a) for a in xyz), capi.MEM_HOST), "vofod_deskew_points", allow)
        return tuple(xyz) if st == capi.OK else st

    def detection_points(self, source: int = capi.POINTS_SYNC, device_out=None, allow: Sequence[int] = ()):
        """Member voxels and AABB of the detections returned last from `source` (vofod_detection_points): capi.POINTS_SYNC for the
        last synchronous process_scan / process_batch, or the ticket of a collected batch.  Returns (ext, points, index): one
        capi.DETECTION_EXTENT record per detection in the order returned, the members as capi.POINT_XYZR - detection by detection,
        ascending by their index in the frame's weighted cloud - and that index.  `device_out` = (points address, index address or
        None, capacity in points) on the handle's device: the points go there and (ext, None, None) comes back.  A status in
        `allow` is returned in place of the tuple."""
        n_ext, n_pts = C.c_size_t(0), C.c_size_t(0)
        st = self.lib.detection_points(self.h, int(source), None, 0, C.byref(n_ext), None, None, 0, C.byref(n_pts), capi.MEM_HOST)
        if st != capi.OK:
            return self._check(st, "vofod_detection_points", allow)
        ext = np.zeros(n_ext.value, dtype=capi.DETECTION_EXTENT)
        if device_out is not None:
            d_pts, d_idx, cap = device_out
            st = self.lib.detection_points(self.h, int(source), capi.ptr(ext), ext.size, C.byref(n_ext), C.c_void_p(int(d_pts)), None if d_idx is None else C.c_void_p(int(d_idx)), int(cap),
                                           C.byref(n_pts), capi.MEM_DEVICE)
            if st != capi.OK:
                return self._check(st, "vofod_detection_points", allow)
            return ext, None, None
        pts = np.zeros(n_pts.value, dtype=capi.POINT_XYZR)
        idx = np.zeros(n_pts.value, dtype=np.uint32)
        st = self.lib.detection_points(self.h, int(source), capi.ptr(ext), ext.size, C.byref(n_ext), capi.ptr(pts), capi.ptr(idx), pts.size, C.byref(n_pts), capi.MEM_HOST)
        if st != capi.OK:
            return self._check(st, "vofod_detection_points", allow)
        return ext, pts, idx

    def detection_pixels(self, source: int = capi.POINTS_SYNC, device_out=None, allow: Sequence[int] = ()):
        """The raw returns of the detections returned last from `source` (vofod_detection_pixels): which pixels row * width + col of
        their frames' scans fell into their member voxels.  Returns (span, pixels, member, xyz): one capi.DETECTION_SPAN record per
        detection in the order returned, the pixel indices - detection by detection, ascending - per pixel the position of its voxel
        in the detection's list of detection_points, and the transformed points as an (n, 3) float32 array.  `device_out` = (pixels
        address, member address or None, xyz address or None, capacity in pixels) on the handle's device: the three go there and
        (span, None, None, None) comes back.  A status in `allow` is returned in place of the tuple."""
        n_span, n_px = C.c_size_t(0), C.c_size_t(0)
        st = self.lib.detection_pixels(self.h, int(source), None, 0, C.byref(n_span), None, None, None, 0, C.byref(n_px), capi.MEM_HOST)
        if st != capi.OK:
            return self._check(st, "vofod_detection_pixels", allow)
        span = np.zeros(n_span.value, dtype=capi.DETECTION_SPAN)
        if device_out is not None:
            d_px, d_member, d_xyz, cap = device_out
            opt = lambda a: None if a is None else C.c_void_p(int(a))
            st = self.lib.detection_pixels(self.h, int(source), capi.ptr(span), span.size, C.byref(n_span), C.c_void_p(int(d_px)), opt(d_member), opt(d_xyz), int(cap), C.byref(n_px),
                                           capi.MEM_DEVICE)
            if st != capi.OK:
                return self._check(st, "vofod_detection_pixels", allow)
            return span, None, None, None
        px = np.zeros(n_px.value, dtype=np.uint32)
        member = np.zeros(n_px.value, dtype=np.uint32)
        xyz = np.zeros((n_px.value, 3), dtype=np.float32)
        st = self.lib.detection_pixels(self.h, int(source), capi.ptr(span), span.size, C.byref(n_span), capi.ptr(px), capi.ptr(member), capi.ptr(xyz), px.size, C.byref(n_px), capi.MEM_HOST)
        if st != capi.OK:
            return self._check(st, "vofod_detection_pixels", allow)
        return span, px, member, xyz

    # ------------------------------------------------- stateless L4 helpers
    def voxel_grid_weighted(self, x, y, z, leaf: float, align_center=None):
        return voxel_grid_weighted(self.lib, x, y, z, leaf, align_center, handle=self.h)

    def voxel_grid_counted(self, x, y, z, intensity, leaf: float, threshold: float):
        return voxel_grid_counted(self.lib, x, y, z, intensity, leaf, threshold, handle=self.h)

    def cluster(self, pts, keys, grid, tolerance: float):
        return cluster(self.lib, pts, keys, grid, tolerance, handle=self.h)


def _view(x, y, z, intensity=None):
    xs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (x, y, z)]
    v = capi.CloudView()
    v.x, v.y, v.z = (capi.ptr(a) for a in xs)
    if intensity is not None:
        it = np.ascontiguousarray(intensity, dtype=np.float32).reshape(-1)
        xs.append(it)
        v.intensity = capi.ptr(it)
    v.stride_bytes = 4
    v.n = xs[0].size
    v.memspace = capi.MEM_HOST
    return v, xs


def voxel_grid_weighted(lib, x, y, z, leaf, align_center=None, handle=None, allow=()):
    v, keep = _view(x, y, z)
    n = max(int(v.n), 1)
    out = np.zeros(n, dtype=capi.POINT_XYZR)
    keys = np.zeros(n, dtype=np.uint32)
    n_out = C.c_size_t(0)
    grid = capi.GridDesc()
    ac = None if align_center is None else np.ascontiguousarray(align_center, dtype=np.float32)
    st = lib.voxel_grid_weighted(handle, C.byref(v), leaf, int(ac is not None), capi.ptr(ac), capi.ptr(out), capi.ptr(keys), n, C.byref(n_out), C.byref(grid))
    if st != capi.OK and st not in allow:
        raise VofodError(st, "vofod_voxel_grid_weighted")
    return out[: n_out.value].copy(), keys[: n_out.value].copy(), grid, st


def voxel_grid_counted(lib, x, y, z, intensity, leaf, threshold, handle=None, allow=()):
    v, keep = _view(x, y, z, intensity)
    n = max(int(v.n), 1)
    out = np.zeros(n, dtype=capi.POINT_XYZR)
    keys = np.zeros(n, dtype=np.uint32)
    n_out = C.c_size_t(0)
    grid = capi.GridDesc()
    st = lib.voxel_grid_counted(handle, C.byref(v), leaf, threshold, capi.ptr(out), capi.ptr(keys), n, C.byref(n_out), C.byref(grid))
    if st != capi.OK and st not in allow:
        raise VofodError(st, "vofod_voxel_grid_counted")
    return out[: n_out.value].copy(), keys[: n_out.value].copy(), grid, st


def cluster(lib, pts, keys, grid, tolerance, handle=None):
    p = np.ascontiguousarray(pts, dtype=capi.POINT_XYZR)
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint32)
    labels = np.zeros(max(p.size, 1), dtype=np.uint32)
    nc = C.c_size_t(0)
    st = lib.cluster(handle, capi.ptr(p), capi.ptr(k), C.byref(grid) if grid is not None else None, p.size, tolerance, capi.ptr(labels), C.byref(nc))
    if st != capi.OK:
        raise VofodError(st, "vofod_cluster")
    return labels[: p.size].copy(), nc.value


def column_poses(lib, tf_begin, tf_end, tf_ref, n: int, frac=None) -> np.ndarray:
    """vofod_column_poses: [n, 3, 4] float32, col_tfs[m] = tf_ref^-1 o P(frac[m]) with P interpolating the two sensor->world poses
    (frac None: m / (n - 1)); what ScanData.range_image(col_tfs=...) takes"""
    a, b, r = (np.ascontiguousarray(t, dtype=np.float32).reshape(12) for t in (tf_begin, tf_end, tf_ref))
    fr = None if frac is None else np.ascontiguousarray(frac, dtype=np.float64).reshape(n)
    out = np.zeros((max(n, 0), 3, 4), dtype=np.float32)
    st = lib.column_poses(capi.ptr(a), capi.ptr(b), capi.ptr(r), capi.ptr(fr), n, capi.ptr(out))
    if st != capi.OK:
        raise VofodError(st, "vofod_column_poses")
    return out


def pose_lattice(lib, tf, step, n, yaw_step: float = 0.0, n_yaw: int = 1) -> np.ndarray:
    """vofod_pose_lattice: [n[0] * n[1] * n[2] * n_yaw, 3, 4] float32 candidate poses around `tf` - shifts of `step` along the world's
    axes, x fastest, and yaws of `yaw_step` radians about the vertical through the sensor's origin, slowest; what VoFOD.map_match takes"""
    t = np.ascontiguousarray(tf, dtype=np.float32).reshape(12)
    s = np.ascontiguousarray(step, dtype=np.float32).reshape(3)
    c = np.ascontiguousarray(n, dtype=np.int32).reshape(3)
    total = int(np.prod(np.maximum(c.astype(np.int64), 0))) * max(int(n_yaw), 0)
    out = np.zeros((min(total, 65535), 3, 4), dtype=np.float32)
    st = lib.pose_lattice(capi.ptr(t), capi.ptr(s), capi.ptr(c), float(yaw_step), int(n_yaw), capi.ptr(out))
    if st != capi.OK:
        raise VofodError(st, "vofod_pose_lattice")
    return out


def load_cloud(lib, filename: str) -> np.ndarray:
    n = C.c_size_t(0)
    st = lib.load_cloud(filename.encode(), None, 0, C.byref(n))
    if st not in (capi.OK, capi.ERR_CAPACITY):
        raise VofodError(st, "vofod_load_cloud")
    out = np.zeros((n.value, 3), dtype=np.float32)
    if n.value:
        st = lib.load_cloud(filename.encode(), capi.ptr(out), n.value, C.byref(n))
        if st != capi.OK:
            raise VofodError(st, "vofod_load_cloud")
    return out


def sim_lut(lib, w: int, h: int, vfov: float) -> np.ndarray:
    out = np.zeros((h * w, 3), dtype=np.float32)
    st = lib.sim_lut(w, h, vfov, capi.ptr(out))
    if st != capi.OK:
        raise VofodError(st, "vofod_sim_lut")
    return out


def ouster_lut(lib, w: int, h: int, azimuth_deg, altitude_deg, range_unit: float = 0.001, origin_mm: float = 0.0, tf=None):
    """initialize_sensor_lut (vofod_nodelet.cpp:358-372): (directions, offsets), each [h*w, 3] float32"""
    az = np.ascontiguousarray(azimuth_deg, dtype=np.float64)
    alt = np.ascontiguousarray(altitude_deg, dtype=np.float64)
    t = None if tf is None else np.ascontiguousarray(tf, dtype=np.float64).reshape(16)
    d = np.zeros((h * w, 3), dtype=np.float32)
    o = np.zeros((h * w, 3), dtype=np.float32)
    st = lib.ouster_lut(w, h, float(range_unit), float(origin_mm), None if t is None else capi.ptr(t), capi.ptr(az), capi.ptr(alt), capi.ptr(d), capi.ptr(o))
    if st != capi.OK:
        raise RuntimeError(f"vofod_ouster_lut: status {st}")
    return d, o


def mask_layout(lib, image, w: int, h: int, pixel_shift_by_row=None, mangle: bool = True):
    """load_mask (vofod_nodelet.cpp:506-560) after decoding: uint8[w*h]"""
    img = None if image is None else np.ascontiguousarray(image, dtype=np.uint8).reshape(h * w)
    sh = None if pixel_shift_by_row is None else np.ascontiguousarray(pixel_shift_by_row, dtype=np.int32)
    out = np.zeros(h * w, dtype=np.uint8)
    st = lib.mask_layout(None if img is None else capi.ptr(img), w, h, None if sh is None else capi.ptr(sh), int(bool(mangle)), capi.ptr(out))
    if st != capi.OK:
        raise RuntimeError(f"vofod_mask_layout: status {st}")
    return out


def check_sensor_params(lib, scan: ScanData, lut_directions, lut_offsets=None, mask=None):
    """check_sensor_params (vofod_nodelet.cpp:1869-1917): (params_ok, checked) for a host-resident organised scan"""
    d = np.ascontiguousarray(lut_directions, dtype=np.float32).reshape(-1)
    o = None if lut_offsets is None else np.ascontiguousarray(lut_offsets, dtype=np.float32).reshape(-1)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    cs = scan.as_c()
    checked = C.c_int32(0)
    st = lib.check_sensor_params(C.byref(cs), capi.ptr(d), None if o is None else capi.ptr(o), None if m is None else capi.ptr(m), C.byref(checked))
    if st not in (capi.OK, capi.ERR_SIZE_MISMATCH):
        raise VofodError(st, "vofod_check_sensor_params")
    return st == capi.OK, bool(checked.value)
