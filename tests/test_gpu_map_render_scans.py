"""vofod_map_render_scans on the device: every output against the numpy statement (map_render_scans_cases.py) bit for bit - sensors
of two waves, a ragged last wave and a second block of 8 live lanes; 1, 3 and 11 views mixing rigid scans, quarter-turn tables and
small rigid motions, host and device scans, strides 4 and 48, tables off 16 bytes, under non-zero column shifts and a mask with
zeros; every burst length, every output form, every refusal, the handle states the call is admitted in, its one launch, and a box
the map does not know seen as NEARER."""
import ctypes as C

import numpy as np
import pytest

import map_render_cases as mrc
import map_render_scans_cases as sc
from vofod_amd import capi, synth
from vofod_amd.detector import ScanData, column_poses

pytestmark = pytest.mark.gpu
F = np.float32
BURSTS = (1, 2, 4, 8)
RANGE_AT = 7  # the word of a 48-byte record that holds the range


# ------------------------------------------------------------------------------------------------ handles and scans
class Rig:
    """a handle of one sensor with the fixtures' mask and column shifts, and the device memory its scans lie in"""

    def __init__(self, hip, name):
        from test_gpu_range_image import DeviceMem

        w, h, area, vs, _ = sc.SENSORS[name]
        self.name, self.hip, self.w, self.h = name, hip, w, h
        dirs, offs = sc.lut_of(name, hip)
        self.dev = sc.make_det(hip, w, h, area, vs, dirs, offs, mask=sc.sensor_mask(w, h), max_batch=2)
        self.dev.set_column_shift(sc.column_shifts(w, h))
        got, want = mrc.geom(self.dev, dirs, offs), sc.geometry(name, dirs, offs)
        assert got.size == want.size and (got.off == want.off).all() and got.vs == want.vs
        self.mem = DeviceMem()

    def close(self):
        self.mem.free()
        self.dev.close()

    def scans(self, c, forms=None):
        """the case's views as ScanData, in the forms given per view (cycled): (memspace, stride).  Host scans are numpy arrays (a
        stride of 48: word 7 of 12-word records); device scans lie in device memory, their tables 4 bytes behind a 16-byte boundary
        for a stride of 48 and on one for a stride of 4."""
        forms = forms or (("host", 4), ("dev", 48), ("host", 48), ("dev", 4))
        out, self.keep = [], []
        for v, (_, tab) in enumerate(c.tabs):
            where, stride = forms[v % len(forms)]
            rec = np.full((c.w * c.h, stride // 4), 0xDEAD0000 + v, np.uint32)
            col = RANGE_AT if stride == 48 else 0
            rec[:, col] = c.ranges[v]
            if where == "host":
                self.keep.append(rec)
                out.append(ScanData.range_image(rec[:, col], c.w, c.h, stride_bytes=stride, col_tfs=tab))
            else:
                base = self.mem.put(rec.view(np.uint8))
                t = None if tab is None else self.mem.put(tab.view(np.uint8).reshape(-1), shift=4 if stride == 48 else 0)
                assert t is None or t % 16 == (4 if stride == 48 else 0)
                out.append(ScanData.range_image(base + 4 * col, c.w, c.h, stride_bytes=stride, memspace=capi.MEM_DEVICE, col_tfs=t))
        return out

    def call(self, c, scans=None, **kw):
        return self.dev.map_render_scans(self.scans(c) if scans is None else scans, c.tfs, c.threshold, c.length, c.tolerance, **kw)


@pytest.fixture(scope="module", params=list(sc.SENSORS))
def rig(request, hip):
    r = Rig(hip, request.param)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rig24(hip):
    r = Rig(hip, "24x11")
    yield r
    r.close()


# ------------------------------------------------------------------------------------------------ the verdict's edges
@pytest.mark.parametrize("case", sc.hand_verdicts(), ids=lambda c: c[0])
def test_hand_verdicts(hip, case):
    name, tf, cells, length, tol, ranges, want = case
    dev = mrc.hand_det(hip, (1.0, 0.0, 0.0))
    try:
        dev.write_map(capi.MAP_VOXELS, mrc.hand_map(cells))
        got = dev.map_render_scans([sc.scan_of(ranges, 2, 2)], tf[None], 0.0, length, tol)
        assert got.verdict.shape == (1, 2, 2) and got.counts.shape == (1, 8)
        assert got.verdict.reshape(-1).tolist() == want
        assert got.counts[0].tolist() == np.bincount(want, minlength=8).tolist()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ the statement, bit for bit
@pytest.mark.parametrize("burst", BURSTS)
def test_views_tables_strides_memspaces_every_burst(rig, monkeypatch, burst):
    monkeypatch.setenv("VOFOD_RENDER_BURST", str(burst))
    for n_views in (1, 3, 11):
        c = sc.shared_case(rig.hip, rig.name, n_views)
        rig.dev.write_map(capi.MAP_VOXELS, c.m)
        got = rig.call(c)
        sc.assert_same(got, c.exp, f"{rig.name}, {n_views} views, burst {burst}")
        assert (got.counts.sum(axis=1) == c.w * c.h).all() and (got.counts[:, 7] == 0).all()
        for v in range(n_views):
            np.testing.assert_array_equal(got.counts[v], np.bincount(got.verdict[v].reshape(-1), minlength=8))
    assert set(np.unique(c.exp.verdict).tolist()) == set(range(7))


@pytest.mark.parametrize("kind", ["empty", "solid"])
def test_empty_and_solid_maps(rig, kind):
    c = sc.shared_case(rig.hip, rig.name, 3, kind)
    rig.dev.write_map(capi.MAP_VOXELS, c.m)
    sc.assert_same(rig.call(c), c.exp, f"{rig.name}, {kind} map")
    assert ((c.exp.what == mrc.HIT).all() if kind == "solid" else not (c.exp.what == mrc.HIT).any())


def test_views_without_a_table_are_map_render(rig):
    """array for array: the four render outputs of the rigid views are those of vofod_map_render for the same tfs"""
    c = sc.shared_case(rig.hip, rig.name, 11)
    rig.dev.write_map(capi.MAP_VOXELS, c.m)
    got = rig.call(c)
    rigid = [v for v, (k, _) in enumerate(c.tabs) if k == "rigid"]
    assert len(rigid) == 4
    r, vx, w, t = rig.dev.map_render(c.tfs[rigid], c.threshold, c.length)
    np.testing.assert_array_equal(got.range[rigid], r)
    np.testing.assert_array_equal(got.voxel[rigid], vx)
    np.testing.assert_array_equal(got.what[rigid], w)
    np.testing.assert_array_equal(got.t_in_out[rigid].view(np.uint32), t.view(np.uint32))
    # ... and a call of rigid scans only, without ranges: the render alone
    bare = [ScanData.range_image(None, c.w, c.h) for _ in rigid]
    alone = rig.dev.map_render_scans(bare, c.tfs[rigid], c.threshold, c.length)
    assert alone.verdict is None and alone.counts is None
    np.testing.assert_array_equal(alone.range, r)
    np.testing.assert_array_equal(alone.t_in_out.view(np.uint32), t.view(np.uint32))
    # ... whatever vofod_set_raycast_motion says, a table is applied: that switch belongs to the raycast role
    for on in (True, False):
        rig.dev.set_raycast_motion(on)
        sc.assert_same(rig.call(c), c.exp, f"raycast motion {on}")


# ------------------------------------------------------------------------------------------------ output forms and counts
CANARY = 0xA5


def _want(c):
    e = c.exp
    return (e.range.view(np.uint8), e.voxel.view(np.uint8), e.what.view(np.uint8), e.tio.view(np.uint8), e.verdict.view(np.uint8))


def _raw(rig, c, scans, ptrs, counts, memspace):
    arr = (capi.Scan * len(scans))(*[s.as_c() for s in scans])
    return rig.dev.lib.map_render_scans(rig.dev.h, arr, capi.ptr(c.tfs), len(scans), c.threshold, c.length, c.tolerance, *ptrs, None if counts is None else capi.ptr(counts), memspace)


def test_output_forms(rig24):
    rig, c = rig24, sc.shared_case(rig24.hip, "24x11", 3)
    rig.dev.write_map(capi.MAP_VOXELS, c.m)
    scans = rig.scans(c)
    n = c.exp.what.size
    sizes, want = (4 * n, 4 * n, n, 8 * n, n), _want(c)
    # ---- each of the six NULL in turn, host outputs
    for skip in range(6):
        host = [np.full(s, CANARY, np.uint8) for s in sizes]
        counts = None if skip == 5 else np.full((3, 8), 0xDEADBEEF, np.uint32)
        ptrs = [None if k == skip else capi.ptr(b) for k, b in enumerate(host)]
        assert _raw(rig, c, scans, ptrs, counts, capi.MEM_HOST) == capi.OK, skip
        for k, (b, w) in enumerate(zip(host, want)):
            assert (b == CANARY).all() if k == skip else b.tobytes() == w.tobytes(), (skip, k)
        if counts is not None:
            np.testing.assert_array_equal(counts, c.exp.counts)
    # ---- counts alone
    counts = np.full((3, 8), 0xDEADBEEF, np.uint32)
    assert _raw(rig, c, scans, [None] * 5, counts, capi.MEM_HOST) == capi.OK
    np.testing.assert_array_equal(counts, c.exp.counts)
    # ---- device outputs in place: range / voxel / t_in_out at 4 / 4 / 8 but not 16 bytes, what and verdict at odd addresses;
    #      counts stays host memory
    addr = [rig.mem.put(np.full(s + 32, CANARY, np.uint8)) for s in sizes]
    shift = (4, 12, 3, 8, 5)
    r = rig.dev.map_render_scans(scans, c.tfs, c.threshold, c.length, c.tolerance, out=tuple(a + s for a, s in zip(addr, shift)))
    assert r.verdict is None and r.range is None
    np.testing.assert_array_equal(r.counts, c.exp.counts)
    for a, s, size, w in zip(addr, shift, sizes, want):
        got = rig.mem.get(a, size + 32, dtype=np.uint8)
        assert got[s : s + size].tobytes() == w.tobytes() and (got[:s] == CANARY).all() and (got[s + size :] == CANARY).all()
    # ---- verdict alone on the device, counts not asked for
    a = rig.mem.put(np.full(n + 32, CANARY, np.uint8))
    assert _raw(rig, c, scans, [None, None, None, None, C.c_void_p(a + 1)], None, capi.MEM_DEVICE) == capi.OK
    got = rig.mem.get(a, n + 32, dtype=np.uint8)
    assert got[1 : 1 + n].tobytes() == want[4].tobytes() and got[0] == CANARY and (got[1 + n :] == CANARY).all()


def test_fewer_views_leave_no_stale_counts(rig24):
    rig = rig24
    c11, c3 = sc.shared_case(rig.hip, "24x11", 11), sc.shared_case(rig.hip, "24x11", 3)
    rig.dev.write_map(capi.MAP_VOXELS, c11.m)
    np.testing.assert_array_equal(rig.call(c11).counts, c11.exp.counts)
    rig.dev.write_map(capi.MAP_VOXELS, c3.m)
    for _ in range(2):
        got = rig.call(c3)
        np.testing.assert_array_equal(got.counts, c3.exp.counts)
        assert (got.counts.sum(axis=1) == c3.w * c3.h).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(rig24):
    rig, c = rig24, sc.shared_case(rig24.hip, "24x11", 3)
    dev = rig.dev
    rig.dev.write_map(capi.MAP_VOXELS, c.m)
    n = c.w * c.h
    host_scans = rig.scans(c, forms=(("host", 4),))
    dev_scans = rig.scans(c, forms=(("dev", 4),))
    sizes = (4 * 3 * n, 4 * 3 * n, 3 * n, 8 * 3 * n, 3 * n)

    def call(scans=host_scans, tfs=c.tfs, n_scans=3, thr=0.5, far=5.0, tol=0.0, memspace=capi.MEM_HOST, null_scans=False, null_tfs=False, outs=None, counts=True):
        bufs = [np.full(s, CANARY, np.uint8) for s in sizes]
        cnt = np.full((3, 8), 0xDEADBEEF, np.uint32)
        arr = (capi.Scan * len(scans))(*[s.as_c() for s in scans])
        ptrs = [capi.ptr(b) for b in bufs] if outs is None else outs
        st = dev.lib.map_render_scans(dev.h, None if null_scans else arr, None if null_tfs else capi.ptr(np.ascontiguousarray(tfs, F)), n_scans, thr, far, tol, *ptrs,
                                      capi.ptr(cnt) if counts else None, memspace)
        assert st == capi.OK or (all((b == CANARY).all() for b in bufs) and (cnt == 0xDEADBEEF).all())
        return st

    def edited(scans, v, **kw):
        out = list(scans)
        out[v] = ScanData(**{**out[v].__dict__, **kw})
        return out

    INV, nan = capi.ERR_INVALID_ARG, float("nan")
    assert call(n_scans=0) == INV and call(n_scans=65536) == INV
    assert call(null_scans=True) == INV and call(null_tfs=True) == INV
    assert call(outs=[None] * 5, counts=False) == INV  # all six NULL
    assert call(far=0.0) == INV and call(far=-1.0) == INV and call(far=nan) == INV
    assert call(thr=nan) == INV
    assert call(tol=nan) == INV and call(tol=-0.001) == INV
    assert call(memspace=7) == INV and call(scans=edited(host_scans, 1, memspace=7)) == INV
    assert call(scans=edited(host_scans, 2, range=None)) == INV and call(scans=edited(dev_scans, 0, range=None)) == INV
    assert call(scans=edited(dev_scans, 1, range=int(dev_scans[1].range) + 2)) == INV
    assert call(scans=edited(dev_scans, 1, stride_bytes=6)) == INV
    assert call(scans=edited(dev_scans, 1, col_tfs=int(dev_scans[1].col_tfs) + 2)) == INV
    assert call(scans=edited(host_scans, 0, width=c.w + 1)) == capi.ERR_SIZE_MISMATCH
    assert call(scans=edited(host_scans, 2, height=c.h - 1)) == capi.ERR_SIZE_MISMATCH
    outside = c.tfs.copy()
    outside[2, 0, 3] = float(c.g.off[0]) - 0.1  # the third view's origin lies outside: the whole call is refused
    assert call(tfs=outside) == capi.ERR_SENSOR_OUTSIDE_MAP
    # misaligned device outputs (MAP RENDER's rule), with canaries on the device
    addr = [rig.mem.put(np.full(s + 32, CANARY, np.uint8)) for s in sizes]
    for bad in ((2, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 0, 4, 0)):
        assert call(scans=dev_scans, memspace=capi.MEM_DEVICE, outs=[C.c_void_p(a + 16 + b) for a, b in zip(addr, bad)]) == INV, bad
    for a, s in zip(addr, sizes):
        assert (rig.mem.get(a, s + 32, dtype=np.uint8) == CANARY).all()
    # what is no refusal: a tolerance of 0 and of +inf, an infinite threshold, an odd host stride, a range NULL when no verdict is asked for
    assert call(tol=float("inf"), outs=[None] * 5) == capi.OK
    assert call(thr=float("inf"), outs=[None] * 5) == capi.OK
    assert call(scans=edited(host_scans, 2, range=None), outs=[None, None, capi.ptr(np.zeros(3 * n, np.uint8)), None, None], counts=False) == capi.OK


# ------------------------------------------------------------------------------------------------ admission and state
def _profiled(dev, fn):
    from test_gpu_stream_route import profiled_calls

    dev.lib.profile_enable(dev.h, 1)
    try:
        profiled_calls(dev.lib, dev)
        out = fn()
        return out, profiled_calls(dev.lib, dev)
    finally:
        dev.lib.profile_enable(dev.h, 0)


PIX = np.arange(5, 16 * 1024, 131)  # 125 pixels of an OS1-16 scan, every ring and odd columns


@pytest.fixture(scope="module")
def field(hip):
    """the warmed OS1-16 handle of the map-shift tests: ground plane, a floating box, 0.5 m voxels, 241 x 201 x 51"""
    import map_shift_cases as mc

    dev = mc.make_det(hip, max_batch=2)
    dev.load_apriori(mc.ground_apriori())
    scans = mc.scans(mc.TARGET_IN_AREA, 0, mc.N_WARM + 2)
    dirs = synth.sim_lut(1024, 16, float(F(np.deg2rad(33.2))))
    a, b = mrc.pose((0.0, 0.0, 0.0)), mrc.pose((0.3, -0.1, 0.05), yaw=0.02)
    table = column_poses(hip, a, b, mrc.IDENT, 1024)
    yield mrc.SimpleNamespace(dev=dev, scans=scans, dirs=dirs, mc=mc, table=table)
    dev.close()


def _scans_are_the_statement(f, case, length=12.0):
    """two views - one with the table, one rigid - of two of the field's scans against the statement on PIX, the counts against the
    device's own verdicts"""
    dev = f.dev
    thr = float(dev.dp.voxel_map__thresholds__new_obstacles)
    src = [f.scans[0], f.scans[2]]
    tfs = np.stack([s.tf for s in src])
    rng = [np.ascontiguousarray(s.scan.range, np.uint32) for s in src]
    g = mrc.geom(dev, f.dirs)  # (the offset moves with a shift)
    exp = sc.statement(g, dev.read_map(), [mrc.SimpleNamespace(col_tfs=f.table, range=rng[0]), mrc.SimpleNamespace(col_tfs=None, range=rng[1])], tfs, thr, length, 0.1, pixels=PIX)
    got = dev.map_render_scans([ScanData.range_image(rng[0], 1024, 16, col_tfs=f.table), ScanData.range_image(rng[1], 1024, 16)], tfs, thr, length, 0.1)
    mrc.assert_same((got.range, got.voxel, got.what, got.t_in_out), exp, case, pixels=PIX)
    np.testing.assert_array_equal(got.verdict.reshape(2, -1)[:, PIX], exp.verdict.reshape(2, -1)[:, PIX], err_msg=case)
    for v in range(2):
        np.testing.assert_array_equal(got.counts[v], np.bincount(got.verdict[v].reshape(-1), minlength=8), err_msg=case)
    return exp


def test_state_routes_and_admission(field):
    f, dev, mc = field, field.dev, field.mc
    s = f.scans
    dev.process_scan(s[0].scan, s[0].tf)
    exp = _scans_are_the_statement(f, "after apriori + scan")
    assert len(set(np.unique(exp.verdict.reshape(2, -1)[:, PIX]).tolist())) >= 3
    # ---- one launch each, under its own name
    one = [ScanData.range_image(np.ascontiguousarray(s[0].scan.range, np.uint32), 1024, 16, col_tfs=f.table)]
    _, names = _profiled(dev, lambda: dev.map_render_scans(one, s[0].tf[None], 0.0, 12.0))
    assert names == {"k_map_render_scans": 1}, names
    _, names = _profiled(dev, lambda: dev.map_render(s[0].tf[None], 0.0, 12.0))
    assert names == {"k_map_render": 1}, names
    for k in range(1, mc.N_WARM):
        dev.process_scan(s[k].scan, s[k].tf, flags=capi.SCAN_AUTO_RAYCAST)
    if dev.status().raycast_pending:
        dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION, capi.ERR_RAYCAST_EMPTY))
    # ---- two tickets in flight: admitted, correct, the maps untouched, and the collects answer what the same batch answers afterwards
    batch, btf = [s[mc.N_WARM].scan, s[mc.N_WARM + 1].scan], np.stack([s[mc.N_WARM].tf, s[mc.N_WARM + 1].tf])
    maps = lambda: [mc.read_bits(dev, w) for w in (capi.MAP_VOXELS, capi.MAP_FLAGS)]
    t0, t1 = dev.batch_submit(batch, btf), dev.batch_submit(batch, btf)
    before = maps()
    _scans_are_the_statement(f, "tickets in flight")
    d1, p1 = dev.batch_collect(t1)
    d0, p0 = dev.batch_collect(t0)
    for a, b in zip(before, maps()):
        np.testing.assert_array_equal(a, b)
    d2, p2 = dev.batch_collect(dev.batch_submit(batch, btf))  # (the same batch without the call in between)
    assert len(d0) == len(d1) == len(d2) and p0.tolist() == p1.tolist() == p2.tolist()
    for k in ("frame", "n_points"):
        np.testing.assert_array_equal(d1[k], d2[k])

    def restore(saved):
        for w, bits in zip((capi.MAP_VOXELS, capi.MAP_FLAGS), saved):
            mc.write_bits(dev, w, bits)

    # ---- an exact raycast pass pending: admitted, accumulator and maps untouched; finished, then run again from the same maps
    #      without the call: the same bits (the exact pass does not depend on the order of its atomics)
    dev.set_raycast_exact(True)
    start = maps()
    dev.raycast_begin(s[3].scan, s[3].tf)
    assert dev.status().raycast_pending
    before, acc = maps(), dev.raycast_units()[0]
    assert (acc != 0).any()
    _scans_are_the_statement(f, "exact raycast pass pending")
    assert dev.status().raycast_pending
    np.testing.assert_array_equal(acc, dev.raycast_units()[0])
    for a, b in zip(before, maps()):
        np.testing.assert_array_equal(a, b)
    n_det = len(dev.process_scan(s[4].scan, s[4].tf))
    assert dev.raycast_finish() == capi.OK
    with_call = maps()
    restore(start)
    dev.raycast_begin(s[3].scan, s[3].tf)
    np.testing.assert_array_equal(acc, dev.raycast_units()[0])
    assert len(dev.process_scan(s[4].scan, s[4].tf)) == n_det
    assert dev.raycast_finish() == capi.OK
    for a, b in zip(with_call, maps()):
        np.testing.assert_array_equal(a, b)
    dev.set_raycast_exact(False)
    # ---- a sepclusters pass pending: the same
    start = maps()
    st, sure = dev.sepclusters_begin()
    assert st == capi.OK and sure, (st, sure)  # (the warmed field has sure background: the pass IS pending here)
    before = maps()
    _scans_are_the_statement(f, "sepclusters pass pending")
    for a, b in zip(before, maps()):
        np.testing.assert_array_equal(a, b)
    assert dev.sepclusters_finish() == capi.OK
    with_call = maps()
    restore(start)
    st, sure = dev.sepclusters_begin()
    assert st == capi.OK and sure, (st, sure)
    assert dev.sepclusters_finish() == capi.OK
    for a, b in zip(with_call, maps()):
        np.testing.assert_array_equal(a, b)
    # ---- after vofod_map_shift
    base = tuple(dev.sp.oparea_offset)
    assert dev.map_shift((2, -1, 0), mc.shifted_offset(base, (2, -1, 0), mc.VS)) == capi.OK
    _scans_are_the_statement(f, "after map_shift")


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("kind", ["added", "erased"])
def test_a_box_the_map_does_not_know(rig24, kind):
    """a scan rendered from a scene with a box in free air, against the map without it: NEARER exactly on the pixels that hit the
    box.  A scan rendered from a scene whose wall misses a box, against the map of the whole wall: THROUGH or BEYOND there, and
    agreement elsewhere.  The expected sets are the statement's."""
    e = sc.e2e_case(kind)
    dev = sc.make_det(rig24.hip, e.w, e.h, sc.SENSORS[sc.E2E_NAME][2], sc.SENSORS[sc.E2E_NAME][3], e.dirs)
    try:
        dev.write_map(capi.MAP_VOXELS, e.map)
        got = dev.map_render_scans([synth.scan_from_render(e.range)], e.tf[None], 0.0, sc.E2E_LENGTH)
        sc.assert_same(got, e.exp, kind)
        v = got.verdict[0]
        if kind == "added":
            assert ((v == sc.NEARER) == e.on_box).all() and got.counts[0, sc.NEARER] == e.on_box.sum()
        else:
            assert np.isin(v[e.on_box], (sc.THROUGH, sc.BEYOND)).all()
        assert np.isin(v[~e.on_box], (sc.AGREES, sc.EMPTY)).all()
    finally:
        dev.close()
