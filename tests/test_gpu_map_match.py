"""vofod_map_match on the device: every count and `best` against the numpy statement (map_match_cases.py) bit for bit - sensors of
two waves, a ragged wave, a second block of 8 lanes and eight blocks; maps with a ragged last bit word, NaN, +inf, -0.0 and
threshold-equal voxels, empty and solid; 1 to 300 candidates with NaN and infinite entries, quarter turns and poses that push every
point out through each face; live lists that straddle chunks of 32 points under every burst length; range images with and without
a pose per column, point scans, host and device memory, strides 4 and 48, an exclude box; every refusal; the handle states the
call is admitted in; its three launches; and a lattice around the true pose whose best candidate is the centre."""
import ctypes as C

import numpy as np
import pytest

import map_match_cases as mm
import map_render_cases as mrc
import range_motion_cases as rm
from vofod_amd import capi, synth
from vofod_amd.detector import ScanData, pose_lattice

pytestmark = pytest.mark.gpu
F = np.float32
BURSTS = (1, 2, 4, 8)
N_POSES = (1, 63, 64, 65, 256, 257, 300)  # a ragged wave, a full one, a ragged group, a second group
CANARY = 0xDEADBEEF
SENSOR_NAMES = ("16x8", "20x7", "24x11", "64x32")


# ------------------------------------------------------------------------------------------------ handles and scans
class Rig:
    """a handle of one sensor with the fixtures' exclude box, and the device memory its scans lie in"""

    def __init__(self, hip, name, exclude=mm.EXCLUDE):
        from test_gpu_range_image import DeviceMem

        self.name, self.hip = name, hip
        self.w, self.h = mm.SENSORS[name][:2]
        dirs, offs = mm.lut_of(name, hip)
        self.dev = mm.make_det(hip, name, dirs, offs, exclude=exclude, max_batch=2)
        got, want = mrc.geom(self.dev, dirs, offs), mm.geometry(name, dirs, offs)
        assert got.size == want.size and (got.off == want.off).all() and got.vs == want.vs
        lo, hi = mm.exclude_bounds(exclude)
        assert (np.array(rm.exclude_bounds(self.dev.sp)) == np.array([lo, hi])).all()
        self.mem = DeviceMem()
        self.keep = []

    def close(self):
        self.mem.free()
        self.dev.close()

    def scan(self, s, where="host", stride=4, tab_shift=0):
        """the statement's scan `s` (range + col_tfs, or xyz) as ScanData: host numpy or device memory, packed (stride 4) or the
        words of 48-byte records (x, y, z at words 0, 1, 2; range at word 7); a device table `tab_shift` bytes behind a 16-byte boundary"""
        n, words = self.w * self.h, stride // 4
        if s.xyz is not None:
            xyz = np.ascontiguousarray(s.xyz, F).view(np.uint32)
            if words == 1:  # three packed columns
                cols = [xyz[:, a].copy() for a in range(3)]
                if where == "host":
                    self.keep.append(cols)
                    return ScanData(x=cols[0], y=cols[1], z=cols[2], width=self.w, height=self.h, stride_bytes=4)
                addr = [self.mem.put(col.view(np.uint8)) for col in cols]
            else:  # one array of records
                rec = np.full((n, words), 0xDEAD0000, np.uint32)
                rec[:, :3] = xyz
                if where == "host":
                    self.keep.append(rec)
                    return ScanData(x=rec[:, 0], y=rec[:, 1], z=rec[:, 2], width=self.w, height=self.h, stride_bytes=stride)
                base = self.mem.put(rec.view(np.uint8))
                addr = [base, base + 4, base + 8]
            return ScanData(x=addr[0], y=addr[1], z=addr[2], width=self.w, height=self.h, stride_bytes=stride, memspace=capi.MEM_DEVICE)
        rec = np.full((n, words), 0xDEAD0000, np.uint32)
        col = 7 if words > 7 else 0
        rec[:, col] = s.range
        tab = None if s.col_tfs is None else np.ascontiguousarray(s.col_tfs, F)
        if where == "host":
            self.keep.append((rec, tab))
            return ScanData.range_image(rec[:, col], self.w, self.h, stride_bytes=stride, col_tfs=tab)
        t = None if tab is None else self.mem.put(tab.view(np.uint8).reshape(-1), shift=tab_shift)
        assert t is None or t % 16 == tab_shift
        return ScanData.range_image(self.mem.put(rec.view(np.uint8)) + 4 * col, self.w, self.h, stride_bytes=stride, memspace=capi.MEM_DEVICE, col_tfs=t)


@pytest.fixture(scope="module", params=SENSOR_NAMES)
def rig(request, hip):
    r = Rig(hip, request.param)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rig24(hip):
    r = Rig(hip, "24x11")
    yield r
    r.close()


def case_of(rig, kind, map_kind="random"):
    c = mm.shared_case(rig.hip, rig.name, kind, 300 if rig.name != "64x32" else 65, map_kind, mm.EXCLUDE)
    rig.dev.set_column_shift(c.shifts)  # (None: zeros)
    rig.dev.write_map(capi.MAP_VOXELS, c.m)
    return c


def assert_same(got, counts, case=""):
    counts = np.asarray(counts, np.uint32)
    np.testing.assert_array_equal(got.counts, counts, err_msg=f"{case}: counts")
    assert got.best == int(np.argmax(counts[:, mm.OCCUPIED])), f"{case}: best {got.best}"


FORMS = (("host", 4, 0), ("dev", 48, 4), ("host", 48, 0), ("dev", 4, 0))


# ------------------------------------------------------------------------------------------------ the statement, bit for bit
@pytest.mark.parametrize("kind", ["range", "motion", "points"])
def test_sensors_inputs_and_candidate_counts(rig, kind):
    """every sensor, every input kind in the four forms (host / device, strides 4 / 48, a table 4 bytes off a 16-byte boundary),
    under non-zero column shifts and the exclude box, for every candidate count: a prefix of the candidates is a call of its own"""
    c = case_of(rig, kind)
    assert set(np.unique(c.exp.classes).tolist()) == {0, 1, 2, 3}
    counts = [n for n in N_POSES if n <= len(c.tfs)]
    for k, n in enumerate(counts):
        where, stride, shift = FORMS[k % 4]
        got = rig.dev.map_match(rig.scan(c.scan, where, stride, shift), c.tfs[:n], c.threshold)
        assert got.counts.shape == (n, 4) and (got.counts.sum(axis=1) == c.w * c.h).all()
        assert_same(got, c.exp.counts[:n], f"{rig.name} {kind}, {n} poses, {where} stride {stride}")
    for where, stride, shift in FORMS:  # ... and every form with all the candidates
        assert_same(rig.dev.map_match(rig.scan(c.scan, where, stride, shift), c.tfs, c.threshold), c.exp.counts, f"{rig.name} {kind} {where} {stride}")


@pytest.mark.parametrize("map_kind", ["empty", "solid"])
def test_empty_and_solid_maps(rig, map_kind):
    c = case_of(rig, "motion", map_kind)
    assert_same(rig.dev.map_match(rig.scan(c.scan), c.tfs, c.threshold), c.exp.counts, f"{rig.name}, {map_kind} map")
    assert (c.exp.counts[:, mm.OCCUPIED if map_kind == "empty" else mm.FREE] == 0).all() and (c.exp.counts[:, mm.FREE if map_kind == "empty" else mm.OCCUPIED] > 0).any()


def test_threshold_is_the_calls_own(rig24):
    """the occupancy image is built per call: two thresholds in turn, and special values of the threshold"""
    c = case_of(rig24, "range")
    scan = rig24.scan(c.scan)
    for thr in (c.threshold, -3.0, 2.5, c.threshold, float("inf"), float("-inf")):
        exp = mm.statement(c.g, c.m, c.scan, c.tfs[:20], thr, c.lo, c.hi)
        assert_same(rig24.dev.map_match(scan, c.tfs[:20], thr), exp.counts, f"threshold {thr}")


# ------------------------------------------------------------------------------------------------ the live list
@pytest.mark.parametrize("burst", BURSTS)
def test_live_lists_that_straddle_chunks(rig24, monkeypatch, burst):
    monkeypatch.setenv("VOFOD_MATCH_CHUNK", "32")
    monkeypatch.setenv("VOFOD_MATCH_BURST", str(burst))
    rig, c = rig24, case_of(rig24, "range")
    n, all_live = c.w * c.h, int((~c.exp.skipped).sum())
    assert 33 < all_live < n
    for n_live in (0, 1, 31, 32, 33, all_live):
        s = mm.SimpleNamespace(range=mm.keep_live(c.scan.range, c.exp.skipped, n_live), col_tfs=None, xyz=None)
        exp = mm.statement(c.g, c.m, s, c.tfs[:70], c.threshold, c.lo, c.hi)
        assert exp.counts[0, 0] == n - n_live
        assert_same(rig.dev.map_match(rig.scan(s), c.tfs[:70], c.threshold), exp.counts, f"{n_live} live, burst {burst}")
    got = rig.dev.map_match(rig.scan(mm.SimpleNamespace(range=np.zeros(n, np.uint32), col_tfs=None, xyz=None)), c.tfs[:70], c.threshold)
    assert (got.counts == (n, 0, 0, 0)).all() and got.best == 0
    # a point scan whose only returns are its last pixels: the live list is filled from the tail block
    p = np.zeros((n, 3), F)
    p[n - 5 :] = mm.scan_points(c.g, c.scan, c.lo, c.hi)[0][np.flatnonzero(~c.exp.skipped)[:5]]
    s = mm.SimpleNamespace(range=None, col_tfs=None, xyz=p)
    assert_same(rig.dev.map_match(rig.scan(s), c.tfs[:70], c.threshold), mm.statement(c.g, c.m, s, c.tfs[:70], c.threshold, c.lo, c.hi).counts, "tail block")


@pytest.fixture(scope="module")
def rig64(hip):
    r = Rig(hip, "64x32")
    yield r
    r.close()


@pytest.mark.parametrize("chunk", ["1", "7", "1000", "1500", "100000", "0", "x"])
def test_chunk_lengths(rig64, monkeypatch, chunk):
    """64 x 32 = 2048 pixels: a chunk of one point, chunks that are no multiple of the burst, chunks longer than the LDS tile of 1024
    (1500: a full tile and a part of one), one longer than the list, and values that mean the kept one"""
    monkeypatch.setenv("VOFOD_MATCH_CHUNK", chunk)
    c = case_of(rig64, "motion")
    assert_same(rig64.dev.map_match(rig64.scan(c.scan), c.tfs, c.threshold), c.exp.counts, f"chunk {chunk}")


# ------------------------------------------------------------------------------------------------ interface
def _raw(dev, scan, tfs, n, thr, counts, best):
    cs = scan.as_c() if scan is not None else None
    return dev.lib.map_match(dev.h, None if cs is None else C.byref(cs), None if tfs is None else capi.ptr(tfs), n, thr, None if counts is None else capi.ptr(counts),
                             None if best is None else C.byref(best))


def test_best_null_and_no_stale_counts(rig24):
    rig, c = rig24, case_of(rig24, "motion")
    scan, tfs = rig.scan(c.scan), np.ascontiguousarray(c.tfs, F)
    counts = np.full((300, 4), CANARY, np.uint32)
    assert _raw(rig.dev, scan, tfs, 300, c.threshold, counts, None) == capi.OK
    np.testing.assert_array_equal(counts, c.exp.counts)
    # fewer poses afterwards, twice: nothing of the longer call is left, nothing behind the answer is written
    for _ in range(2):
        counts = np.full((300, 4), CANARY, np.uint32)
        best = C.c_int32(-7)
        assert _raw(rig.dev, scan, tfs[20:], 11, c.threshold, counts, best) == capi.OK
        np.testing.assert_array_equal(counts[:11], c.exp.counts[20:31])
        assert (counts[11:] == CANARY).all() and best.value == int(np.argmax(c.exp.counts[20:31, 3]))
    # ties: the smallest k
    twice = np.concatenate([tfs[:9], tfs[:9]])
    assert rig.dev.map_match(scan, twice, c.threshold).best == int(np.argmax(c.exp.counts[:9, 3]))


def test_refusals_leave_the_outputs_untouched(rig24):
    rig, c = rig24, case_of(rig24, "motion")
    dev, tfs = rig.dev, np.ascontiguousarray(c.tfs[:5], F)
    host, devs = rig.scan(c.scan), rig.scan(c.scan, "dev", 48, 4)
    pts = mm.SimpleNamespace(range=None, col_tfs=None, xyz=mm.scan_points(c.g, c.scan, c.lo, c.hi)[0])
    hpts, dpts = rig.scan(pts), rig.scan(pts, "dev", 48)

    def call(scan=host, tfs=tfs, n=5, thr=0.5, null_counts=False, null_h=False):
        counts, best = np.full((5, 4), CANARY, np.uint32), C.c_int32(-7)
        if null_h:
            cs = scan.as_c()
            st = dev.lib.map_match(None, C.byref(cs), capi.ptr(tfs), n, thr, capi.ptr(counts), C.byref(best))
        else:
            st = _raw(dev, scan, tfs, n, thr, None if null_counts else counts, best)
        assert st == capi.OK or ((counts == CANARY).all() and best.value == -7)
        return st

    def edited(s, **kw):
        return ScanData(**{**s.__dict__, **kw})

    INV = capi.ERR_INVALID_ARG
    assert call() == capi.OK
    assert call(null_h=True) == INV and call(scan=None) == INV and call(tfs=None) == INV and call(null_counts=True) == INV
    assert call(n=0) == INV and call(n=65536) == INV
    assert call(thr=float("nan")) == INV
    assert call(scan=edited(host, memspace=7)) == INV
    assert call(scan=edited(hpts, x=None)) == INV and call(scan=edited(hpts, y=None, z=None)) == INV  # one or two of x, y, z NULL
    assert call(scan=edited(host, range=None)) == INV  # all three NULL and no range
    dev.set_point_motion(True)
    assert call(scan=edited(hpts, col_tfs=host.col_tfs)) == INV  # a point scan with col_tfs, whatever the switch says
    dev.set_point_motion(False)
    assert call(scan=edited(hpts, col_tfs=host.col_tfs)) == INV
    assert call(scan=edited(devs, range=int(devs.range) + 2)) == INV and call(scan=edited(devs, stride_bytes=6)) == INV
    assert call(scan=edited(dpts, y=int(dpts.y) + 1)) == INV and call(scan=edited(dpts, stride_bytes=50)) == INV
    assert call(scan=edited(devs, col_tfs=int(devs.col_tfs) + 2)) == INV
    assert call(scan=edited(host, width=c.w + 1)) == capi.ERR_SIZE_MISMATCH and call(scan=edited(hpts, height=c.h - 1)) == capi.ERR_SIZE_MISMATCH
    # what is no refusal: an infinite threshold, a candidate far outside the map (no SENSOR_OUTSIDE_MAP rule), an odd host stride
    assert call(thr=float("inf")) == capi.OK
    far = tfs.copy()
    far[:, :, 3] += 1000.0
    assert call(tfs=far) == capi.OK
    odd = np.zeros(c.w * c.h * 5 + 4, np.uint8)
    assert call(scan=edited(host, range=odd[1:], stride_bytes=5)) == capi.OK


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


@pytest.fixture(scope="module")
def field(hip):
    """the warmed OS1-16 handle of the map-shift tests: ground plane, a floating box, 0.5 m voxels, 241 x 201 x 51, the default exclude box"""
    import map_shift_cases as mc

    dev = mc.make_det(hip, max_batch=2)
    dev.load_apriori(mc.ground_apriori())
    scans = mc.scans(mc.TARGET_IN_AREA, 0, mc.N_WARM + 2)
    dirs = synth.sim_lut(1024, 16, float(F(np.deg2rad(33.2))))
    yield mm.SimpleNamespace(dev=dev, scans=scans, dirs=dirs, mc=mc)
    dev.close()


def _match_is_the_statement(f, case):
    """a range image with a table, a plain one and a point scan of the field's scans, each under a 3 x 3 x 2 lattice with three yaws,
    against the statement over all 16384 pixels"""
    from vofod_amd.detector import column_poses

    dev = f.dev
    thr = float(dev.dp.voxel_map__thresholds__new_obstacles)
    g = mrc.geom(dev, f.dirs)  # (the offset moves with a shift)
    m = dev.read_map()
    lo, hi = rm.exclude_bounds(dev.sp)
    table = np.ascontiguousarray(column_poses(dev.lib, mrc.pose((0.0, 0.0, 0.0)), mrc.pose((0.3, -0.1, 0.05), yaw=0.02), mrc.IDENT, 1024), F)
    seen = set()
    for k, (s, kind) in enumerate(((f.scans[0], "motion"), (f.scans[2], "range"), (f.scans[1], "points"))):
        tfs = pose_lattice(dev.lib, s.tf, (0.5, 0.5, 0.5), (3, 3, 2), 0.05, 3)
        rng = np.ascontiguousarray(s.scan.range, np.uint32)
        if kind == "points":
            st = mm.SimpleNamespace(range=None, col_tfs=None, xyz=np.stack([s.scan.x, s.scan.y, s.scan.z], axis=1).astype(F))
            scan = ScanData(x=st.xyz[:, 0].copy(), y=st.xyz[:, 1].copy(), z=st.xyz[:, 2].copy(), width=1024, height=16)
        else:
            st = mm.SimpleNamespace(range=rng, col_tfs=table if kind == "motion" else None, xyz=None)
            scan = ScanData.range_image(rng, 1024, 16, col_tfs=st.col_tfs)
        exp = mm.statement(g, m, st, tfs, thr, lo, hi)
        assert_same(dev.map_match(scan, tfs, thr), exp.counts, f"{case}: {kind}")
        seen |= set(np.unique(exp.classes).tolist())
    return seen


def test_state_routes_and_admission(field):
    f, dev, mc = field, field.dev, field.mc
    s = f.scans
    dev.process_scan(s[0].scan, s[0].tf)
    assert _match_is_the_statement(f, "after apriori + scan") == {0, 1, 2, 3}
    # ---- three launches per call, under their own names; the other entries' launches as they were
    one = ScanData.range_image(np.ascontiguousarray(s[0].scan.range, np.uint32), 1024, 16)
    _, names = _profiled(dev, lambda: dev.map_match(one, s[0].tf[None], 0.0))
    assert names == {"k_match_bits": 1, "k_match_points": 1, "k_match_score": 1}, names
    _, names = _profiled(dev, lambda: dev.map_match(one, pose_lattice(dev.lib, s[0].tf, (0.5,) * 3, (9, 9, 5), 0.02, 3), 0.0))
    assert names == {"k_match_bits": 1, "k_match_points": 1, "k_match_score": 1}, names
    _, names = _profiled(dev, lambda: dev.map_render(s[0].tf[None], 0.0, 12.0))
    assert names == {"k_map_render": 1}, names
    _, a = _profiled(dev, lambda: dev.process_scan(s[0].scan, s[0].tf))
    dev.map_match(one, s[0].tf[None], 0.0)
    _, b = _profiled(dev, lambda: dev.process_scan(s[0].scan, s[0].tf))
    assert a == b and not any(k.startswith("k_match") for k in a), (a, b)
    for k in range(1, mc.N_WARM):
        dev.process_scan(s[k].scan, s[k].tf, flags=capi.SCAN_AUTO_RAYCAST)
    if dev.status().raycast_pending:
        dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION, capi.ERR_RAYCAST_EMPTY))
    # ---- two tickets in flight: admitted, correct, the maps untouched, and the collects answer what the same batch answers afterwards
    batch, btf = [s[mc.N_WARM].scan, s[mc.N_WARM + 1].scan], np.stack([s[mc.N_WARM].tf, s[mc.N_WARM + 1].tf])
    maps = lambda: [mc.read_bits(dev, w) for w in (capi.MAP_VOXELS, capi.MAP_FLAGS)]
    t0, t1 = dev.batch_submit(batch, btf), dev.batch_submit(batch, btf)
    before = maps()
    _match_is_the_statement(f, "tickets in flight")
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
    #      without the call: the same bits
    dev.set_raycast_exact(True)
    start = maps()
    dev.raycast_begin(s[3].scan, s[3].tf)
    assert dev.status().raycast_pending
    before, acc = maps(), dev.raycast_units()[0]
    assert (acc != 0).any()
    _match_is_the_statement(f, "exact raycast pass pending")
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
    _match_is_the_statement(f, "sepclusters pass pending")
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
    _match_is_the_statement(f, "after map_shift")
    # ---- with the world store: the window is matched
    assert dev.world_enable((8, 8, 0), (8, 8, 0), 4096) == capi.OK
    base = tuple(dev.sp.oparea_offset)
    assert dev.map_shift((-3, 2, 0), mc.shifted_offset(base, (-3, 2, 0), mc.VS)) == capi.OK
    _match_is_the_statement(f, "world store, after a shift")
    assert dev.world_disable() == capi.OK


# ------------------------------------------------------------------------------------------------ end to end
def test_the_centre_of_the_lattice_is_the_best_candidate(hip):
    """a scan rendered from pose P by the device, matched against the same map under a 5 x 5 x 3 lattice with 3 yaws around P: the
    statement's counts bit for bit, and best == the centre"""
    e = mm.e2e_case()
    dev = mm.make_det(hip, mm.E2E_NAME, e.dirs)
    try:
        dev.write_map(capi.MAP_VOXELS, e.map)
        rng = dev.map_render(e.P[None], mm.E2E_THRESHOLD, mm.E2E_LENGTH)[0]
        np.testing.assert_array_equal(rng[0], e.range)
        n, n_yaw, yaw_step = e.lattice
        tfs = pose_lattice(hip, e.P, (float(e.g.vs),) * 3, n, yaw_step, n_yaw)
        np.testing.assert_array_max_ulp(tfs, e.tfs, maxulp=1)
        got = dev.map_match(synth.scan_from_render(rng[0]), e.tfs, mm.E2E_THRESHOLD)
        assert_same(got, e.exp.counts, "end to end")
        assert got.best == e.centre
        assert dev.map_match(synth.scan_from_render(rng[0]), tfs, mm.E2E_THRESHOLD).best == e.centre
    finally:
        dev.close()
