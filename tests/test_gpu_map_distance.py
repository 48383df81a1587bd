"""vofod_map_distance and vofod_map_match_field on the device: every d2, count, cost and `best` against the numpy statement
(map_distance_cases.py) bit for bit.  The distance: maps with a ragged last bit word, rows that cross word boundaries and start
mid-word, an axis longer than 255 and than a block, each pass's own long axis; empty, solid, one voxel in each corner, random at
three densities with NaN, +inf, -0.0 and threshold-equal voxels; radii either side of one bit word and one larger than every axis;
host and device outputs, one 2 bytes off a 4-byte boundary; the call's own threshold; every refusal.  The field match: the sensors,
input kinds, candidate lists, chunk and burst lengths of test_gpu_map_match.py (its case builders, imported), the call's own field
and an arbitrary one, host and device; the tie to vofod_map_match at near2 = 0; a sum beyond 2^32; every refusal.  Both calls in the
handle states they are admitted in, their launches, and the scene whose cost is lowest at the centre."""
import ctypes as C

import numpy as np
import pytest

import map_distance_cases as md
import map_match_cases as mm
import map_render_cases as mrc
import range_motion_cases as rm
import test_gpu_map_match as tm
from vofod_amd import capi, synth
from vofod_amd.detector import ScanData, pose_lattice

pytestmark = pytest.mark.gpu
F = np.float32
CANARY16 = 0xABCD
NEAR2, OUTSIDE_COST, RADIUS = 4, 64, 8  # the field match's defaults here: NEAR within two voxels, OUTSIDE costs R * R


@pytest.fixture(scope="module")
def mem():
    from test_gpu_range_image import DeviceMem

    m = DeviceMem()
    yield m
    m.free()


def _to_device(mem, addr, arr):
    arr = np.ascontiguousarray(arr)
    assert mem.rt.hipMemcpy(C.c_void_p(addr), arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0  # hipMemcpyHostToDevice


# ------------------------------------------------------------------------------------------------ the distance, bit for bit
@pytest.mark.parametrize("name", list(md.MAPS))
def test_distance_is_the_statement(hip, mem, name):
    """every content and radius on one map; a third of the calls write a device buffer on a 4-byte boundary, a third one 2 bytes off
    a 4-byte boundary, between canaries that stay"""
    dev = md.make_det(hip, name)
    n = int(np.prod(md.MAPS[name]))
    buf = mem.empty(2 * (n + 4))
    try:
        for k, kind in enumerate(md.CONTENTS):
            m, full = md.shared_full(name, kind)
            dev.write_map(capi.MAP_VOXELS, m)
            for j, R in enumerate(md.RADII):
                exp = md.clamp(full, R)
                where = (k + j) % 3
                if where == 0:
                    got = dev.map_distance(md.THRESHOLD, R)
                else:
                    skew = where - 1  # in uint16 elements: 0, or 1 = two bytes off
                    _to_device(mem, buf, np.full(n + 4, CANARY16, np.uint16))
                    assert dev.map_distance(md.THRESHOLD, R, device=buf + 2 * (1 + skew)) is None
                    raw = mem.get(buf, n + 4, np.uint16)
                    assert (raw[: 1 + skew] == CANARY16).all() and (raw[1 + skew + n :] == CANARY16).all(), f"{name} {kind} R {R}: canaries"
                    got = raw[1 + skew : 1 + skew + n].reshape(exp.shape)
                assert got.dtype == np.uint16 and got.shape == exp.shape
                np.testing.assert_array_equal(got, exp, err_msg=f"{name} {kind} R {R} output {where}")
    finally:
        dev.close()


def test_threshold_is_the_calls_own(hip):
    """two thresholds in turn on one handle - no stale image - and the infinite ones"""
    name = "21x13x9"
    dev = md.make_det(hip, name)
    try:
        m, _ = md.shared_full(name, "random50")
        dev.write_map(capi.MAP_VOXELS, m)
        for thr in (md.THRESHOLD, -3.0, 2.5, md.THRESHOLD, float("inf"), float("-inf"), md.THRESHOLD):
            np.testing.assert_array_equal(dev.map_distance(thr, 3), md.distance(m, thr, 3), err_msg=f"threshold {thr}")
        assert (dev.map_distance(float("inf"), 5) == 25).all() and (dev.map_distance(float("-inf"), 5) == 0).sum() == (m > -np.inf).sum()  # (NaN and -inf itself are not above -inf)
    finally:
        dev.close()


def test_distance_refusals_leave_the_output_untouched(hip, mem):
    name = "9x9x9"
    dev = md.make_det(hip, name)
    n = 729
    dbuf = mem.empty(2 * n + 16)
    try:
        def call(h=True, thr=0.5, R=3, null=False, n_=n, memspace=capi.MEM_HOST, addr=None):
            out = np.full(n + 8, CANARY16, np.uint16)
            if addr is not None:
                _to_device(mem, dbuf, np.full(n + 8, CANARY16, np.uint16))
            d2 = None if null else capi.ptr(out) if addr is None else C.c_void_p(addr)
            st = dev.lib.map_distance(dev.h if h else None, thr, R, d2, n_, memspace)
            if addr is not None:
                out = mem.get(dbuf, n + 8, np.uint16)
            assert st == capi.OK or (out == CANARY16).all()
            return st

        INV = capi.ERR_INVALID_ARG
        assert call() == capi.OK
        assert call(h=False) == INV and call(null=True) == INV
        assert call(thr=float("nan")) == INV
        assert call(R=0) == INV and call(R=-1) == INV and call(R=256) == INV and call(R=2**31 - 1) == INV
        assert call(memspace=7) == INV and call(memspace=-1) == INV
        assert call(memspace=capi.MEM_DEVICE, addr=dbuf + 1) == INV and call(memspace=capi.MEM_DEVICE, addr=dbuf + 3) == INV
        assert call(n_=n - 1) == capi.ERR_SIZE_MISMATCH and call(n_=n + 1) == capi.ERR_SIZE_MISMATCH and call(n_=0) == capi.ERR_SIZE_MISMATCH
        # what is no refusal: the infinite thresholds, the radii at the ends of the range, a device buffer on any even address
        assert call(thr=float("inf")) == capi.OK and call(thr=float("-inf")) == capi.OK and call(R=1) == capi.OK and call(R=255) == capi.OK
        assert call(memspace=capi.MEM_DEVICE, addr=dbuf + 2) == capi.OK and call(memspace=capi.MEM_DEVICE, addr=dbuf) == capi.OK
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ the field match, bit for bit
@pytest.fixture(scope="module", params=tm.SENSOR_NAMES)
def rig(request, hip):
    r = tm.Rig(hip, request.param)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rig24(hip):
    r = tm.Rig(hip, "24x11")
    yield r
    r.close()


@pytest.fixture(scope="module")
def rig64(hip):
    r = tm.Rig(hip, "64x32")
    yield r
    r.close()


_EXP = {}


def expected(c, key, d2, near2=NEAR2, outside_cost=OUTSIDE_COST, scan=None, n=None):
    """the statement of one case, field and parameter pair, computed once per process"""
    k = (c.name, c.kind, key, near2, outside_cost)
    if scan is not None:
        return md.field_statement(c.g, d2, scan, c.tfs[:n], near2, outside_cost, c.lo, c.hi, c.shifts)
    if k not in _EXP:
        _EXP[k] = md.field_statement(c.g, d2, c.scan, c.tfs, near2, outside_cost, c.lo, c.hi, c.shifts)
    return _EXP[k]


def assert_same(got, exp, n=None, case=""):
    counts, cost = np.asarray(exp.counts[:n], np.uint32), np.asarray(exp.cost[:n], np.uint64)
    np.testing.assert_array_equal(got.counts, counts, err_msg=f"{case}: counts")
    np.testing.assert_array_equal(got.cost, cost, err_msg=f"{case}: cost")
    assert got.cost.dtype == np.uint64 and got.best == int(np.argmin(cost)), f"{case}: best {got.best}"


def own_field(rig, c):
    """the field of vofod_map_distance for the case's map, held to the statement"""
    d2 = rig.dev.map_distance(c.threshold, RADIUS)
    np.testing.assert_array_equal(d2, md.distance(c.m, c.threshold, RADIUS))
    return d2


@pytest.mark.parametrize("kind", ["range", "motion", "points"])
def test_field_sensors_inputs_and_candidate_counts(rig, kind):
    """every sensor, every input kind in the four forms, for every candidate count, the field of vofod_map_distance on the host and
    on the device; then an arbitrary field, on the host and on the device 2 bytes off a 4-byte boundary"""
    c = tm.case_of(rig, kind)
    d2 = own_field(rig, c)
    exp = expected(c, "own", d2)
    assert set(np.flatnonzero(exp.counts.any(axis=0)).tolist()) == {0, 1, 2, 3} and len(set(exp.cost.tolist())) > len(exp.cost) // 3
    on_device = rig.mem.put(d2.view(np.uint8).reshape(-1))
    for k, n in enumerate(n for n in tm.N_POSES if n <= len(c.tfs)):
        where, stride, shift = tm.FORMS[k % 4]
        got = rig.dev.map_match_field(rig.scan(c.scan, where, stride, shift), c.tfs[:n], d2 if k % 2 else on_device, NEAR2, OUTSIDE_COST)
        assert got.counts.shape == (n, 4) and (got.counts.sum(axis=1) == c.w * c.h).all()
        assert_same(got, exp, n, f"{rig.name} {kind}, {n} poses, {where} stride {stride}")
    for where, stride, shift in tm.FORMS:
        assert_same(rig.dev.map_match_field(rig.scan(c.scan, where, stride, shift), c.tfs, on_device, NEAR2, OUTSIDE_COST), exp, None, f"{rig.name} {kind} {where} {stride}")
    anyf = md.random_field(d2.size, 3)
    exp = expected(c, "random", anyf, 30000, 65535)
    skewed = rig.mem.put(anyf.view(np.uint8), shift=2)
    assert skewed % 4 == 2
    assert_same(rig.dev.map_match_field(rig.scan(c.scan), c.tfs, anyf, 30000, 65535), exp, None, f"{rig.name} {kind}: an arbitrary host field")
    assert_same(rig.dev.map_match_field(rig.scan(c.scan, "dev", 48, 4), c.tfs, skewed, 30000, 65535), exp, None, f"{rig.name} {kind}: an arbitrary device field")


def test_near2_zero_is_map_matchs_occupied(rig):
    """near2 = 0 with the call's own field: NEAR is vofod_map_match's OCCUPIED at the same threshold and FAR its FREE, for every
    candidate - on the device, one call against the other"""
    c = tm.case_of(rig, "motion")
    scan = rig.scan(c.scan)
    for thr, R in ((c.threshold, 1), (2.5, RADIUS)):
        d2 = rig.dev.map_distance(thr, R)
        field, count = rig.dev.map_match_field(scan, c.tfs, d2, 0, 0), rig.dev.map_match(scan, c.tfs, thr)
        np.testing.assert_array_equal(field.counts[:, md.NEAR], count.counts[:, mm.OCCUPIED])
        np.testing.assert_array_equal(field.counts[:, md.FAR], count.counts[:, mm.FREE])
        np.testing.assert_array_equal(field.counts[:, :2], count.counts[:, :2])
        assert thr != c.threshold or (count.counts[:, mm.OCCUPIED] > 0).any()


def test_near2_and_outside_cost_at_their_ends(rig24):
    c = tm.case_of(rig24, "range")
    d2 = own_field(rig24, c)
    anyf = md.random_field(d2.size, 9)
    scan = rig24.scan(c.scan)
    for near2 in (0, 65535):
        for oc in (0, 65535):
            assert_same(rig24.dev.map_match_field(scan, c.tfs[:70], d2, near2, oc), expected(c, "own", d2, near2, oc), 70, f"own field, near2 {near2}, outside_cost {oc}")
            exp = expected(c, "random9", anyf, near2, oc)
            assert_same(rig24.dev.map_match_field(scan, c.tfs[:70], anyf, near2, oc), exp, 70, f"arbitrary field, near2 {near2}, outside_cost {oc}")
            assert near2 == 0 or (exp.counts[:, md.FAR] == 0).all()  # 65535: everything inside is NEAR
    # a near2 above the field's maximum is no refusal
    got = rig24.dev.map_match_field(scan, c.tfs[:70], anyf, 0xFFFFFFFF, 1)
    assert_same(got, expected(c, "random9", anyf, 65535, 1), 70, "near2 = 2^32 - 1")


@pytest.mark.parametrize("burst", tm.BURSTS)
def test_field_live_lists_that_straddle_chunks(rig24, monkeypatch, burst):
    monkeypatch.setenv("VOFOD_MATCH_CHUNK", "32")
    monkeypatch.setenv("VOFOD_MATCH_BURST", str(burst))
    rig, c = rig24, tm.case_of(rig24, "range")
    d2 = own_field(rig, c)
    n, all_live = c.w * c.h, int((~c.exp.skipped).sum())
    for n_live in (0, 1, 31, 32, 33, all_live):
        s = mm.SimpleNamespace(range=mm.keep_live(c.scan.range, c.exp.skipped, n_live), col_tfs=None, xyz=None)
        exp = expected(c, None, d2, scan=s, n=70)
        assert exp.counts[0, 0] == n - n_live
        assert_same(rig.dev.map_match_field(rig.scan(s), c.tfs[:70], d2, NEAR2, OUTSIDE_COST), exp, None, f"{n_live} live, burst {burst}")
    got = rig.dev.map_match_field(rig.scan(mm.SimpleNamespace(range=np.zeros(n, np.uint32), col_tfs=None, xyz=None)), c.tfs[:70], d2, NEAR2, OUTSIDE_COST)
    assert (got.counts == (n, 0, 0, 0)).all() and (got.cost == 0).all() and got.best == 0


@pytest.mark.parametrize("chunk", ["1", "7", "1000", "1500", "100000", "0", "x"])
def test_field_chunk_lengths(rig64, monkeypatch, chunk):
    monkeypatch.setenv("VOFOD_MATCH_CHUNK", chunk)
    c = tm.case_of(rig64, "motion")
    d2 = own_field(rig64, c)
    assert_same(rig64.dev.map_match_field(rig64.scan(c.scan), c.tfs, d2, NEAR2, OUTSIDE_COST), expected(c, "own", d2), None, f"chunk {chunk}")


def test_a_sum_beyond_32_bits_comes_back_exact(hip, monkeypatch):
    """300 x 256 returns in ONE chunk, every one of them in a voxel that holds 65535: a lane's sum is 76 800 x 65 535 > 2^32"""
    monkeypatch.setenv("VOFOD_MATCH_CHUNK", "100000")
    w, h = 300, 256
    dirs = mrc.sim_lut(w, h)
    dev = mrc.make_det(hip, w, h, (5.0, 3.0, 2.0), 0.25, dirs)
    try:
        g = mrc.geom(dev, dirs)
        centre = mm.centre_pose(g)
        near, far = centre.copy(), centre.copy()
        near[0, 3] += F(0.1)
        far[0, 3] += F(1000.0)
        tfs = np.stack([far, centre, near])
        scan = mm.SimpleNamespace(range=np.full(w * h, 200, np.uint32), col_tfs=None, xyz=None)
        field = np.full(int(np.prod(g.size)), 65535, np.uint16)
        exp = md.field_statement(g, field, scan, tfs, 65534, 65535)
        assert exp.cost.tolist() == [76800 * 65535] * 3 and 76800 * 65535 > 2**32 and exp.counts.tolist() == [[0, 76800, 0, 0], [0, 0, 76800, 0], [0, 0, 76800, 0]]
        got = dev.map_match_field(ScanData.range_image(scan.range, w, h), tfs, field, 65534, 65535)
        assert_same(got, exp, None, "the wrap case")
        assert got.best == 0
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ interface
def _raw(dev, scan, tfs, n_poses, d2, n, memspace, near2, oc, counts, cost, best, null_h=False):
    cs = scan.as_c() if scan is not None else None
    as_ptr = lambda a: None if a is None else a if isinstance(a, C.c_void_p) else capi.ptr(a)
    return dev.lib.map_match_field(None if null_h else dev.h, None if cs is None else C.byref(cs), as_ptr(tfs), n_poses, as_ptr(d2), n, memspace, near2, oc, as_ptr(counts), as_ptr(cost),
                                   None if best is None else C.byref(best))


def test_field_best_null_and_no_stale_counts_or_costs(rig24):
    rig, c = rig24, tm.case_of(rig24, "motion")
    d2 = own_field(rig, c)
    exp = expected(c, "own", d2)
    scan, tfs, n = rig.scan(c.scan), np.ascontiguousarray(c.tfs, F), d2.size
    counts, cost = np.full((300, 4), tm.CANARY, np.uint32), np.full(300, 2**64 - 7, np.uint64)
    assert _raw(rig.dev, scan, tfs, 300, d2, n, capi.MEM_HOST, NEAR2, OUTSIDE_COST, counts, cost, None) == capi.OK
    np.testing.assert_array_equal(counts, exp.counts)
    np.testing.assert_array_equal(cost, exp.cost)
    for _ in range(2):  # fewer poses afterwards, twice: nothing of the longer call is left, nothing behind the answer is written
        counts, cost, best = np.full((300, 4), tm.CANARY, np.uint32), np.full(300, 2**64 - 7, np.uint64), C.c_int32(-7)
        assert _raw(rig.dev, scan, tfs[20:], 11, d2, n, capi.MEM_HOST, NEAR2, OUTSIDE_COST, counts, cost, best) == capi.OK
        np.testing.assert_array_equal(counts[:11], exp.counts[20:31])
        np.testing.assert_array_equal(cost[:11], exp.cost[20:31])
        assert (counts[11:] == tm.CANARY).all() and (cost[11:] == 2**64 - 7).all() and best.value == int(np.argmin(exp.cost[20:31]))
    twice = np.concatenate([tfs[:9], tfs[:9]])  # ties: the smallest k
    assert rig.dev.map_match_field(scan, twice, d2, NEAR2, OUTSIDE_COST).best == int(np.argmin(exp.cost[:9]))


def test_field_refusals_leave_the_outputs_untouched(rig24):
    rig, c = rig24, tm.case_of(rig24, "motion")
    dev, tfs = rig.dev, np.ascontiguousarray(c.tfs[:5], F)
    field = md.random_field(int(np.prod(c.g.size)), 1)
    dfield = rig.mem.put(field.view(np.uint8))
    host, devs = rig.scan(c.scan), rig.scan(c.scan, "dev", 48, 4)
    pts = mm.SimpleNamespace(range=None, col_tfs=None, xyz=mm.scan_points(c.g, c.scan, c.lo, c.hi)[0])
    hpts, dpts = rig.scan(pts), rig.scan(pts, "dev", 48)

    def call(scan=host, tfs=tfs, n_poses=5, d2=field, n=field.size, memspace=capi.MEM_HOST, near2=3, oc=9, null_counts=False, null_cost=False, null_h=False):
        counts, cost, best = np.full((5, 4), tm.CANARY, np.uint32), np.full(5, 2**64 - 7, np.uint64), C.c_int32(-7)
        st = _raw(dev, scan, tfs, n_poses, d2, n, memspace, near2, oc, None if null_counts else counts, None if null_cost else cost, best, null_h)
        assert st == capi.OK or ((counts == tm.CANARY).all() and (cost == 2**64 - 7).all() and best.value == -7)
        return st

    def edited(s, **kw):
        return ScanData(**{**s.__dict__, **kw})

    INV = capi.ERR_INVALID_ARG
    assert call() == capi.OK and call(d2=C.c_void_p(dfield), memspace=capi.MEM_DEVICE) == capi.OK
    # MAP MATCH's refusals
    assert call(null_h=True) == INV and call(scan=None) == INV and call(tfs=None) == INV and call(null_counts=True) == INV
    assert call(n_poses=0) == INV and call(n_poses=65536) == INV
    assert call(scan=edited(host, memspace=7)) == INV
    assert call(scan=edited(hpts, x=None)) == INV and call(scan=edited(hpts, y=None, z=None)) == INV and call(scan=edited(host, range=None)) == INV
    for on in (True, False):
        dev.set_point_motion(on)
        assert call(scan=edited(hpts, col_tfs=host.col_tfs)) == INV
    assert call(scan=edited(devs, range=int(devs.range) + 2)) == INV and call(scan=edited(devs, stride_bytes=6)) == INV
    assert call(scan=edited(dpts, y=int(dpts.y) + 1)) == INV and call(scan=edited(dpts, stride_bytes=50)) == INV
    assert call(scan=edited(devs, col_tfs=int(devs.col_tfs) + 2)) == INV
    assert call(scan=edited(host, width=c.w + 1)) == capi.ERR_SIZE_MISMATCH and call(scan=edited(hpts, height=c.h - 1)) == capi.ERR_SIZE_MISMATCH
    # the field's own
    assert call(d2=None) == INV and call(null_cost=True) == INV
    assert call(memspace=7) == INV and call(memspace=-1) == INV
    assert call(d2=C.c_void_p(dfield + 1), memspace=capi.MEM_DEVICE) == INV
    assert call(oc=65536) == INV and call(oc=0xFFFFFFFF) == INV
    assert call(n=field.size - 1) == capi.ERR_SIZE_MISMATCH and call(n=field.size + 1) == capi.ERR_SIZE_MISMATCH
    # what is no refusal: any near2, the largest outside_cost, a host field on an odd address, a candidate far outside the map
    assert call(near2=0xFFFFFFFF) == capi.OK and call(oc=65535) == capi.OK
    odd = np.zeros(2 * field.size + 1, np.uint8)
    assert call(d2=C.c_void_p(odd.ctypes.data + 1)) == capi.OK
    far = tfs.copy()
    far[:, :, 3] += 1000.0
    assert call(tfs=far) == capi.OK


# ------------------------------------------------------------------------------------------------ admission and state
@pytest.fixture(scope="module")
def warmed(hip):
    """the warmed OS1-16 handle of the map-shift tests: ground plane, a floating box, 0.5 m voxels, 241 x 201 x 51"""
    import map_shift_cases as mc

    dev = mc.make_det(hip, max_batch=2)
    dev.load_apriori(mc.ground_apriori())
    scans = mc.scans(mc.TARGET_IN_AREA, 0, mc.N_WARM + 2)
    dirs = synth.sim_lut(1024, 16, float(F(np.deg2rad(33.2))))
    yield mm.SimpleNamespace(dev=dev, scans=scans, dirs=dirs, mc=mc)
    dev.close()


def _both_are_the_statement(f, mem, dbuf, case):
    """the distance of the handle's 2.5 M voxels at radius 3 - against scipy's exact transform everywhere (held equal to the brute
    force on every small map by test_map_distance_cpu.py) and against the brute force itself at 48 voxels next to the occupied
    ones and 16 anywhere - to the host and to the device, the same bits; then a scan under a 3 x 3 x 2 lattice with three yaws by
    that field, host and device, against the statement"""
    dev = f.dev
    thr = float(dev.dp.voxel_map__thresholds__new_obstacles)
    g = mrc.geom(dev, f.dirs)  # (the offset moves with a shift)
    m = dev.read_map()
    d2 = dev.map_distance(thr, 3)
    np.testing.assert_array_equal(d2, md.distance_edt(m, thr, 3), err_msg=f"{case}: distance")
    occ = np.argwhere(md.occupied(m, thr)).astype(np.int64)
    assert 100 < len(occ) < m.size // 2
    rs = np.random.default_rng(len(case))
    shape = np.array(m.shape)
    sample = np.concatenate([np.clip(occ[rs.integers(0, len(occ), 48)] + rs.integers(-4, 5, (48, 3)), 0, shape - 1), rs.integers(0, shape, (16, 3))])
    for z, y, x in sample:
        d = occ - np.array([z, y, x])
        assert d2[z, y, x] == min(9, int((d * d).sum(axis=1).min())), (case, z, y, x)
    assert dev.map_distance(thr, 3, device=dbuf) is None
    np.testing.assert_array_equal(mem.get(dbuf, d2.size, np.uint16), d2.reshape(-1), err_msg=f"{case}: device output")
    lo, hi = rm.exclude_bounds(dev.sp)
    s = f.scans[2]
    rng = np.ascontiguousarray(s.scan.range, np.uint32)
    tfs = pose_lattice(dev.lib, s.tf, (0.5, 0.5, 0.5), (3, 3, 2), 0.05, 3)
    exp = md.field_statement(g, d2, mm.SimpleNamespace(range=rng, col_tfs=None, xyz=None), tfs, 1, 9, lo, hi)
    assert exp.counts[:, 2:].any(axis=0).all()  # (NEAR and FAR both occur)
    scan = ScanData.range_image(rng, 1024, 16)
    assert_same(dev.map_match_field(scan, tfs, d2, 1, 9), exp, None, f"{case}: host field")
    assert_same(dev.map_match_field(scan, tfs, dbuf, 1, 9), exp, None, f"{case}: device field")


def test_state_routes_and_admission(warmed, mem):
    f, dev, mc = warmed, warmed.dev, warmed.mc
    s = f.scans
    dbuf = mem.empty(2 * dev.n_voxels)
    dev.process_scan(s[0].scan, s[0].tf)
    _both_are_the_statement(f, mem, dbuf, "after apriori + scan")
    # ---- the launches of a call, under their own names; the other entries' launches as they were
    one = ScanData.range_image(np.ascontiguousarray(s[0].scan.range, np.uint32), 1024, 16)
    for R in (1, 8, 64, 255):  # (every instantiation of the y pass)
        _, names = tm._profiled(dev, lambda: dev.map_distance(0.0, R, device=dbuf))
        assert names == {"k_match_bits": 1, "k_dist_x": 1, "k_dist_y": 1, "k_dist_z": 1}, (R, names)
    _, names = tm._profiled(dev, lambda: dev.map_distance(0.0, 8))
    assert names == {"k_match_bits": 1, "k_dist_x": 1, "k_dist_y": 1, "k_dist_z": 1}, names
    for tfs in (s[0].tf[None], pose_lattice(dev.lib, s[0].tf, (0.5,) * 3, (9, 9, 5), 0.02, 3)):
        _, names = tm._profiled(dev, lambda: dev.map_match_field(one, tfs, dbuf, 4, 64))
        assert names == {"k_match_points": 1, "k_match_field": 1}, names
    _, names = tm._profiled(dev, lambda: dev.map_match(one, s[0].tf[None], 0.0))
    assert names == {"k_match_bits": 1, "k_match_points": 1, "k_match_score": 1}, names
    _, a = tm._profiled(dev, lambda: dev.process_scan(s[0].scan, s[0].tf))
    dev.map_distance(0.0, 8, device=dbuf)
    dev.map_match_field(one, s[0].tf[None], dbuf, 4, 64)
    _, b = tm._profiled(dev, lambda: dev.process_scan(s[0].scan, s[0].tf))
    assert a == b and not any(k.startswith(("k_match", "k_dist")) for k in a), (a, b)
    for k in range(1, mc.N_WARM):
        dev.process_scan(s[k].scan, s[k].tf, flags=capi.SCAN_AUTO_RAYCAST)
    if dev.status().raycast_pending:
        dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION, capi.ERR_RAYCAST_EMPTY))
    maps = lambda: [mc.read_bits(dev, w) for w in (capi.MAP_VOXELS, capi.MAP_FLAGS)]
    # ---- two tickets in flight: admitted, correct, the maps untouched, the collects answer alike
    batch, btf = [s[mc.N_WARM].scan, s[mc.N_WARM + 1].scan], np.stack([s[mc.N_WARM].tf, s[mc.N_WARM + 1].tf])
    t0, t1 = dev.batch_submit(batch, btf), dev.batch_submit(batch, btf)
    before = maps()
    _both_are_the_statement(f, mem, dbuf, "tickets in flight")
    d1, p1 = dev.batch_collect(t1)
    d0, p0 = dev.batch_collect(t0)
    for x, y in zip(before, maps()):
        np.testing.assert_array_equal(x, y)
    assert len(d0) == len(d1) and p0.tolist() == p1.tolist()
    # ---- an exact raycast pass pending: admitted, the accumulator and the maps untouched, the pass still pending, then finished
    dev.set_raycast_exact(True)
    dev.raycast_begin(s[3].scan, s[3].tf)
    assert dev.status().raycast_pending
    before, acc = maps(), dev.raycast_units()[0]
    assert (acc != 0).any()
    _both_are_the_statement(f, mem, dbuf, "exact raycast pass pending")
    assert dev.status().raycast_pending
    np.testing.assert_array_equal(acc, dev.raycast_units()[0])
    for x, y in zip(before, maps()):
        np.testing.assert_array_equal(x, y)
    dev.process_scan(s[4].scan, s[4].tf)  # (the scan whose detections the pass is finished for)
    assert dev.raycast_finish() == capi.OK
    dev.set_raycast_exact(False)
    # ---- a sepclusters pass pending: the same
    st, sure = dev.sepclusters_begin()
    assert st == capi.OK and sure, (st, sure)  # (the warmed field has sure background: the pass IS pending here)
    before = maps()
    _both_are_the_statement(f, mem, dbuf, "sepclusters pass pending")
    for x, y in zip(before, maps()):
        np.testing.assert_array_equal(x, y)
    assert dev.sepclusters_finish() == capi.OK
    # ---- after vofod_map_shift
    base = tuple(dev.sp.oparea_offset)
    assert dev.map_shift((2, -1, 0), mc.shifted_offset(base, (2, -1, 0), mc.VS)) == capi.OK
    _both_are_the_statement(f, mem, dbuf, "after map_shift")
    # ---- with the world store: the window is transformed
    assert dev.world_enable((8, 8, 0), (8, 8, 0), 4096) == capi.OK
    base = tuple(dev.sp.oparea_offset)
    assert dev.map_shift((-3, 2, 0), mc.shifted_offset(base, (-3, 2, 0), mc.VS)) == capi.OK
    _both_are_the_statement(f, mem, dbuf, "world store, after a shift")
    assert dev.world_disable() == capi.OK


# ------------------------------------------------------------------------------------------------ end to end
def test_the_cost_is_lowest_at_the_centre_of_the_lattice(hip):
    """the scan rendered from pose P by the device, the field of the same map by the device, the 5 x 5 x 3 lattice with 3 yaws
    around P: field, counts and costs bit for bit, and best == the centre"""
    c = md.e2e_field_case()
    e = c.e
    dev = mm.make_det(hip, mm.E2E_NAME, e.dirs)
    try:
        dev.write_map(capi.MAP_VOXELS, e.map)
        rng = dev.map_render(e.P[None], mm.E2E_THRESHOLD, mm.E2E_LENGTH)[0]
        np.testing.assert_array_equal(rng[0], e.range)
        d2 = dev.map_distance(mm.E2E_THRESHOLD, md.E2E_RADIUS)
        np.testing.assert_array_equal(d2, c.d2)
        got = dev.map_match_field(synth.scan_from_render(rng[0]), e.tfs, d2, md.E2E_NEAR2, md.E2E_OUTSIDE_COST)
        assert_same(got, c.exp, None, "end to end")
        assert got.best == e.centre
    finally:
        dev.close()
