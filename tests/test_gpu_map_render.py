"""vofod_map_render on the device: every output against the numpy statement (map_render_cases.py) bit for bit - shapes at which
strides, tails and views can go wrong, every burst length, both memspaces, every refusal, the handle states the call is admitted
in, its one launch, and the rendered scan fed back into the raycast role and the detection pipeline."""
import numpy as np
import pytest

import map_render_cases as mrc
from vofod_amd import capi, synth
from vofod_amd.detector import ouster_lut

pytestmark = pytest.mark.gpu
F = np.float32
BURSTS = (1, 2, 4, 8)


def _check(dev, g, m, tfs, thr, length, case, **kw):
    dev.write_map(capi.MAP_VOXELS, m)
    exp = mrc.render(g, m, tfs, thr, length, **kw)
    mrc.assert_same(dev.map_render(tfs, thr, length), exp, case)
    return exp


# ------------------------------------------------------------------------------------------------ hand cases
@pytest.mark.parametrize("case", mrc.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(hip, case):
    name, direction, tf, cells, thr, length, what, voxel, t_in, t_out, rng = case
    dev = mrc.hand_det(hip, direction)
    try:
        dev.write_map(capi.MAP_VOXELS, mrc.hand_map(cells))
        r, v, w, t = dev.map_render(tf, thr, length)
        assert r.shape == v.shape == w.shape == (1, 2, 2) and t.shape == (1, 2, 2, 2)
        assert (w == what).all() and (v == voxel).all() and (r == rng).all(), (w, v, r)
        assert (t[..., 0] == F(t_in)).all() and (t[..., 1] == F(t_out)).all(), t
    finally:
        dev.close()


def test_not_cast_and_the_range_floor(hip):
    tf = mrc.pose((-0.75, 0.0, 0.25))
    dev = mrc.hand_det(hip, (1.0, 0.0, 0.0), offs=(-1.0, 0.0, 0.0))  # the beam's offset puts the start at x = -1.75: outside
    try:
        dev.write_map(capi.MAP_VOXELS, mrc.hand_map({(0, 1, 0): 1.0}))
        r, v, w, t = dev.map_render(tf, 0.0, 10.0)
        assert (w == mrc.NOT_CAST).all() and (v == mrc.NO_VOXEL).all() and (r == 0).all() and (t == 0).all()
    finally:
        dev.close()
    dev = mrc.hand_det(hip, (1.0, 0.0, 0.0))
    try:
        dev.write_map(capi.MAP_VOXELS, mrc.hand_map({(0, 1, 0): 1.0}))
        r, v, w, t = dev.map_render(tf, 0.0, 0.001)
        assert (w == mrc.HIT).all() and (r == 1).all() and (t[..., 1] == F(0.001)).all()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ shapes
# (w, h, area, voxel size) -> map: 9 x 9 x 9, 21 x 13 x 9 (three different extents: a swapped stride shows), 121 x 81 x 33 once
SMALL = (16, 8, (4.0, 4.0, 4.0), 0.5)      # 128 rays: less than a block
RAGGED = (20, 7, (5.0, 3.0, 2.0), 0.25)    # 140 rays: a wave with a ragged tail; 21 x 13 x 9 at 0.25 m
LARGE = (64, 16, (30.0, 20.0, 8.0), 0.25)  # 1024 rays: four blocks; 121 x 81 x 33


def _poses_of(g):
    sx, sy, sz = g.size
    c = mrc.voxel_centre(g, sx // 2, sy // 2, sz // 2)
    out = {"centred": mrc.pose(c), "rotated": mrc.pose(c + 0.07, yaw=0.7, pitch=-0.4, roll=0.2)}
    for k, (ix, iy, iz) in enumerate([(x, y, z) for x in (0, sx - 1) for y in (0, sy - 1) for z in (0, sz - 1)]):
        out[f"corner {k}"] = mrc.pose(mrc.voxel_centre(g, ix, iy, iz) + 0.03, yaw=0.4 * k)
    face = mrc.voxel_centre(g, sx // 2, sy // 2, sz // 2)
    face[0] = float(g.off[0]) + float(g.vs) * 3  # exactly on a voxel face
    out["on a face"] = mrc.pose(face, yaw=-1.1)
    return out


@pytest.fixture(scope="module")
def small(hip):
    w, h, area, vs = SMALL
    dirs = mrc.sim_lut(w, h)
    dev = mrc.make_det(hip, w, h, area, vs, dirs)
    assert dev.map_size == (9, 9, 9)
    yield dev, mrc.geom(dev, dirs)
    dev.close()


@pytest.fixture(scope="module")
def ragged(hip):
    w, h, area, vs = RAGGED
    az = np.linspace(360.0, 0.0, w, endpoint=False)
    alt = np.linspace(20.0, -20.0, h)
    dirs, offs = ouster_lut(hip, w, h, az, alt, origin_mm=27.67)  # an Ouster LUT: unit directions and non-zero beam offsets
    offs = (offs + F(0.01)).astype(F)
    assert np.abs(offs).max() > 0
    dev = mrc.make_det(hip, w, h, area, vs, dirs, offs)
    assert dev.map_size == (21, 13, 9)
    yield dev, mrc.geom(dev, dirs, offs)
    dev.close()


@pytest.mark.parametrize("burst", BURSTS)
def test_random_maps_all_poses_every_burst(small, monkeypatch, burst):
    """a fifth of the voxels over the threshold, NaN, +inf, -0.0 and threshold-equal values sprinkled in; centred, every corner
    voxel, on a face, rotated - as 11 views of one call; max_distance beyond the map's diagonal"""
    monkeypatch.setenv("VOFOD_RENDER_BURST", str(burst))
    dev, g = small
    tfs = np.stack(list(_poses_of(g).values()))
    thr = -0.0
    exp = _check(dev, g, mrc.random_map(g.size, 11, thr), tfs, thr, 50.0, f"burst {burst}")
    assert {int(x) for x in np.unique(exp.what)} >= {mrc.HIT, mrc.LEFT}


@pytest.mark.parametrize("burst", BURSTS)
def test_ragged_sensor_ouster_lut_three_extents(ragged, monkeypatch, burst):
    monkeypatch.setenv("VOFOD_RENDER_BURST", str(burst))
    dev, g = ragged
    p = _poses_of(g)
    for n_views in (1, 3, 5):
        tfs = np.stack(list(p.values())[:n_views])
        exp = _check(dev, g, mrc.random_map(g.size, 20 + n_views, 0.5, frac=0.05), tfs, 0.5, 1.6, f"{n_views} views, burst {burst}")
        assert {int(x) for x in np.unique(exp.what)} >= {mrc.HIT, mrc.END}


def test_large_map_and_sensor_once(hip):
    w, h, area, vs = LARGE
    dirs = mrc.sim_lut(w, h)
    dev = mrc.make_det(hip, w, h, area, vs, dirs)
    try:
        assert dev.map_size == (121, 81, 33)
        g = mrc.geom(dev, dirs)
        tfs = np.stack([mrc.pose(mrc.voxel_centre(g, 60, 40, 16), yaw=0.2, pitch=0.1), mrc.pose(mrc.voxel_centre(g, 3, 77, 30), roll=0.3)])
        exp = _check(dev, g, mrc.random_map(g.size, 3, 0.0, frac=0.01), tfs, 0.0, 12.0, "large")
        assert {int(x) for x in np.unique(exp.what)} == {mrc.HIT, mrc.END, mrc.LEFT}
    finally:
        dev.close()


def test_empty_solid_short_and_axis_aligned(small, hip):
    dev, g = small
    tfs = np.stack([_poses_of(g)[k] for k in ("centred", "corner 3", "rotated")])
    empty = np.full(g.size[::-1], -1.0, F)
    exp = _check(dev, g, empty, tfs, 0.0, 1.7, "empty map")
    assert set(np.unique(exp.what).tolist()) == {mrc.END, mrc.LEFT}
    exp = _check(dev, g, np.full(g.size[::-1], 3.0, F), tfs, 0.0, 50.0, "solid map")
    assert (exp.what == mrc.HIT).all() and (exp.tio[..., 0] == 0).all() and (exp.range >= 1).all()
    exp = _check(dev, g, empty, tfs, 0.0, 0.2, "max_distance below one voxel")
    assert (exp.what == mrc.END).all()
    # an axis-aligned LUT: zero direction components, tdelta = inf on two axes
    w, h = SMALL[0], SMALL[1]
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0.6, 0.8), (0.0, 0.0, 0.0)], F)
    dirs = np.tile(axes, (w * h // len(axes), 1))
    dev2 = mrc.make_det(hip, w, h, SMALL[2], SMALL[3], dirs)
    try:
        g2 = mrc.geom(dev2, dirs)
        _check(dev2, g2, mrc.random_map(g2.size, 8, 0.0, frac=0.1), np.stack([mrc.pose(mrc.voxel_centre(g2, 4, 4, 4)), mrc.pose(mrc.voxel_centre(g2, 1, 7, 2) + 0.1)]), 0.0, 30.0, "axis-aligned")
    finally:
        dev2.close()


@pytest.mark.parametrize("burst", BURSTS)
def test_burst_boundaries(small, monkeypatch, burst):
    """rays whose hit is the 1st .. 10th voxel visited and rays whose END or LEFT falls on the 1st .. 10th: every position of a
    burst of every length and the step behind it, built from the statement's visited lists"""
    monkeypatch.setenv("VOFOD_RENDER_BURST", str(burst))
    dev, g = small
    # from a corner column (walks of up to 19 voxels), from the middle and from between: LEFT after 1 .. 10 voxels
    tf = np.stack([mrc.pose(mrc.voxel_centre(g, 0, 0, 4) + 0.05, yaw=0.1), mrc.pose(mrc.voxel_centre(g, 4, 4, 4)), mrc.pose(mrc.voxel_centre(g, 2, 6, 3) - 0.1, yaw=2.0, pitch=0.2)])
    empty = np.full(g.size[::-1], -1.0, F)
    base = mrc.render(g, empty, tf, 0.0, 50.0, want_visited=True)
    all_rays = lambda r: [v for view in r.visited for v in view]
    lengths = [len(v) for v in all_rays(base)]
    assert max(lengths) >= 10 and set(range(1, 10)) <= set(lengths), sorted(set(lengths))  # LEFT on every position
    seen_hit, seen_end = set(), set()
    for pos in range(1, 11):
        m = empty.copy()
        blocked = set()
        for vis in all_rays(base):
            # the pos-th voxel of every ray that has one and whose earlier voxels stay free becomes a hit
            if len(vis) >= pos and not any(lin in blocked for lin, _ in vis[: pos - 1]):
                blocked.add(vis[pos - 1][0])
        m.reshape(-1)[list(blocked)] = 1.0
        exp = _check(dev, g, m, tf, 0.0, 50.0, f"hit on voxel {pos}, burst {burst}", want_visited=True)
        seen_hit |= {len(v) for v, w in zip(all_rays(exp), exp.what.reshape(-1)) if w == mrc.HIT}
        # END on the pos-th voxel: a length that runs out inside it
        vis = max(all_rays(base), key=len)
        length = float(sum(dd for _, dd in vis[: pos - 1]) + vis[pos - 1][1] * F(0.5))
        exp = _check(dev, g, empty, tf, 0.0, length, f"END near voxel {pos}, burst {burst}", want_visited=True)
        seen_end |= {len(v) for v, w in zip(all_rays(exp), exp.what.reshape(-1)) if w == mrc.END}
    assert set(range(1, 10)) <= seen_hit and set(range(1, 10)) <= seen_end, (sorted(seen_hit), sorted(seen_end))


# ------------------------------------------------------------------------------------------------ memspaces, options, refusals
def test_device_outputs_null_outputs_and_misalignment(small):
    from test_gpu_range_image import DeviceMem

    dev, g = small
    tfs = np.stack([_poses_of(g)[k] for k in ("centred", "rotated", "corner 5")])
    m = mrc.random_map(g.size, 4, 0.0)
    exp = _check(dev, g, m, tfs, 0.0, 50.0, "host")
    n = exp.what.size
    want = (exp.range.view(np.uint8), exp.voxel.view(np.uint8), exp.what.view(np.uint8), exp.tio.view(np.uint8))
    sizes = (4 * n, 4 * n, n, 8 * n)
    CANARY = 0xA5
    mem = DeviceMem()
    try:
        fresh = lambda: [mem.put(np.full(s + 32, CANARY, np.uint8)) for s in sizes]
        # all four in place, at bases that are 4 / 4 / 1 / 8-byte but not 16-byte aligned
        addr = fresh()
        shift = (4, 12, 3, 8)
        assert dev.map_render(tfs, 0.0, 50.0, out=tuple(a + s for a, s in zip(addr, shift))) is None
        for a, s, size, w in zip(addr, shift, sizes, want):
            got = mem.get(a, size + 32, dtype=np.uint8)
            assert got[s : s + size].tobytes() == w.tobytes() and (got[:s] == CANARY).all() and (got[s + size :] == CANARY).all()
        # each output NULL in turn: the other three arrive, on the device and on the host
        for skip in range(4):
            addr = fresh()
            assert dev.map_render(tfs, 0.0, 50.0, out=tuple(None if k == skip else a + 8 for k, a in enumerate(addr))) is None
            for k, (a, size, w) in enumerate(zip(addr, sizes, want)):
                got = mem.get(a, size + 32, dtype=np.uint8)
                assert (got == CANARY).all() if k == skip else got[8 : 8 + size].tobytes() == w.tobytes()
            host = [np.full(s, CANARY, np.uint8) for s in sizes]
            ptrs = [None if k == skip else capi.ptr(b) for k, b in enumerate(host)]
            assert dev.lib.map_render(dev.h, capi.ptr(tfs), len(tfs), 0.0, 50.0, *ptrs, capi.MEM_HOST) == capi.OK
            for k, (b, w) in enumerate(zip(host, want)):
                assert (b == CANARY).all() if k == skip else b.tobytes() == w.tobytes()
        # a misaligned device base is refused, nothing written
        addr = fresh()
        for bad in ((2, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 4)):
            out = tuple(a + 16 + b for a, b in zip(addr, bad))
            assert dev.map_render(tfs, 0.0, 50.0, out=out, allow=(capi.ERR_INVALID_ARG,)) == capi.ERR_INVALID_ARG, bad
        for a, size in zip(addr, sizes):
            assert (mem.get(a, size + 32, dtype=np.uint8) == CANARY).all()
    finally:
        mem.free()


def test_refusals_leave_the_outputs_untouched(small):
    dev, g = small
    tf = _poses_of(g)["centred"][None]
    n = g.h * g.w
    bufs = lambda: [np.full(n, 0xDEADBEEF, np.uint32), np.full(n, 0xDEADBEEF, np.uint32), np.full(n, 0xA5, np.uint8), np.full(2 * n, 0xDEADBEEF, np.uint32)]
    outside = tf.copy()
    outside[0, 0, 3] = float(g.off[0]) - 0.1
    two = np.concatenate([tf, outside])  # the second view's origin lies outside: the whole call is refused
    cases = [
        ("n_views == 0", lambda b: dev.lib.map_render(dev.h, capi.ptr(tf), 0, 0.0, 5.0, *map(capi.ptr, b), capi.MEM_HOST), capi.ERR_INVALID_ARG),
        ("tfs == NULL", lambda b: dev.lib.map_render(dev.h, None, 1, 0.0, 5.0, *map(capi.ptr, b), capi.MEM_HOST), capi.ERR_INVALID_ARG),
        ("max_distance == 0", lambda b: dev.lib.map_render(dev.h, capi.ptr(tf), 1, 0.0, 0.0, *map(capi.ptr, b), capi.MEM_HOST), capi.ERR_INVALID_ARG),
        ("max_distance < 0", lambda b: dev.lib.map_render(dev.h, capi.ptr(tf), 1, 0.0, -1.0, *map(capi.ptr, b), capi.MEM_HOST), capi.ERR_INVALID_ARG),
        ("max_distance NaN", lambda b: dev.lib.map_render(dev.h, capi.ptr(tf), 1, 0.0, float("nan"), *map(capi.ptr, b), capi.MEM_HOST), capi.ERR_INVALID_ARG),
        ("threshold NaN", lambda b: dev.lib.map_render(dev.h, capi.ptr(tf), 1, float("nan"), 5.0, *map(capi.ptr, b), capi.MEM_HOST), capi.ERR_INVALID_ARG),
        ("n_views above 65535", lambda b: dev.lib.map_render(dev.h, capi.ptr(tf), 65536, 0.0, 5.0, *map(capi.ptr, b), capi.MEM_HOST), capi.ERR_INVALID_ARG),
        ("unknown memspace", lambda b: dev.lib.map_render(dev.h, capi.ptr(tf), 1, 0.0, 5.0, *map(capi.ptr, b), 7), capi.ERR_INVALID_ARG),
        ("sensor outside", lambda b: dev.lib.map_render(dev.h, capi.ptr(outside), 1, 0.0, 5.0, *map(capi.ptr, b), capi.MEM_HOST), capi.ERR_SENSOR_OUTSIDE_MAP),
        ("second view outside", lambda b: dev.lib.map_render(dev.h, capi.ptr(two), 2, 0.0, 5.0, *map(capi.ptr, b), capi.MEM_HOST), capi.ERR_SENSOR_OUTSIDE_MAP),
    ]
    for name, call, status in cases:
        b = bufs() if name != "second view outside" else [np.concatenate([x, x]) for x in bufs()]
        assert call(b) == status, name
        assert (b[0] == 0xDEADBEEF).all() and (b[1] == 0xDEADBEEF).all() and (b[2] == 0xA5).all() and (b[3] == 0xDEADBEEF).all(), name
    assert dev.lib.map_render(dev.h, capi.ptr(tf), 1, 0.0, 5.0, None, None, None, None, capi.MEM_HOST) == capi.ERR_INVALID_ARG  # all four NULL
    assert dev.lib.map_render(dev.h, capi.ptr(tf), 1, float("inf"), 5.0, *map(capi.ptr, bufs()), capi.MEM_HOST) == capi.OK  # an infinite threshold is a threshold


# ------------------------------------------------------------------------------------------------ routes and state
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
    yield mrc.SimpleNamespace(dev=dev, scans=scans, g=mrc.geom(dev, dirs), mc=mc)
    dev.close()


def _render_is_read_map(f, case, thr=None, length=12.0):
    dev = f.dev
    thr = float(dev.dp.voxel_map__thresholds__new_obstacles) if thr is None else thr
    tfs = np.stack([f.scans[0].tf, f.scans[2].tf])
    g = mrc.geom(dev, f.g.dirs)  # (the offset moves with a shift)
    exp = mrc.render(g, dev.read_map(), tfs, thr, length, pixels=PIX)
    got = dev.map_render(tfs, thr, length)
    mrc.assert_same(got, exp, case, pixels=PIX)
    return exp


def test_state_routes_and_admission(field):
    f, dev, mc = field, field.dev, field.mc
    s = f.scans
    # ---- the routes before the first render (a read-only scan, a batch, a pass that is abandoned: the maps stay as they are)
    dev.process_scan(s[0].scan, s[0].tf)
    routes = lambda: [_profiled(dev, lambda: dev.process_scan(s[1].scan, s[1].tf, flags=capi.SCAN_NO_MAP_UPDATE))[1],
                      _profiled(dev, lambda: dev.process_batch([s[1].scan, s[2].scan], np.stack([s[1].tf, s[2].tf])))[1],
                      _profiled(dev, lambda: (dev.raycast_begin(s[1].scan, s[1].tf), dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION, capi.ERR_RAYCAST_EMPTY))))[1]]
    routes()  # (an abandoned pass leaves the accumulator to be cleared by the next begin: from the second round on the rounds are alike)
    names_before = routes()
    assert all(n and "k_map_render" not in n for n in names_before) and "k_raycast" in names_before[2], names_before
    # ---- after load_apriori and a scan with map update: the render is that of read_map; one launch, no other kernel
    exp = _render_is_read_map(f, "after apriori + scan")
    assert (exp.what.reshape(2, -1)[:, PIX] == mrc.HIT).any()
    tf1 = s[0].tf[None]
    _, names = _profiled(dev, lambda: dev.map_render(tf1, 0.0, 12.0))
    assert names == {"k_map_render": 1}, names
    # ---- the routes after: process_scan, process_batch and raycast_begin launch what they launched before
    assert routes() == names_before
    for k in range(1, mc.N_WARM):
        dev.process_scan(s[k].scan, s[k].tf, flags=capi.SCAN_AUTO_RAYCAST)
    if dev.status().raycast_pending:
        dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION, capi.ERR_RAYCAST_EMPTY))
    _render_is_read_map(f, "after the warm-up")
    # ---- ticket 1 in flight (ticket 0 is taken first): admitted, correct, and the collect answers what the same batch answers afterwards
    batch, btf = [s[mc.N_WARM].scan, s[mc.N_WARM + 1].scan], np.stack([s[mc.N_WARM].tf, s[mc.N_WARM + 1].tf])
    maps = lambda: [mc.read_bits(dev, w) for w in (capi.MAP_VOXELS, capi.MAP_FLAGS)]
    t0, t1 = dev.batch_submit(batch, btf), dev.batch_submit(batch, btf)
    before = maps()
    _render_is_read_map(f, "tickets in flight")
    d1, p1 = dev.batch_collect(t1)
    d0, p0 = dev.batch_collect(t0)
    for a, b in zip(before, maps()):
        np.testing.assert_array_equal(a, b)
    t2 = dev.batch_submit(batch, btf)
    d2, p2 = dev.batch_collect(t2)  # (the same batch without a render in between)
    assert len(d0) == len(d1) == len(d2) and p0.tolist() == p1.tolist() == p2.tolist()
    for k in ("frame", "n_points"):
        np.testing.assert_array_equal(d1[k], d2[k])
    np.testing.assert_allclose(d1["position"], d2["position"], atol=1e-3)  # (the tolerance the parity tests give positions)
    # ---- a raycast pass pending, rigid and exact: admitted, the three maps (the accumulator's units included) untouched, finish as always
    def restore(saved):
        for w, bits in zip((capi.MAP_VOXELS, capi.MAP_FLAGS), saved):
            mc.write_bits(dev, w, bits)

    for exact in (False, True):
        dev.set_raycast_exact(exact)
        start = maps()
        dev.raycast_begin(s[3].scan, s[3].tf)
        raw = lambda: dev.raycast_units()[0] if exact else mc.read_bits(dev, capi.MAP_RAYCAST)
        before, acc = maps(), raw()
        assert (acc != 0).any()
        _render_is_read_map(f, f"raycast pass pending, exact={exact}")
        np.testing.assert_array_equal(acc, raw())
        for a, b in zip(before, maps()):
            np.testing.assert_array_equal(a, b)
        n_det = len(dev.process_scan(s[4].scan, s[4].tf))
        assert dev.raycast_finish() == capi.OK
        _render_is_read_map(f, "after raycast_finish")
        if exact:
            # the same pass from the same maps without a render in between: the exact pass does not depend on the order of its atomics,
            # so the finished maps are the same bits (a float pass sums in the order its atomics arrive: two runs of it may differ in
            # the last bits with or without a render, and the untouched accumulator above is what can be held exactly)
            with_render = maps()
            restore(start)
            dev.raycast_begin(s[3].scan, s[3].tf)
            np.testing.assert_array_equal(acc, raw())
            assert len(dev.process_scan(s[4].scan, s[4].tf)) == n_det
            assert dev.raycast_finish() == capi.OK
            for a, b in zip(with_render, maps()):
                np.testing.assert_array_equal(a, b)
    dev.set_raycast_exact(False)
    # ---- a sepclusters pass pending: admitted, the maps untouched, and the finish leaves the maps it leaves without a render in between
    start = maps()
    st, sure = dev.sepclusters_begin()
    assert st == capi.OK and sure, (st, sure)  # (the warmed field has sure background: the pass IS pending here)
    before = maps()
    _render_is_read_map(f, "sepclusters pass pending")
    for a, b in zip(before, maps()):
        np.testing.assert_array_equal(a, b)
    assert dev.sepclusters_finish() == capi.OK
    with_render = maps()
    restore(start)
    st, sure = dev.sepclusters_begin()
    assert st == capi.OK and sure, (st, sure)
    assert dev.sepclusters_finish() == capi.OK
    for a, b in zip(with_render, maps()):
        np.testing.assert_array_equal(a, b)
    # ---- after vofod_map_shift, and with the world store enabled: the window is rendered
    base = tuple(dev.sp.oparea_offset)
    assert dev.map_shift((2, -1, 0), mc.shifted_offset(base, (2, -1, 0), mc.VS)) == capi.OK
    _render_is_read_map(f, "after map_shift")
    assert dev.world_enable((8, 8, 0), (8, 8, 0), 4096) == capi.OK
    assert dev.map_shift((-3, 2, 0), mc.shifted_offset(tuple(dev.sp.oparea_offset), (-3, 2, 0), mc.VS)) == capi.OK
    exp = _render_is_read_map(f, "world store: the window", length=200.0)
    assert (exp.what.reshape(2, -1)[:, PIX] == mrc.LEFT).any()


# ------------------------------------------------------------------------------------------------ back into the pipeline
W2, H2, AREA2, VS2, MAXD2 = 16, 8, (10.0, 8.0, 4.0), 0.5, 3.5


@pytest.mark.parametrize("exact", [False, True], ids=["rigid", "exact"])
def test_rendered_scan_carves_only_what_the_render_called_free(hip, exact):
    dirs = mrc.sim_lut(W2, H2)
    dev = mrc.make_det(hip, W2, H2, AREA2, VS2, dirs, raycast__max_distance=MAXD2, raycast__min_intensity=10.0)
    try:
        g = mrc.geom(dev, dirs)
        m = mrc.random_map(g.size, 5, 0.0, special=False, frac=0.03)
        tf = mrc.pose(mrc.voxel_centre(g, 10, 8, 4) + (0.13, -0.21, 0.07), yaw=0.7, pitch=-0.4)
        dev.write_map(capi.MAP_VOXELS, m)
        dev.set_raycast_exact(exact)
        rng, vox, what, tio = dev.map_render(tf, 0.0, MAXD2)
        assert (what == mrc.HIT).sum() > 20 and (what != mrc.HIT).sum() > 5
        dev.raycast_begin(synth.scan_from_render(rng[0], intensity=100.0), tf)
        ray = dev.read_map(capi.MAP_RAYCAST)
        dev.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION, capi.ERR_RAYCAST_EMPTY))
        assert (ray != 0).sum() > 50 and (m[ray != 0] <= 0.0).all()
    finally:
        dev.close()


def test_a_rendered_box_comes_back_as_its_detection(hip):
    """the end-to-end scene on the device: render, erase the box, feed the render back as the range image it is - one detection,
    inside the box; the render is the statement's"""
    dev, g = mrc.e2e_det(hip)
    try:
        m, free, tf = mrc.e2e_scene(dev, g)
        thr = dev.dp.voxel_map__thresholds__new_obstacles
        got = dev.map_render(tf, thr, 30.0)
        mrc.assert_same(got, mrc.render(g, m, tf[None], thr, 30.0), "end to end")
        dev.write_map(capi.MAP_VOXELS, free)
        d = dev.process_scan(synth.scan_from_render(got[0][0]), tf)
        assert len(d) == 1, d
        assert all(lo < x < hi for lo, x, hi in zip(mrc.E2E_BOX_MIN, d["position"][0], mrc.E2E_BOX_MAX)), d["position"]
    finally:
        dev.close()
