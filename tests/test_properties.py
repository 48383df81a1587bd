"""Property tests of the oracle: conservation, permutation invariance, clustering vs brute force - and whole
stages of a scan against numpy / scipy.  The statements that go through the C-ABI alone live in tests/statements.py, where
tests/test_gpu_statements.py holds the HIP library to the very same functions; here they run on the oracle."""
import ctypes as C
import math

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import statements
from frame_geometry import FALLBACK_SWITCHES, ROOT, TABLE, capacities, ref_lattice
from vofod_amd import capi


@settings(max_examples=25, deadline=None)
@given(seed=st.integers(0, 10_000), n=st.integers(1, 3000), leaf=st.sampled_from([0.1, 0.25, 0.5, 1.0, 3.0]), aligned=st.booleans())
def test_weighted_grid_conserves_points_and_is_permutation_invariant(oracle, seed, n, leaf, aligned):
    statements.weighted_grid_conserves_points_and_is_permutation_invariant(oracle, seed, n, leaf, aligned)


@settings(max_examples=15, deadline=None)
@given(seed=st.integers(0, 10_000), n=st.integers(1, 2000), thr=st.sampled_from([-100.0, -0.1, 0.5]))
def test_counted_grid_total_is_the_true_total(oracle, seed, n, thr):
    statements.counted_grid_total_is_the_true_total(oracle, seed, n, thr)


@settings(max_examples=15, deadline=None)
@given(seed=st.integers(0, 10_000), n=st.integers(2, 600), tol=st.sampled_from([0.7, 1.5, 2.0]))
def test_cluster_labels_match_bruteforce_union_find(oracle, seed, n, tol):
    pts, labels, nc = statements.cluster_labels_match_scipy_components(oracle, seed, n, tol)
    bf = oracle.extra("vofod_oracle_cluster_bruteforce", C.c_int, [C.c_void_p, C.c_size_t, C.c_float, C.c_void_p])
    ref = np.zeros(len(pts), dtype=np.uint32)
    bf(capi.ptr(pts), len(pts), tol, capi.ptr(ref))
    np.testing.assert_array_equal(labels, ref)
    assert nc == len(np.unique(ref))


def test_sensor_helpers_of_the_product_match_the_oracle(oracle):
    """vofod_ouster_lut / vofod_mask_layout are host code on both sides (no GPU involved): identical outputs"""
    import vofod_amd
    from vofod_amd.detector import mask_layout, ouster_lut

    try:
        hip = vofod_amd.library()
    except (ImportError, OSError) as e:  # libamdhip64 missing on a CPU-only box
        pytest.skip(f"product library not loadable here: {e}")
    rng = np.random.default_rng(11)
    w, h = 64, 16
    az = rng.uniform(-3, 3, h)
    alt = np.linspace(16.6, -16.6, h)
    tf = np.eye(4)
    tf[:3, :3] = [[-1, 0, 0], [0, -1, 0], [0, 0, 1]]
    tf[:3, 3] = [0.0, 0.0, 36.18]
    for kw in ({}, {"tf": tf, "origin_mm": 15.806}):
        a = ouster_lut(oracle, w, h, az, alt, **kw)
        b = ouster_lut(hip, w, h, az, alt, **kw)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    sh = rng.integers(0, 9, h).astype(np.int32)
    np.testing.assert_array_equal(mask_layout(oracle, img, w, h, sh), mask_layout(hip, img, w, h, sh))
    # check_sensor_params: independent implementations (oracle: the reference's statements; product: its own), same verdicts
    from vofod_amd.detector import ScanData, check_sensor_params, sim_lut

    lut = sim_lut(oracle, w, h, 0.58).reshape(h * w, 3)
    for trial in range(40):
        r = rng.integers(0, 60000, h * w).astype(np.uint32)
        r[rng.random(h * w) < 0.3] = 0
        scale = r[:, None].astype(np.float32) * np.float32(0.001)
        p = (lut * scale + rng.normal(0, [0.0, 2e-4, 6e-4, 2e-3][trial % 4], (h * w, 3))).astype(np.float32)
        m = (rng.random(h * w) < 0.8).astype(np.uint8)
        sc = ScanData(x=np.ascontiguousarray(p[:, 0]), y=np.ascontiguousarray(p[:, 1]), z=np.ascontiguousarray(p[:, 2]), width=w, height=h,
                      intensity=np.zeros(h * w, np.float32), range=r, stride_bytes=4)
        assert check_sensor_params(oracle, sc, lut, mask=m) == check_sensor_params(hip, sc, lut, mask=m)


def test_message_serialisation_byte_layout():
    """row N3: vofod/Detections, vofod/Status, vofod/ProfilingInfo in the ROS 1 wire format - expected bytes built by hand
    from msgs/*.msg (little endian, uint32 length prefixes; Header = seq, stamp.sec, stamp.nsec, frame_id)"""
    import ctypes as C
    import struct

    import vofod_amd
    from vofod_amd import capi

    try:
        hip = vofod_amd.library()
    except (ImportError, OSError) as e:
        pytest.skip(f"product library not loadable here: {e}")
    hdr = capi.MsgHeader(7, 1700000000, 250000000, b"uav1/world_origin")
    hdr_bytes = struct.pack("<III", 7, 1700000000, 250000000) + struct.pack("<I", 17) + b"uav1/world_origin"
    dets = np.zeros(2, dtype=capi.DETECTION)
    dets["id"] = [41, 42]
    dets["n_points"] = [9, 3]
    dets["confidence"] = [0.75, 0.5]
    dets["detection_probability"] = [0.9, 0.1]
    dets["position"] = [[1.0, 2.0, 3.0], [-4.0, 5.5, 6.25]]
    dets["covariance"][:, 0] = dets["covariance"][:, 4] = dets["covariance"][:, 8] = [0.3, 0.6]
    want = hdr_bytes + struct.pack("<I", 2)
    for d in dets:
        want += struct.pack("<I", int(d["id"])) + struct.pack("<d", float(d["confidence"])) + struct.pack("<Q", int(d["n_points"]))
        want += struct.pack("<3d", *d["position"]) + struct.pack("<9d", *d["covariance"]) + struct.pack("<d", float(d["detection_probability"]))
    n = C.c_size_t(0)
    assert hip.serialize_detections(C.byref(hdr), capi.ptr(dets), 2, None, 0, C.byref(n)) == capi.ERR_CAPACITY and n.value == len(want)
    buf = np.zeros(n.value, dtype=np.uint8)
    assert hip.serialize_detections(C.byref(hdr), capi.ptr(dets), 2, capi.ptr(buf), buf.size, C.byref(n)) == capi.OK
    assert buf.tobytes() == want
    # Detection.msg: 4 + 8 + 8 + 24 + 72 + 8 bytes per record
    assert len(want) == len(hdr_bytes) + 4 + 2 * 124
    buf = np.zeros(64, dtype=np.uint8)
    assert hip.serialize_status(C.byref(hdr), 1, 0, capi.ptr(buf), buf.size, C.byref(n)) == capi.OK
    assert buf[: n.value].tobytes() == hdr_bytes + bytes([1, 0])
    assert hip.serialize_profiling_info(12, 34, 5, 6, 2, capi.ptr(buf), buf.size, C.byref(n)) == capi.OK
    assert buf[: n.value].tobytes() == struct.pack("<IIIQB", 12, 34, 5, 6, 2) and n.value == 21


@pytest.mark.parametrize("sensor,vs,seed", [("os1-16", 0.5, 3), ("os1-16", 0.25, 4), ("os1-128", 0.5, 5)])
def test_far_clusters_are_the_untainted_components_of_the_far_voxels(oracle, sensor, vs, seed):
    """statements.far_clusters_are_the_untainted_components_of_the_far_voxels on the ORACLE's own output; the per-voxel close bit
    of the dilated occupancy image must also be the oracle's hasCloseTo, voxel by voxel."""

    def has_close_to(det, pts, tol, thr):
        f = oracle.extra("vofod_oracle_map_has_close_to", C.c_int, [C.c_void_p] + [C.c_float] * 5)
        return np.array([bool(f(det.h, float(p[0]), float(p[1]), float(p[2]), float(tol), float(thr))) for p in pts])

    statements.far_clusters_are_the_untainted_components_of_the_far_voxels(oracle, sensor, vs, seed, close_of=has_close_to)


@settings(max_examples=80, deadline=None)
@given(seed=st.integers(0, 100_000), p_unknown=st.sampled_from([0.15, 0.25, 0.3, 0.4, 0.6]), p_ground=st.sampled_from([0.0, 0.01, 0.05]), R=st.integers(2, 14))
def test_explore_to_ground_against_scipy_labelling(oracle, seed, p_unknown, p_ground, R):
    """exploreToGround (voxel_map.cpp:402-488) on random maps against scipy.ndimage: the walk spreads through UNKNOWN voxels
    (unknown_thr < v <= ground_thr, 6-neighbourhood, Manhattan distance <= R from the start); it is "connected" iff a voxel it
    pops lies above the ground threshold or an unknown voxel at distance exactly R - 1 is popped; otherwise it returns the
    unknown voxels it popped (some twice: SURVEY Q7) - as a set, the start's component.  The depth-first order does not matter
    for any of this, which is what the wave-parallel fill of kernels_classify.h relies on."""
    from scipy import ndimage

    from vofod_amd.detector import VoFOD, default_params

    sp, dp = default_params(oracle)
    sp.voxel_size = 0.5
    sp.oparea_offset[:] = (5.0, 5.0, 0.0)
    sp.oparea_size[:] = (10.0, 10.0, 10.0)
    sp.sensor_hrays, sp.sensor_vrays = 8, 2
    det = VoFOD(oracle, sp, dp)
    sx, sy, sz = det.map_size
    rng = np.random.default_rng(seed)
    u = rng.random((sz, sy, sx))
    m = np.full((sz, sy, sx), -1000.0, dtype=np.float32)  # air
    m[u < p_unknown] = -740.0                              # unknown
    m[u > 1.0 - p_ground] = 0.0                            # ground / obstacles
    o = tuple(int(v) for v in rng.integers(3, [sx - 3, sy - 3, sz - 3]))
    if rng.random() < 0.8:
        m[o[2], o[1], o[0]] = -740.0
    det.write_map(capi.MAP_VOXELS, m)
    f = oracle.extra("vofod_oracle_map_explore_to_ground", C.c_int, [C.c_void_p] + [C.c_float] * 6 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)])
    buf = np.zeros((8192, 3), dtype=np.int32)
    n = C.c_size_t(0)
    off = det.map_offset
    c = [off[a] + (o[a] + 0.5) * 0.5 for a in range(3)]
    conn = bool(f(det.h, c[0], c[1], c[2], -750.0, -300.0, float(R), capi.ptr(buf), 8192, C.byref(n)))
    got = {tuple(r) for r in buf[: n.value].tolist()}

    zz, yy, xx = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    manh = np.abs(xx - o[0]) + np.abs(yy - o[1]) + np.abs(zz - o[2])
    ball = manh <= R
    unknown = (m > -750.0) & (m <= -300.0)
    ground = m > -300.0
    start_unknown = bool(unknown[o[2], o[1], o[0]])
    if ground[o[2], o[1], o[0]]:
        want_conn, want = True, set()
    elif not start_unknown:
        want_conn, want = False, set()  # popped, neither ground nor unknown: nothing spreads
    else:
        lab, _ = ndimage.label(unknown & ball)  # 6-neighbourhood by default
        comp = lab == lab[o[2], o[1], o[0]]
        popped = ndimage.binary_dilation(comp) & ball  # the component and everything it pushes
        want_conn = bool((popped & ground).any() or (comp & (manh == R - 1)).any())
        want = set() if want_conn else {(int(x), int(y), int(z)) for z, y, x in zip(*np.nonzero(comp))}
    assert conn == want_conn
    assert got == want
    det.close()


@settings(max_examples=150, deadline=None)
@given(seed=st.integers(0, 1_000_000), length=st.floats(0.05, 9.0))
def test_ray_walk_is_the_geometric_intersection_of_the_segment_with_the_lattice(oracle, seed, length):
    """forEachRay (voxel_map.cpp:229-263, Amanatides-Woo) for random rays inside the default map, against plain geometry: the
    pieces tile the segment (their lengths are >= 0 and sum to the ray's length), consecutive voxels differ by one step along one
    axis in the ray's direction, and the middle of every piece of positive length lies inside the voxel it was charged to."""
    from vofod_amd.detector import VoFOD

    big = VoFOD(oracle)  # 241 x 201 x 51 voxels of 0.5 m, offset (-20, -30, -1.25)
    f = oracle.extra("vofod_oracle_map_ray", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)])
    rng = np.random.default_rng(seed)
    off = np.float64(big.map_offset)
    start = (off + np.float64([40.0, 40.0, 12.0]) + rng.uniform(-3, 3, 3)).astype(np.float32)  # >= 9 m from every face
    d = rng.normal(size=3)
    if rng.random() < 0.2:
        d[rng.integers(0, 3)] = 0.0  # axis-parallel planes: an infinite tmax on that axis
    if not np.any(d):
        d[0] = 1.0
    d = (d / np.linalg.norm(d)).astype(np.float32)
    vox = np.zeros((256, 3), dtype=np.int32)
    dd = np.zeros(256, dtype=np.float32)
    n = C.c_size_t(0)
    f(big.h, capi.ptr(start), capi.ptr(d), np.float32(length), capi.ptr(vox), capi.ptr(dd), 256, C.byref(n))
    k = n.value
    assert 0 < k < 256
    v, w = vox[:k].astype(np.int64), dd[:k].astype(np.float64)
    assert (w >= -1e-6).all()
    assert abs(w.sum() - np.float32(length)) < 1e-4
    first = np.floor((start.astype(np.float64) - off) / 0.5).astype(np.int64)
    np.testing.assert_array_equal(v[0], first)
    steps = np.diff(v, axis=0)
    assert (np.abs(steps).sum(axis=1) == 1).all()            # one axis at a time
    assert (steps * np.sign(d.astype(np.float64)) >= 0).all()  # never against the ray
    t1 = np.cumsum(w)
    mid = start.astype(np.float64) + d.astype(np.float64) * (t1 - 0.5 * w)[:, None]
    cell = (mid - off) / 0.5
    inside = (cell >= v - 1e-4) & (cell <= v + 1 + 1e-4)
    assert inside[w > 1e-4].all()
    big.close()


@settings(max_examples=40, deadline=None)
@given(seed=st.integers(0, 100_000), n=st.integers(1, 5000), leaf=st.sampled_from([0.1, 0.25, 0.5, 1.0]), aligned=st.booleans())
def test_weighted_grid_against_numpy_unique(oracle, seed, n, leaf, aligned):
    statements.weighted_grid_against_numpy_unique(oracle, seed, n, leaf, aligned)


@settings(max_examples=12, deadline=None)
@given(seed=st.integers(0, 100_000), p_bg=st.sampled_from([0.002, 0.01, 0.05]), max_dist=st.sampled_from([0.5, 1.0, 1.5, 1.7]))
def test_has_close_to_is_a_dilation_of_the_occupancy_image(oracle, seed, p_bg, max_dist):
    """hasCloseTo (voxel_map.cpp:376-400) at EVERY cell of a small map against scipy's binary dilation of the thresholded map by
    the stencil {o in [-d, d)^3 : floor(sqrt(|o|^2)) <= max_dist / vs} (half-open cube, truncated integer norm: SURVEY Q3 / Q4),
    cut at the map's faces - i.e. the answer depends on the cell only and is one bit of a dilated image, which is what k_dilate
    builds once per map state and the frame kernel reads (`mapclose`)."""
    from scipy import ndimage

    from vofod_amd.detector import VoFOD, default_params

    sp, dp = default_params(oracle)
    sp.voxel_size = 0.5
    sp.oparea_offset[:] = (3.0, 3.0, 0.0)
    sp.oparea_size[:] = (6.0, 6.0, 6.0)
    sp.sensor_hrays, sp.sensor_vrays = 8, 2
    det = VoFOD(oracle, sp, dp)
    sx, sy, sz = det.map_size
    rng = np.random.default_rng(seed)
    m = np.full((sz, sy, sx), -1000.0, dtype=np.float32)
    m[rng.random((sz, sy, sx)) < p_bg] = 0.0
    det.write_map(capi.MAP_VOXELS, m)
    thr = -300.0
    f = oracle.extra("vofod_oracle_map_has_close_to", C.c_int, [C.c_void_p] + [C.c_float] * 5)
    off = det.map_offset
    got = np.zeros((sz, sy, sx), dtype=bool)
    for k in range(sz):
        for j in range(sy):
            for i in range(sx):
                got[k, j, i] = bool(f(det.h, off[0] + (i + 0.5) * 0.5, off[1] + (j + 0.5) * 0.5, off[2] + (k + 0.5) * 0.5, max_dist, thr))
    mdi = np.float32(max_dist) * np.float32(2.0)  # max_dist * vs_inv
    d = int(np.ceil(mdi))
    # structuring element over offsets -d .. d (scipy wants odd sizes): the +d plane stays empty (half-open cube)
    o = np.arange(-d, d + 1)
    oz, oy, ox = np.meshgrid(o, o, o, indexing="ij")
    S = (np.floor(np.sqrt((ox * ox + oy * oy + oz * oz).astype(np.float64))).astype(np.float32) <= mdi) & (ox < d) & (oy < d) & (oz < d)
    # close(c) = OR over o in S of occ(c + o): a dilation by the REFLECTED stencil (scipy's convention is occ(c - o))
    want = ndimage.binary_dilation(m > thr, structure=S[::-1, ::-1, ::-1])
    np.testing.assert_array_equal(got, want)
    det.close()


def test_whole_scan_raycast_map_is_segment_voxel_geometry(oracle):
    statements.whole_scan_raycast_map_is_segment_voxel_geometry(oracle)


@pytest.mark.parametrize("new_rule", [1, 0])
def test_raycast_update_sweep_is_the_voxelwise_formula(oracle, new_rule):
    statements.raycast_update_sweep_is_the_voxelwise_formula(oracle, new_rule)


@pytest.mark.parametrize("sensor,vs", [("os1-16", 0.5), ("os1-128", 0.25)])
def test_map_update_of_a_scan_is_the_voxelwise_formula(oracle, sensor, vs):
    statements.map_update_of_a_scan_is_the_voxelwise_formula(oracle, sensor, vs)


@pytest.mark.parametrize("sensor,vs,seed", [("os1-16", 0.5, 300), ("os1-128", 0.25, 301)])
def test_filter_and_transform_of_a_scan_against_numpy_crops(oracle, sensor, vs, seed):
    statements.filter_and_transform_of_a_scan_against_numpy_crops(oracle, sensor, vs, seed)


def test_detection_records_against_the_formulas_in_numpy(oracle):
    statements.detection_records_against_the_formulas_in_numpy(oracle)


def test_classification_of_a_scan_against_scipy_fills_in_cluster_order(oracle):
    statements.classification_of_a_scan_against_scipy_fills_in_cluster_order(oracle)


@pytest.mark.parametrize("sensor,vs", [("os1-16", 0.5), ("os1-128", 0.25)])
def test_close_far_split_and_clusters_of_a_scan_against_scipy(oracle, sensor, vs):
    statements.close_far_split_and_clusters_of_a_scan_against_scipy(oracle, sensor, vs)


@pytest.mark.parametrize("seed,max_bg", [(1, 0.8), (2, 0.8), (3, 1.6), (4, 2.2), (5, 0.8)])
def test_sepclusters_role_against_numpy(oracle, seed, max_bg):
    statements.sepclusters_role_against_numpy(oracle, seed, max_bg)


# ---- the frame kernel's area x voxel-size limit (fill_ref_lattice, vofod_hip.hip) --------------------------------------------
@pytest.mark.parametrize("row", list(TABLE))
def test_geometry_table_mirrors_fill_ref_lattice(row):
    """fill_ref_lattice in host float32 arithmetic: dims, bricks, eps and exactly the stated failing conditions for every row -
    each "off" row lies just beyond ONE limit, its "on" neighbour just inside it"""
    off, size, vs, dims, bricks, eps, fails, _, _ = TABLE[row]
    cap = capacities()
    assert (cap["LB_BITWORDS"], cap["FR_ROWS_MAX"], cap["FR_MAX_NBZ"]) == (9984, 8192, 64)  # what the table was worked out for
    rl = ref_lattice(off, size, vs, cap)
    assert tuple(rl["dims"]) == dims
    assert rl["bricks"] == bricks
    assert abs(rl["eps"] - eps) < 5e-5, rl["eps"]
    assert tuple(k for k, ok in rl["conds"].items() if not ok) == fails
    assert rl["on"] == (not fails)
    n_vox = np.prod([math.ceil(float(np.float32(1) / np.float32(vs) * np.float32(s))) + 1 for s in size])
    assert n_vox <= (38.0e6 if row == "default_0.2" else 20.0e6)  # voxels of the map each detector allocates three times (host memory of the GPU cases)


def test_geometry_table_limits_are_tight():
    """the rows that name a limit sit at it: 99.5 % of the brick cap, nbx 509 / 521 around 512, nbz 63 / 67 around 64, rows 8 016 /
    9 018 around 8 192"""
    cap = capacities()
    rl = {k: ref_lattice(*TABLE[k][:3], cap) for k in TABLE}
    assert 0.99 < rl["default"]["bricks"] / (cap["LB_BITWORDS"] * 32) <= 1.0
    assert (rl["long_x_508"]["nb"][0], rl["long_x_520"]["nb"][0]) == (509, 521)
    assert (rl["tall_62"]["nb"][2], rl["tall_66"]["nb"][2]) == (63, 67)
    assert (rl["long_y_rows_8016"]["rows"], rl["long_y_rows_9018"]["rows"]) == (8016, 9018)
    assert rl["far_4000"]["eps"] < 0.05 < rl["far_5000"]["eps"]


def test_fallback_switch_list_is_the_matrix_script_s():
    """the route assertions of test_gpu_frame_inputs.py loosen under exactly the switches tools/run_fallback_matrix.sh runs"""
    import re

    text = (ROOT / "tools" / "run_fallback_matrix.sh").read_text()
    assert set(re.findall(r"VOFOD_[A-Z_]+(?==)", text)) == set(FALLBACK_SWITCHES)
