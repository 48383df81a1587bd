"""vofod_map_distance and vofod_map_match_field without a GPU: the declared surface, the numpy statement of MAP DISTANCE
(map_distance_cases.py) against scipy's exact Euclidean transform on every map, content and radius of the device tests and by hand
on the 5 x 4 x 3 hand map, the field match's transform against map_match_cases', and the end-to-end scene, whose cost - unlike
the count of vofod_map_match - falls all the way to the centre of the lattice."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import map_distance_cases as md
import map_match_cases as mm
import map_render_cases as mrc
from vofod_amd import capi

ROOT = Path(__file__).resolve().parent.parent
F = np.float32


@pytest.fixture(scope="module")
def hostlib():
    """the product library, for its argument checks only: no device is touched"""
    so = ROOT / "vofod_amd" / "csrc" / "libvofod_hip.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    return capi.Library(so, "vofod_")


# ------------------------------------------------------------------------------------------------ surface
def test_declared_surface_and_mirror():
    from vofod_amd import detector

    text = capi.HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("map_distance", "map_match_field"):
        assert name in capi.declared_entry_points() and name in capi.PRODUCT_ONLY and name in capi._SIGS, name
    params = lambda name: [" ".join(p.split()) for p in re.search(rf"int vofod_{name}\((.*?)\);", code, flags=re.S).group(1).split(",")]
    assert params("map_distance") == ["vofod_handle* h", "float threshold", "int32_t radius", "uint16_t* d2", "size_t n", "int32_t memspace"]
    assert params("map_match_field") == ["vofod_handle* h", "const vofod_scan* scan", "const float* tfs", "size_t n_poses", "const uint16_t* d2", "size_t n", "int32_t field_memspace",
                                         "uint32_t near2", "uint32_t outside_cost", "uint32_t* counts", "uint64_t* cost", "int32_t* best"]
    assert capi._SIGS["map_distance"] == (C.c_int, [C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32])
    assert capi._SIGS["map_match_field"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
    assert re.search(r"enum \{ VOFOD_DIST_MAX_RADIUS = 255 \};", code)
    assert re.search(r"enum \{ VOFOD_FIELD_SKIPPED = 0, VOFOD_FIELD_OUTSIDE = 1, VOFOD_FIELD_FAR = 2, VOFOD_FIELD_NEAR = 3 \};", code)
    assert (capi.FIELD_SKIPPED, capi.FIELD_OUTSIDE, capi.FIELD_FAR, capi.FIELD_NEAR) == (0, 1, 2, 3) == (md.SKIPPED, md.OUTSIDE, md.FAR, md.NEAR)
    assert capi.DIST_MAX_RADIUS == 255 == md.MAX_RADIUS
    for phrase in ("MAP DISTANCE", "k_dist_x", "k_dist_y", "k_dist_z", "k_match_field", "smallest k with the smallest cost", "word for word"):
        assert phrase in text, phrase
    assert text.index("MAP MATCH (product library only)") < text.index("MAP DISTANCE (product library only)") < text.index("WORLD STORE (product library only)")
    p = inspect.signature(detector.VoFOD.map_distance).parameters
    assert list(p) == ["self", "threshold", "radius", "device", "allow"] and p["device"].default is False
    p = inspect.signature(detector.VoFOD.map_match_field).parameters
    assert list(p) == ["self", "scan", "tfs", "d2", "near2", "outside_cost", "allow"]


def test_hip_library_exports_both(hostlib, oracle):
    for name in ("map_distance", "map_match_field"):
        assert hasattr(hostlib, name) and not hasattr(oracle, name), name
    # argument checks come before anything touches a device
    assert hostlib.map_distance(None, 0.0, 1, None, 0, capi.MEM_HOST) == capi.ERR_INVALID_ARG
    assert hostlib.map_match_field(None, None, None, 0, None, 0, capi.MEM_HOST, 0, 0, None, None, None) == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ the statement against scipy
@pytest.mark.parametrize("name", list(md.MAPS))
def test_statement_is_scipys_transform_on_every_map_content_and_radius(name):
    for kind in md.CONTENTS:
        m, full = md.shared_full(name, kind)
        occ = md.occupied(m, md.THRESHOLD)
        assert occ.any() == (kind != "empty") and occ.all() == (kind == "solid"), kind
        for R in md.RADII:
            d2 = md.clamp(full, R)
            assert d2.dtype == np.uint16 and d2.shape == m.shape
            np.testing.assert_array_equal(d2, md.distance_edt(m, md.THRESHOLD, R), err_msg=f"{name} {kind} R {R}")
            assert (d2[occ] == 0).all() and (d2[~occ] > 0).all() and d2.max() <= R * R
    # the random maps hold what they are said to hold
    for kind, lo, hi in (("random0.2", 0.0, 0.03), ("random5", 0.02, 0.1), ("random50", 0.4, 0.6)):
        m, _ = md.shared_full(name, kind)
        assert lo < md.occupied(m, md.THRESHOLD).mean() < hi, (name, kind)
        assert np.isnan(m).any() and np.isposinf(m).any() and (m == F(md.THRESHOLD)).any()


def test_corner_maps_reach_across_the_longest_axes():
    """one occupied voxel in a corner: the opposite end of an axis longer than 255 is beyond every radius, and a radius that is
    larger than every axis of a small map reaches all of it"""
    m, full = md.shared_full("300x5x3", "corner0")
    d2 = md.clamp(full, 255)
    assert d2[0, 0, 0] == 0 and d2[0, 0, 255] == 255 * 255 and d2[0, 0, 254] == 254 * 254 and d2[0, 0, 299] == 255 * 255 and full[0, 0, 299] == 299 * 299
    m, full = md.shared_full("9x9x9", "corner7")
    assert md.clamp(full, 255)[0, 0, 0] == 3 * 64 and (md.clamp(full, 255) == full).all()


# ------------------------------------------------------------------------------------------------ the statement by hand
def test_hand_neighbours_radius_and_the_compare():
    # the 5 x 4 x 3 hand map [z, y, x], one occupied voxel at (x, y, z) = (1, 1, 1)
    m = mrc.hand_map({(1, 1, 1): 1.0})
    d = md.distance(m, 0.0, 2)
    assert d[1, 1, 1] == 0                                       # an occupied voxel
    assert d[1, 1, 2] == 1 and d[1, 0, 1] == 1 and d[2, 1, 1] == 1  # face neighbours
    assert d[1, 2, 2] == 2 and d[0, 1, 0] == 2                   # edge neighbours
    assert d[0, 0, 0] == 3 and d[2, 2, 2] == 3                   # corner neighbours
    assert d[1, 1, 3] == 4                                       # exactly at the radius: d2 == R * R
    assert d[1, 1, 4] == 4 and d[1, 3, 3] == 4                   # beyond it (9 and 8): R * R
    assert md.distance(m, 0.0, 3)[1, 1, 4] == 9 and md.distance(m, 0.0, 3)[1, 3, 3] == 8
    assert md.distance(m, 0.0, 1).max() == 1 and (md.distance(m, 0.0, 1) == 0).sum() == 1
    # nothing occupied: R * R everywhere
    assert (md.distance(mrc.hand_map({}), 0.0, 7) == 49).all()
    # NaN and threshold-equal voxels (of either sign of zero) are free, +inf is occupied
    m = mrc.hand_map({(0, 0, 0): np.nan, (2, 0, 0): 0.0, (3, 0, 0): -0.0, (4, 3, 2): np.inf})
    d = md.distance(m, 0.0, 255)
    assert (d == 0).sum() == 1 and d[2, 3, 4] == 0 and d[0, 0, 0] == 16 + 9 + 4
    # an infinite threshold: nothing is above +inf, everything that is not NaN is above -inf
    assert (md.distance(m, np.inf, 5) == 25).all()
    d = md.distance(m, -np.inf, 5)
    assert d[0, 0, 0] == 1 and (d == 0).sum() == 59
    # nothing wraps: the far end of a row is not next to the start of the next one
    m = mrc.hand_map({(4, 0, 0): 1.0})
    assert md.distance(m, 0.0, 255)[0, 1, 0] == 16 + 1


# ------------------------------------------------------------------------------------------------ the field match
def test_transform_is_map_match_cases_own(hostlib):
    """voxel_of against map_match_cases.classes: with the field as a float map and near2 as the threshold, FAR is its OCCUPIED and
    NEAR its FREE, candidate by candidate - NaN and infinite candidates and the six faces included"""
    c = mm.shared_case(hostlib, "24x11", "motion", 300, exclude=mm.EXCLUDE)
    field = md.random_field(int(np.prod(c.g.size)), 5)
    near2 = 30000
    exp = md.field_statement(c.g, field, c.scan, c.tfs, near2, 7, c.lo, c.hi, c.shifts)
    p, zero = mm.scan_points(c.g, c.scan, c.lo, c.hi, c.shifts)
    skip = mm.skipped(p, zero, c.lo, c.hi)
    as_map = field.astype(F).reshape(c.g.size[::-1])
    for k, tf in enumerate(c.tfs):
        cls = np.bincount(mm.classes(c.g, as_map, p, skip, tf, float(near2)), minlength=4)
        assert exp.counts[k].tolist() == [cls[mm.SKIPPED], cls[mm.OUTSIDE], cls[mm.OCCUPIED], cls[mm.FREE]], k
    assert (exp.counts.sum(axis=1) == c.w * c.h).all() and set(np.flatnonzero(exp.counts.any(axis=0)).tolist()) == {0, 1, 2, 3}
    assert exp.best == int(np.argmin(exp.cost)) and (exp.cost[: exp.best] > exp.cost[exp.best]).all()
    # the cost by hand for one candidate: nothing inside under the NaN candidate, so it is outside_cost per live pixel
    assert exp.cost[5] == 7 * exp.counts[5, md.OUTSIDE] and exp.counts[5, md.NEAR] == exp.counts[5, md.FAR] == 0


def test_near2_zero_with_the_calls_own_field_is_map_match(hostlib):
    c = mm.shared_case(hostlib, "20x7", "range", 300, exclude=mm.EXCLUDE)
    d2 = md.distance(c.m, c.threshold, 8)
    exp = md.field_statement(c.g, d2, c.scan, c.tfs, 0, 0, c.lo, c.hi)
    np.testing.assert_array_equal(exp.counts[:, md.NEAR], c.exp.counts[:, mm.OCCUPIED])
    np.testing.assert_array_equal(exp.counts[:, md.FAR], c.exp.counts[:, mm.FREE])
    np.testing.assert_array_equal(exp.counts[:, :2], c.exp.counts[:, :2])


def test_hand_field_cost_and_classes():
    pts = [(-0.75, -0.5, 0.25), (0.25, 0.0, 0.75), (1.25, 1.0, 1.25), (1.5, 0.0, 0.25), (0.25, 0.0, 0.75)]  # voxels (0,0,0), (2,1,1), (4,3,2); outside; no return
    g = mm.hand_geometry(pts)
    d2 = np.zeros((3, 4, 5), np.uint16)
    d2[0, 0, 0], d2[1, 1, 2], d2[2, 3, 4], d2[0, 0, 1], d2[1, 1, 3] = 5, 9, 65535, 100, 200
    scan = SimpleNamespace(range=np.array([1000, 1000, 1000, 1000, 0], np.uint32), col_tfs=None, xyz=None)
    r = md.field_statement(g, d2, scan, [mrc.IDENT, mrc.pose((0.5, 0.0, 0.0))], 9, 1000)
    assert r.counts.tolist() == [[1, 1, 1, 2], [1, 2, 2, 0]]  # one voxel along +x: (1,0,0) and (3,1,1) are FAR, the third leaves the map
    assert r.cost.tolist() == [5 + 9 + 65535 + 1000, 100 + 200 + 2000] and r.best == 1 and r.cost.dtype == np.uint64
    assert md.field_statement(g, d2, scan, [mrc.IDENT], 8, 0).counts.tolist() == [[1, 1, 2, 1]]  # d2 == near2 + 1 is FAR, d2 <= near2 is NEAR


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_cost_has_a_slope_the_count_lacks():
    c = md.e2e_field_case()
    e = c.e
    n, n_yaw, _ = e.lattice
    assert n[:2] == (5, 5) and e.centre == 112
    cost = c.exp.cost.astype(np.int64)
    assert c.exp.best == e.centre and (np.delete(cost, e.centre) > cost[e.centre]).all()  # the unique minimum
    lat = cost.reshape(n_yaw, n[2], n[1], n[0])
    x, y = lat[1, 1, 2, :], lat[1, 1, :, 2]  # the lines through the centre along x and along y
    assert x[2] == y[2] == cost[e.centre]
    # strictly lower one voxel from the centre than two voxels from it, either way, along x and along y
    assert x[1] < x[0] and x[3] < x[4] and y[1] < y[0] and y[3] < y[4], (x, y)
    assert x[2] < x[1] and x[2] < x[3] and y[2] < y[1] and y[2] < y[3]
    assert (c.exp.counts.sum(axis=1) == e.w * e.h).all()
