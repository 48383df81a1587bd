"""vofod_map_match and vofod_pose_lattice without a GPU: the declared surface, vofod_pose_lattice against its float64 statement, the
numpy statement of MAP MATCH (map_match_cases.py) by hand on the 5 x 4 x 3 hand map, the fixtures of the device tests - every class
occurs, shifts and tables matter - and the end-to-end scene, whose OCCUPIED count peaks at the centre of the lattice alone."""
import ctypes as C
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import map_match_cases as mm
import map_render_cases as mrc
from vofod_amd import capi

ROOT = Path(__file__).resolve().parent.parent
F = np.float32


@pytest.fixture(scope="module")
def hostlib():
    """the product library, for its handle-free entry points only: no device is touched"""
    so = ROOT / "vofod_amd" / "csrc" / "libvofod_hip.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    return capi.Library(so, "vofod_")


# ------------------------------------------------------------------------------------------------ surface
def test_declared_surface_and_mirror():
    from vofod_amd import detector

    text = capi.HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("map_match", "pose_lattice"):
        assert name in capi.declared_entry_points() and name in capi.PRODUCT_ONLY and name in capi._SIGS, name
    params = lambda name: [" ".join(p.split()) for p in re.search(rf"int vofod_{name}\((.*?)\);", code, flags=re.S).group(1).split(",")]
    assert params("map_match") == ["vofod_handle* h", "const vofod_scan* scan", "const float* tfs", "size_t n_poses", "float threshold", "uint32_t* counts", "int32_t* best"]
    assert params("pose_lattice") == ["const float tf[12]", "const float step[3]", "const int32_t n[3]", "float yaw_step", "int32_t n_yaw", "float* tfs_out"]
    assert capi._SIGS["map_match"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p])
    assert capi._SIGS["pose_lattice"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p])
    assert re.search(r"enum \{ VOFOD_MATCH_SKIPPED = 0, VOFOD_MATCH_OUTSIDE = 1, VOFOD_MATCH_FREE = 2, VOFOD_MATCH_OCCUPIED = 3 \};", code)
    assert (capi.MATCH_SKIPPED, capi.MATCH_OUTSIDE, capi.MATCH_FREE, capi.MATCH_OCCUPIED) == (0, 1, 2, 3) == (mm.SKIPPED, mm.OUTSIDE, mm.FREE, mm.OCCUPIED)
    assert callable(getattr(detector.VoFOD, "map_match")) and callable(detector.pose_lattice)
    for phrase in ("MAP MATCH", "k_match_bits", "k_match_points", "k_match_score", "no SENSOR_OUTSIDE_MAP rule", "smallest k with the largest"):
        assert phrase in text, phrase
    assert text.index("SCANS AGAINST THE MAP (product library only)") < text.index("MAP MATCH (product library only)") < text.index("WORLD STORE (product library only)")


def test_hip_library_exports_both(hostlib, oracle):
    for name in ("map_match", "pose_lattice"):
        assert hasattr(hostlib, name) and not hasattr(oracle, name), name
    # argument checks come before anything touches a device
    assert hostlib.map_match(None, None, None, 0, 0.0, None, None) == capi.ERR_INVALID_ARG


def test_python_wrapper_signatures():
    import inspect

    from vofod_amd import detector

    p = inspect.signature(detector.VoFOD.map_match).parameters
    assert list(p) == ["self", "scan", "tfs", "threshold", "allow"] and p["allow"].default == ()
    p = inspect.signature(detector.pose_lattice).parameters
    assert list(p) == ["lib", "tf", "step", "n", "yaw_step", "n_yaw"] and p["yaw_step"].default == 0.0 and p["n_yaw"].default == 1


# ------------------------------------------------------------------------------------------------ vofod_pose_lattice
TF = mrc.pose((1.25, -0.7, 2.1), yaw=0.4, pitch=-0.2, roll=0.1)


@pytest.mark.parametrize("n", [(1, 1, 1), (5, 4, 3), (2, 1, 7), (255, 257, 1)])
def test_lattice_without_yaw_is_the_statement_bit_for_bit(hostlib, n):
    from vofod_amd.detector import pose_lattice

    step = (0.25, 0.1, 0.3)
    got = pose_lattice(hostlib, TF, step, n)
    exp = mm.lattice(TF, step, n).astype(F)
    assert got.shape == (n[0] * n[1] * n[2], 3, 4)
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
    # x fastest: candidate 1 is one step along x from candidate 0 (where there is one)
    if n[0] > 1:
        assert got[1, 0, 3] > got[0, 0, 3] and got[1, 1, 3] == got[0, 1, 3]


def test_lattice_with_yaw_within_one_ulp_and_centre_is_tf(hostlib):
    from vofod_amd.detector import pose_lattice

    n, step = (3, 5, 1), (0.25, 0.25, 0.5)
    got = pose_lattice(hostlib, TF, step, n, 0.07, 5)
    exp = mm.lattice(TF, step, n, 0.07, 5).astype(F)
    assert got.shape == (75, 3, 4)
    np.testing.assert_array_max_ulp(got, exp, maxulp=1)
    np.testing.assert_array_equal(got[75 // 2], TF)  # (as values: the centre candidate of odd counts)
    # the yaw is the slowest index, a rotation about the vertical through the sensor's own origin: t does not turn
    np.testing.assert_array_equal(got[:15, :, 3], got[60:, :, 3])
    assert (got[:15, :2, :3] != got[60:, :2, :3]).any()
    np.testing.assert_array_equal(got[:, 2, :3], np.broadcast_to(TF[2, :3], (75, 3)))
    # psi = -2 * 0.07 for the first yaw: R_k = Rz(psi) R
    psi = -2 * float(F(0.07))
    Rz = np.array([[np.cos(psi), -np.sin(psi), 0], [np.sin(psi), np.cos(psi), 0], [0, 0, 1]])
    np.testing.assert_allclose(got[0, :, :3], Rz @ TF[:, :3].astype(np.float64), atol=1e-6)


def test_lattice_refusals_leave_the_output_untouched(hostlib):
    tf, step = np.ascontiguousarray(TF).reshape(12), np.array([0.1, 0.1, 0.1], F)

    def call(tf=tf, step=step, n=(2, 2, 2), yaw_step=0.0, n_yaw=1, null_out=False):
        out = np.full(8 * 12 + 12, 7.5, F)
        nn = None if n is None else np.array(n, np.int32)
        st = hostlib.pose_lattice(capi.ptr(tf), capi.ptr(step), capi.ptr(nn), yaw_step, n_yaw, None if null_out else capi.ptr(out))
        assert st == capi.OK or (out == 7.5).all()
        assert (out[8 * 12 :] == 7.5).all()
        return st

    INV = capi.ERR_INVALID_ARG
    assert call() == capi.OK
    assert call(tf=None) == INV and call(step=None) == INV and call(n=None) == INV and call(null_out=True) == INV
    assert call(n=(0, 2, 2)) == INV and call(n=(2, -1, 2)) == INV and call(n=(2, 2, 0)) == INV and call(n_yaw=0) == INV
    assert call(n=(256, 256, 1)) == INV and call(n=(65535, 1, 1), n_yaw=2) == INV and call(n=(2**31 - 1, 2**31 - 1, 2**31 - 1), n_yaw=2**31 - 1) == INV
    for bad in (np.nan, np.inf, -np.inf):
        assert call(step=np.array([0.1, bad, 0.1], F)) == INV
        assert call(yaw_step=bad, n_yaw=1) == INV


# ------------------------------------------------------------------------------------------------ the statement by hand
# the hand map: 5 x 4 x 3 voxels of 0.5 m, origin (-1, -0.75, 0).  Voxel (ix, iy, iz) spans x in [-1 + 0.5 ix, -0.5 + 0.5 ix),
# y in [-0.75 + 0.5 iy, ...), z in [0.5 iz, ...).
def _hand(points, cells, tfs, threshold=0.0, ranges=None, lo=(0, 0, 0), hi=(0, 0, 0)):
    g = mm.hand_geometry(points)
    rng = np.full(g.w, 1000, np.uint32) if ranges is None else np.asarray(ranges, np.uint32)
    assert F(1000) * F(0.001) == F(1.0)
    return mm.statement(g, mrc.hand_map(cells), SimpleNamespace(range=rng, col_tfs=None, xyz=None), np.asarray(tfs, F).reshape(-1, 3, 4), threshold, lo, hi)


def test_hand_every_class_and_the_compare():
    pts = [(-0.75, -0.5, 0.25),  # the centre of voxel (0, 0, 0)
           (0.25, 0.0, 0.75),    # the centre of voxel (2, 1, 1)
           (1.25, 1.0, 1.25),    # the centre of voxel (4, 3, 2)
           (1.5, 0.0, 0.25),     # x on the far face: f == size -> OUTSIDE
           (-1.0, -0.75, 0.0),   # the map's own corner: f == 0 -> inside, voxel (0, 0, 0)
           (0.25, 0.0, 0.75)]    # ... no return (range 0)
    cells = {(0, 0, 0): 1.0, (2, 1, 1): 0.5, (4, 3, 2): np.inf}
    r = _hand(pts, cells, [mrc.IDENT], threshold=0.5, ranges=[1000] * 5 + [0])
    assert r.classes[0].tolist() == [mm.OCCUPIED, mm.FREE, mm.OCCUPIED, mm.OUTSIDE, mm.OCCUPIED, mm.SKIPPED]  # (threshold-equal: FREE; +inf: OCCUPIED)
    assert r.counts.tolist() == [[1, 1, 1, 3]] and r.best == 0
    r = _hand(pts[:3], {(0, 0, 0): np.nan, (2, 1, 1): -0.0, (4, 3, 2): 0.0}, [mrc.IDENT], threshold=0.0)
    assert r.classes[0].tolist() == [mm.FREE] * 3  # (a NaN voxel, and voxels equal to the threshold of either sign of zero)


def test_hand_candidates():
    pts = [(-0.75, -0.5, 0.25), (0.25, 0.0, 0.75), (1.25, 1.0, 1.25)]
    cells = {(1, 0, 0): 1.0, (3, 1, 1): 1.0, (3, 0, 0): 1.0}
    shift_x = mrc.pose((0.5, 0.0, 0.0))  # one voxel along +x: (0,0,0) -> (1,0,0), (2,1,1) -> (3,1,1), (4,3,2) -> outside
    nan_tf = mrc.IDENT.copy()
    nan_tf[2, 0] = np.nan
    inf_tf = mrc.IDENT.copy()
    inf_tf[1, 3] = -np.inf
    # (x, y) -> (-y, x): (0.5, -0.75, 0.25) is voxel (3, 0, 0); (0, 0.25, 0.75) is voxel (2, 2, 1); (-1, 1.25, 1.25) has f[1] == 4 == size
    quarter = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]], F)
    r = _hand(pts, cells, [mrc.IDENT, shift_x, nan_tf, inf_tf, quarter, shift_x])
    assert r.classes[0].tolist() == [mm.FREE] * 3
    assert r.classes[1].tolist() == [mm.OCCUPIED, mm.OCCUPIED, mm.OUTSIDE]
    assert (r.classes[2] == mm.OUTSIDE).all() and (r.classes[3] == mm.OUTSIDE).all()  # a NaN or infinite w is OUTSIDE
    assert r.classes[4].tolist() == [mm.OCCUPIED, mm.FREE, mm.OUTSIDE]
    assert r.best == 1  # the smallest k with the largest count: 5 ties with 1
    assert (r.counts.sum(axis=1) == 3).all() and (r.counts[:, 0] == 0).all()


def test_hand_skipped_rules():
    pts = [(0.25, 0.0, 0.75), (0.3, 0.1, 0.8), (0.25, 0.0, 0.75), (np.nan, 0.0, 0.75), (0.25, np.inf, 0.75)]
    # a zero range; a point in the closed exclude box (on its face); a point outside it; a NaN and an infinite coordinate
    lo, hi = (0.3, 0.0, 0.0), (0.5, 0.1, 0.8)
    r = _hand(pts, {}, [mrc.IDENT, mrc.pose((9.0, 0.0, 0.0))], ranges=[0, 1000, 1000, 1000, 1000], lo=lo, hi=hi)
    assert r.skipped.tolist() == [True, True, False, True, True]
    assert r.counts.tolist() == [[4, 0, 1, 0], [4, 1, 0, 0]]  # SKIPPED does not depend on the candidate
    # a point scan: all three zero of either sign is "no return"; one zero coordinate is a point
    g = mm.hand_geometry(pts)
    xyz = np.array([(0.0, -0.0, 0.0), (0.0, 0.0, 0.25), (-0.0, -0.0, -0.0), (0.25, 0.0, 0.75), (np.nan, 0.0, 0.0)], F)
    r = mm.statement(g, mrc.hand_map({}), SimpleNamespace(xyz=xyz, range=None, col_tfs=None), mrc.IDENT[None], 0.0, (5.0, 5.0, 5.0), (6.0, 6.0, 6.0))
    assert r.skipped.tolist() == [True, False, True, False, True]


# ------------------------------------------------------------------------------------------------ the fixtures of the device tests
@pytest.mark.parametrize("name", ["16x8", "20x7", "24x11", "64x32"])
def test_device_fixtures_hold_every_class(hostlib, name):
    """what tests/test_gpu_map_match.py compares the device with: every class occurs for every sensor and input kind, the four slots
    sum to the pixel count, the candidates disagree, and the shifts and the table change the answer"""
    for kind in ("range", "motion", "points"):
        c = mm.shared_case(hostlib, name, kind, 300 if name != "64x32" else 65, exclude=mm.EXCLUDE)
        e = c.exp
        assert set(np.unique(e.classes).tolist()) == {0, 1, 2, 3}, (name, kind)
        assert (e.counts.sum(axis=1) == c.w * c.h).all() and (e.counts[:, 0] == e.counts[0, 0]).all()
        assert len({r.tobytes() for r in e.classes}) > len(e.counts) // 2 and len({tuple(r) for r in e.counts.tolist()}) >= 30  # (a kernel that mixed candidates up would show)
        assert (e.counts[5, 1:] == (c.w * c.h - e.counts[0, 0], 0, 0)).all() and (e.counts[6, 1:] == (c.w * c.h - e.counts[0, 0], 0, 0)).all()  # the NaN and the inf candidate
        for k in range(7, 13):  # pushed out through each of the six faces
            assert e.counts[k, mm.OUTSIDE] == c.w * c.h - e.counts[0, 0], k
        assert e.best == int(np.argmax(e.counts[:, 3])) and (e.counts[: e.best, 3] < e.counts[e.best, 3]).all()
        bare = mm.statement(c.g, c.m, c.scan, c.tfs, c.threshold, shift_by_row=c.shifts)
        assert bare.counts[0, 0] < e.counts[0, 0]  # the exclude box removes returns
    c = mm.shared_case(hostlib, name, "motion", 300 if name != "64x32" else 65, exclude=mm.EXCLUDE)
    unshifted = mm.statement(c.g, c.m, c.scan, c.tfs, c.threshold, c.lo, c.hi)
    rigid = mm.statement(c.g, c.m, SimpleNamespace(range=c.scan.range, col_tfs=None, xyz=None), c.tfs, c.threshold, c.lo, c.hi)
    assert (unshifted.counts != c.exp.counts).any() and (rigid.counts != c.exp.counts).any()


def test_exact_quarter_turns_are_exact(hostlib):
    c = mm.shared_case(hostlib, "16x8", "range", 300)
    assert set(np.unique(c.tfs[2:5, :, :3]).tolist()) <= {-1.0, 0.0, 1.0}
    assert np.isnan(c.tfs[5]).any() and np.isinf(c.tfs[6]).any()


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_scene_peaks_at_the_centre_alone():
    e = mm.e2e_case()
    n, n_yaw, _ = e.lattice
    assert len(e.tfs) == 5 * 5 * 3 * 3 and e.centre == 112
    np.testing.assert_array_equal(e.tfs[e.centre], e.P)
    occ = e.exp.counts[:, mm.OCCUPIED].astype(np.int64)
    n_returns = int((e.range != 0).sum())
    # a return lies in the voxel that was hit - but for one whose piece is shorter than the millimetre its range was rounded to
    assert n_returns > e.w * e.h // 3 and n_returns - n_returns // 100 <= occ[e.centre] <= n_returns
    assert e.exp.best == e.centre and (np.delete(occ, e.centre) < occ[e.centre]).all()
    # the map is asymmetric: the two neighbours along each axis score differently
    lat = occ.reshape(n_yaw, n[2], n[1], n[0])
    assert lat[1, 1, 2, 1] != lat[1, 1, 2, 3] and lat[1, 1, 1, 2] != lat[1, 1, 3, 2]
