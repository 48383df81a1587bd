"""vofod_map_render_scans without a GPU: the declared surface, the numpy statement (map_render_scans_cases.py) held to things that
are not itself - the rigid statement under an identity table, under exact quarter turns, the measurement column of the range
decode - the verdict by hand on the 5 x 4 x 3 hand map, and the fixtures of the device tests: every verdict occurs in them."""
import ctypes as C
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import map_render_cases as mrc
import map_render_scans_cases as sc
import range_motion_cases as rm
import raycast_motion_cases as rmc
from vofod_amd import capi

ROOT = Path(__file__).resolve().parent.parent
F = np.float32


@pytest.fixture(scope="module")
def hostlib():
    """the product library, for its handle-free entry points only (vofod_column_poses, vofod_ouster_lut): no device is touched"""
    so = ROOT / "vofod_amd" / "csrc" / "libvofod_hip.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    return capi.Library(so, "vofod_")


# ------------------------------------------------------------------------------------------------ surface
def test_declared_surface_and_mirror():
    from vofod_amd.detector import VoFOD

    text = capi.HEADER.read_text()
    assert "map_render_scans" in capi.declared_entry_points() and "map_render_scans" in capi.PRODUCT_ONLY and "map_render_scans" in capi._SIGS
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"int vofod_map_render_scans\((.*?)\);", code, flags=re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["vofod_handle* h", "const vofod_scan* scans", "const float* tfs", "size_t n_scans", "float threshold", "float max_distance", "float tolerance", "uint32_t* range",
                      "uint32_t* voxel", "uint8_t* what", "float* t_in_out", "uint8_t* verdict", "uint32_t* counts", "int32_t out_memspace"], params
    res, args = capi._SIGS["map_render_scans"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_float] + [C.c_void_p] * 6 + [C.c_int32]
    enum = re.search(r"enum \{ VOFOD_VERDICT_NONE = 0, VOFOD_VERDICT_AGREES = 1, VOFOD_VERDICT_EMPTY = 2, VOFOD_VERDICT_NEARER = 3,\s*VOFOD_VERDICT_THROUGH = 4, "
                     r"VOFOD_VERDICT_MISSING = 5, VOFOD_VERDICT_BEYOND = 6 \};", code)
    assert enum
    assert (capi.VERDICT_NONE, capi.VERDICT_AGREES, capi.VERDICT_EMPTY, capi.VERDICT_NEARER, capi.VERDICT_THROUGH, capi.VERDICT_MISSING, capi.VERDICT_BEYOND) == tuple(range(7))
    assert (sc.NONE, sc.AGREES, sc.EMPTY, sc.NEARER, sc.THROUGH, sc.MISSING, sc.BEYOND) == tuple(range(7))
    assert callable(getattr(VoFOD, "map_render_scans"))
    for phrase in ("SCANS AGAINST THE MAP", "k_map_render_scans", "never multiplied together", "ALWAYS host", "slot 7 is 0"):
        assert phrase in text, phrase
    assert text.index("MAP RENDER (product library only)") < text.index("SCANS AGAINST THE MAP (product library only)") < text.index("WORLD STORE (product library only)")


def test_hip_library_exports_map_render_scans(hostlib, oracle):
    assert hasattr(hostlib, "map_render_scans") and not hasattr(oracle, "map_render_scans")
    # argument checks come before anything touches a device
    assert hostlib.map_render_scans(None, None, None, 0, 0.0, 1.0, 0.0, None, None, None, None, None, None, capi.MEM_HOST) == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ the statement against what it is not
def _small(name="16x8", seed=2):
    w, h = sc.SENSORS[name][:2]
    dirs, offs = mrc.sim_lut(w, h), (np.random.default_rng(seed).uniform(-0.03, 0.03, (w * h, 3))).astype(F)
    g = sc.geometry(name, dirs, offs)
    m = mrc.random_map(g.size, seed + 1, sc.THRESHOLD, frac=0.08)
    return g, m, sc.view_poses(g, 3)


def test_geometry_is_the_handles(oracle):
    """the geometry the fixtures are built on is the one a handle of that sensor has"""
    for name, (w, h, area, vs, _) in sc.SENSORS.items():
        dirs = mrc.sim_lut(w, h)
        det = sc.make_det(oracle, w, h, area, vs, dirs, mask=sc.sensor_mask(w, h))
        try:
            g, want = sc.geometry(name, dirs, None), mrc.geom(det, dirs)
            assert g.size == want.size and g.vs == want.vs and (g.w, g.h) == (want.w, want.h)
            np.testing.assert_array_equal(g.off, want.off)
        finally:
            det.close()


def test_identity_table_is_the_rigid_statement():
    g, m, tfs = _small()
    exp = mrc.render(g, m, tfs, sc.THRESHOLD, 2.6)
    scans = [SimpleNamespace(col_tfs=sc.identity_table(g.w), range=None)] * 3
    got = sc.statement(g, m, scans, tfs, sc.THRESHOLD, 2.6, shift_by_row=sc.column_shifts(g.w, g.h))
    mrc.assert_same((got.range, got.voxel, got.what, got.tio), exp, "identity table")
    assert got.verdict is None and got.counts is None
    none = sc.statement(g, m, [SimpleNamespace(col_tfs=None, range=None)] * 3, tfs, sc.THRESHOLD, 2.6)
    mrc.assert_same((none.range, none.voxel, none.what, none.tio), exp, "no table")
    assert {int(x) for x in np.unique(exp.what)} >= {mrc.HIT, mrc.END}


@pytest.mark.parametrize("shifted", [False, True], ids=["no shifts", "column shifts"])
def test_quarter_turn_table_is_the_rigid_statement_under_the_composed_pose(shifted):
    """T d is an exact signed permutation and tf o T exact, so every pixel of the view is the rigid pixel under
    compose_quarter(tf, k) for the k of its measurement column - which is range_motion_cases.measurement_column's"""
    g, m, tfs = _small("20x7", seed=5)
    shifts = sc.column_shifts(g.w, g.h, 1) if shifted else None
    k_of_m, table = rmc.quarter_table(g.w, 3)
    length = 1.6
    got = sc.statement(g, m, [SimpleNamespace(col_tfs=table, range=None)] * 3, tfs, sc.THRESHOLD, length, shift_by_row=shifts)
    i = np.arange(g.w * g.h)
    col = rm.measurement_column(i // g.w, i % g.w, g.w, shifts)
    if shifted:
        assert (col != i % g.w).any() and min(shifts) < 0 and max(shifts) >= g.w
    differs, unturned = 0, mrc.render(g, m, tfs, sc.THRESHOLD, length)
    for k in range(4):
        rigid = mrc.render(g, m, np.stack([rmc.compose_quarter(tf, k) for tf in tfs]), sc.THRESHOLD, length)
        sel = k_of_m[col] == k
        assert sel.any()
        for name, a, b in (("what", got.what, rigid.what), ("voxel", got.voxel, rigid.voxel), ("range", got.range, rigid.range), ("tio", got.tio.view(np.uint32), rigid.tio.view(np.uint32))):
            a, b = a.reshape(3, g.w * g.h, -1), b.reshape(3, g.w * g.h, -1)
            np.testing.assert_array_equal(a[:, sel], b[:, sel], err_msg=f"{name}, k = {k}")
        if k:
            differs += int((got.voxel.reshape(3, -1)[:, sel] != unturned.voxel.reshape(3, -1)[:, sel]).sum())
    assert differs > 0  # (the table matters: the turned pixels are not the unturned ones)


# ------------------------------------------------------------------------------------------------ the verdict by hand
# the hand map (map_render_cases): +x from the centre of voxel (0, 1, 0), faces at t = 0.25, 0.75, 1.25, 1.75, 2.25; a hit in
# voxel (3, 1, 0) is the piece [1.25, 1.75].  END with max_distance 0.5: the piece [0.25, 0.5].  Every number is exact in float32
# but 0.001f * r: the cases say which side the rounded product falls on.
def _hand(direction, tf, cells, thr, length, ranges, mask, tol, offs=None):
    dirs = np.tile(np.asarray(direction, F).reshape(1, 3), (4, 1))
    g = SimpleNamespace(size=mrc.HAND_SIZE, off=np.asarray(mrc.HAND_OFF, F), vs=F(mrc.HAND_VS), dirs=dirs, offs=None if offs is None else np.tile(np.asarray(offs, F).reshape(1, 3), (4, 1)), h=2, w=2)
    s = SimpleNamespace(col_tfs=None, range=np.asarray(ranges, np.uint32))
    return sc.statement(g, mrc.hand_map(cells), [s], tf[None], thr, length, tol, mask)


def test_verdict_hand_cases_cover_every_class():
    X, tf, hit = (1.0, 0.0, 0.0), mrc.pose((-0.75, 0.0, 0.25)), {(3, 1, 0): 1.0}
    ones = np.ones(4, np.uint8)
    seen = set()
    # ---- HIT [1.25, 1.75], tol 0.25.  1000 mm: rm + tol == 1.25 == t_in exactly (1000 * 0.001f rounds to 1.0f): not NEARER.
    #      999 mm: NEARER.  2000 mm: rm == 2.0 == t_out + tol exactly: not THROUGH.  2001 mm: THROUGH.
    assert F(1000) * F(0.001) == F(1.0) and F(2000) * F(0.001) == F(2.0)
    r = _hand(X, tf, hit, 0.0, 10.0, [1000, 999, 2000, 2001], ones, 0.25)
    assert (r.what == mrc.HIT).all() and (r.tio[..., 0] == F(1.25)).all() and (r.tio[..., 1] == F(1.75)).all()
    assert r.verdict.reshape(-1).tolist() == [sc.AGREES, sc.NEARER, sc.AGREES, sc.THROUGH]
    assert r.counts.tolist() == [[0, 2, 0, 1, 1, 0, 0, 0]]
    seen |= set(r.verdict.reshape(-1).tolist())
    # ---- HIT without a return: MISSING where the mask lets the pixel through, NONE where it does not; a return there counts all the same
    r = _hand(X, tf, hit, 0.0, 10.0, [0, 0, 1500, 1500], np.array([1, 0, 1, 0], np.uint8), 0.0)
    assert r.verdict.reshape(-1).tolist() == [sc.MISSING, sc.NONE, sc.AGREES, sc.AGREES]
    assert r.counts.tolist() == [[1, 2, 0, 0, 0, 1, 0, 0]]
    seen |= set(r.verdict.reshape(-1).tolist())
    # ---- END [0.25, 0.5] (max_distance 0.5), tol 0.25.  125 mm: 0.125 + 0.25 < 0.5: NEARER.  250 mm: rm + tol == 0.5 == t_out
    #      exactly: not NEARER, BEYOND.  900 mm: BEYOND.  0: EMPTY.
    assert F(125) * F(0.001) == F(0.125) and F(250) * F(0.001) == F(0.25)
    r = _hand(X, tf, hit, 0.0, 0.5, [125, 250, 900, 0], ones, 0.25)
    assert (r.what == mrc.END).all() and (r.tio[..., 1] == F(0.5)).all()
    assert r.verdict.reshape(-1).tolist() == [sc.NEARER, sc.BEYOND, sc.BEYOND, sc.EMPTY]
    assert r.counts.tolist() == [[0, 0, 1, 1, 0, 0, 2, 0]]
    seen |= set(r.verdict.reshape(-1).tolist())
    # ---- LEFT at the +x face from the centre of (2, 1, 1): the piece [0.75, 1.25]; a masked-out pixel without a return is NONE
    r = _hand(X, mrc.pose((0.25, 0.0, 0.75)), {}, 0.0, 10.0, [1000, 1300, 0, 0], np.array([1, 1, 1, 0], np.uint8), 0.0)
    assert (r.what == mrc.LEFT).all()
    assert r.verdict.reshape(-1).tolist() == [sc.NEARER, sc.BEYOND, sc.EMPTY, sc.NONE]
    # ---- NOT_CAST (the beam's offset puts the start outside): NONE whatever was measured
    r = _hand(X, tf, hit, 0.0, 10.0, [0, 1, 1500, 4000], ones, 0.0, offs=(-1.0, 0.0, 0.0))
    assert (r.what == mrc.NOT_CAST).all() and (r.verdict == sc.NONE).all() and r.counts.tolist() == [[4, 0, 0, 0, 0, 0, 0, 0]]
    assert seen == set(range(7)), seen


@pytest.mark.parametrize("case", sc.hand_verdicts(), ids=lambda c: c[0])
def test_hand_verdicts_shared_with_the_device(case):
    name, tf, cells, length, tol, ranges, want = case
    for r in (125, 250, 1000, 2000):
        assert F(r) * F(0.001) == F(r / 1000.0)
    r = _hand((1.0, 0.0, 0.0), tf, cells, 0.0, length, ranges, np.ones(4, np.uint8), tol)
    assert r.verdict.reshape(-1).tolist() == want


def test_verdict_compares_are_float_compares():
    """a NaN on either side makes every compare false: AGREES on a HIT, BEYOND on an open ray; the tolerance is added in float32"""
    one = lambda what, t_in, t_out, r, tol=0.0: int(sc.verdict(np.uint8([what]), F([t_in]), F([t_out]), np.uint32([r]), np.uint8([1]), tol)[0])
    assert one(mrc.HIT, np.nan, np.nan, 1000) == sc.AGREES and one(mrc.END, 0.0, np.nan, 1000) == sc.BEYOND
    # 16777217 mm is not a float: (float) r rounds to 16777216 before the product
    assert one(mrc.HIT, 0.0, float(F(16777216) * F(0.001)), 16777217) == sc.AGREES
    # rm + tol is rounded once: 1.0f + 2^-25 == 1.0f, so a t_in of the next float above 1 is still in front
    assert one(mrc.HIT, float(np.nextafter(F(1.0), F(2.0))), 2.0, 1000, tol=2.0 ** -25) == sc.NEARER


# ------------------------------------------------------------------------------------------------ the fixtures of the device tests
@pytest.mark.parametrize("name", list(sc.SENSORS))
def test_device_fixtures_hold_every_verdict(hostlib, name):
    """what tests/test_gpu_map_render_scans.py compares the device with: every one of the seven classes occurs in the statement's
    answer for every sensor (otherwise a device test could pass while leaving a class out), the counts are the bincount, and the
    shifts and tables do matter"""
    c = sc.shared_case(hostlib, name, 3)
    e = c.exp
    assert set(np.unique(e.verdict).tolist()) == set(range(7)), np.unique(e.verdict)
    assert {int(x) for x in np.unique(e.what)} >= {mrc.HIT, mrc.END}
    for v in range(3):
        np.testing.assert_array_equal(e.counts[v], np.bincount(e.verdict[v].reshape(-1), minlength=8))
    assert (e.counts.sum(axis=1) == c.w * c.h).all() and (e.counts[:, 7] == 0).all()
    assert [k for k, _ in c.tabs] == ["rigid", "quarter", "small"]
    assert (c.mask == 0).any() and ((c.ranges == 0) & (c.mask == 0)[None]).any()
    # the column shifts and the tables change the answer
    bare = [SimpleNamespace(col_tfs=t, range=None) for _, t in c.tabs]
    unshifted = sc.statement(c.g, c.m, bare, c.tfs, c.threshold, c.length, mask=c.mask)
    np.testing.assert_array_equal(unshifted.voxel[0], e.voxel[0])  # (a rigid view reads no shift)
    assert (unshifted.voxel[1] != e.voxel[1]).any() and (unshifted.tio[2].view(np.uint32) != e.tio[2].view(np.uint32)).any()
    rigid = mrc.render(c.g, c.m, c.tfs, c.threshold, c.length)
    np.testing.assert_array_equal(rigid.voxel[0], e.voxel[0])
    assert (rigid.voxel[1] != e.voxel[1]).any() and (rigid.tio[2].view(np.uint32) != e.tio[2].view(np.uint32)).any()
    # a view that used view 0's table would differ
    swapped = sc.statement(c.g, c.m, [bare[0]] * 3, c.tfs, c.threshold, c.length, mask=c.mask, shift_by_row=c.shifts)
    assert (swapped.voxel[1] != e.voxel[1]).any() and (swapped.tio[2].view(np.uint32) != e.tio[2].view(np.uint32)).any()


def test_the_tail_blocks_fixture_has_a_tail(hostlib):
    """24 x 11 = 264 rays: a second block of 8 live lanes and 248 dead ones - were those counted as NONE, slot 0 would be 248 too large"""
    c = sc.shared_case(hostlib, "24x11", 3)
    assert c.w * c.h == 264 and 264 - 256 == 8
    assert (c.exp.counts[:, 0] < 248).all()


def test_end_to_end_fixtures_say_what_the_device_test_will_ask():
    """a box the map does not know is NEARER exactly on the pixels that hit it; a box missing from the wall the map knows is THROUGH
    or BEYOND there; everything else agrees (AGREES on the wall, EMPTY where neither the scan nor the map has anything)"""
    a = sc.e2e_case("added")
    v = a.exp.verdict[0]
    assert a.on_box.sum() >= 4 and ((v == sc.NEARER) == a.on_box).all()
    assert set(np.unique(v[~a.on_box]).tolist()) == {sc.AGREES, sc.EMPTY}
    e = sc.e2e_case("erased")
    v = e.exp.verdict[0]
    assert e.on_box.sum() >= 4 and np.isin(v[e.on_box], (sc.THROUGH, sc.BEYOND)).all() and (v[e.on_box] == sc.THROUGH).any()
    assert set(np.unique(v[~e.on_box]).tolist()) == {sc.AGREES, sc.EMPTY}
    for c in (a, e):
        np.testing.assert_array_equal(c.exp.counts[0], np.bincount(c.exp.verdict[0].reshape(-1), minlength=8))


def test_python_wrapper_signature():
    import inspect

    from vofod_amd.detector import VoFOD

    p = inspect.signature(VoFOD.map_render_scans).parameters
    assert list(p) == ["self", "scans", "tfs", "threshold", "max_distance", "tolerance", "out", "allow"]
    assert p["tolerance"].default == 0.0 and p["out"].default is None and p["allow"].default == ()
