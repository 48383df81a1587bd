"""Motion-compensated point scans (include/vofod.h, MOTION COMPENSATION OF POINT SCANS) - what needs no GPU: (a) the declared surface,
its Python mirror and the exports of the cross-compiled product library; (b) the numpy statement of the definition
(tests/point_motion_cases.py) on the rigid decode of a range image against the statement of the compensated range image
(tests/range_motion_cases.py), bit for bit; (c) the statement by hand."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from vofod_amd import capi
from vofod_amd.detector import ScanData, default_params

import point_motion_cases as pm
import range_motion_cases as rm
from test_range_image_cpu import decode_definition, offset_lut, sample_ranges, sim_directions

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ (a) surface
def test_header_mirror_exports_and_scan_size():
    names = capi.declared_entry_points()
    assert set(names) == set(capi._SIGS)
    for n in ("set_point_motion", "deskew_points"):
        assert n in names and n in capi.PRODUCT_ONLY
    assert capi._SIGS["set_point_motion"] == (C.c_int, [C.c_void_p, C.c_int])
    res, args = capi._SIGS["deskew_points"]
    assert res is C.c_int and len(args) == 6  # (handle, scan, x, y, z, out_memspace)
    text = capi.HEADER.read_text()
    assert "int vofod_set_point_motion(vofod_handle* h, int on);" in text
    assert "int vofod_deskew_points(vofod_handle* h, const vofod_scan* scan, float* x, float* y, float* z, int32_t out_memspace);" in text
    assert "MOTION COMPENSATION OF POINT SCANS" in text
    assert C.sizeof(capi.Scan) == 80 and capi.Scan.col_tfs.offset == 72  # vofod_scan does not change
    so = ROOT / "vofod_amd" / "csrc" / "libvofod_hip.so"
    if not so.exists():  # hipcc cross-compiles gfx950 without a GPU
        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    lib = capi.Library(so, "vofod_")
    for n in ("set_point_motion", "deskew_points"):
        assert hasattr(lib, n) and getattr(lib, n).argtypes == capi._SIGS[n][1]
    # NULL handles need no device
    assert lib.set_point_motion(None, 1) == capi.ERR_INVALID_ARG
    out = np.zeros(3, dtype=f32)
    assert lib.deskew_points(None, None, capi.ptr(out), capi.ptr(out), capi.ptr(out), capi.MEM_HOST) == capi.ERR_INVALID_ARG


def test_oracle_does_not_export_them(oracle):
    assert not hasattr(oracle, "set_point_motion") and not hasattr(oracle, "deskew_points")


def test_a_point_scan_carries_the_pose_table():
    x = np.zeros(16 * 1024, dtype=f32)
    T = rm.identity_poses(1024)
    c = ScanData(x=x, y=x, z=x, width=1024, height=16, stride_bytes=48, col_tfs=T).as_c()
    assert c.col_tfs == T.ctypes.data and c.x == x.ctypes.data and c.stride_bytes == 48


# ------------------------------------------------------------------------------------------------ (b) against the range statement
def lut_of(shape_name, kind):
    shape = pm.SHAPES[shape_name]
    return (sim_directions(shape), None) if kind == "simulated" else offset_lut(shape)


@pytest.mark.parametrize("lut_kind", ["simulated", "offsets"])
@pytest.mark.parametrize("shape_name", list(pm.SHAPES))
def test_statement_on_the_rigid_decode_is_the_compensated_range_image(oracle, shape_name, lut_kind):
    """points = the rigid decode of a range image: the point statement equals motion_definition of that image bit for bit, NaN mask
    included - every shape, the three kinds of table, the three kinds of shift"""
    h_, w_ = pm.SHAPES[shape_name][:2]
    n = h_ * w_
    lut = lut_of(shape_name, lut_kind)
    lo, hi = rm.exclude_bounds(default_params(oracle)[0])
    rng = rm.near_ranges(sample_ranges(n, seed=n) if n >= 64 else np.random.default_rng(n).integers(0, 60_000, n).astype(np.uint32), share=0.25, seed=n)
    rng[:: max(n // 9, 1)] = 0
    x, y, z = decode_definition(rng, *lut)
    for pose_kind, make in pm.POSES.items():
        T = make(w_, seed=n)
        for shift_kind in pm.SHIFTS:
            shift = rm.shifts(shift_kind, h_, w_, seed=n)
            want = rm.motion_definition(rng, lut[0], lut[1], T, w_, lo, hi, shift)
            got = pm.point_definition(x, y, z, T, w_, lo, hi, shift)
            for a in range(3):
                np.testing.assert_array_equal(bits(got[a]), bits(want[a]), err_msg=f"{shape_name}/{lut_kind}/{pose_kind}/{shift_kind}: axis {a}")
            np.testing.assert_array_equal(got[3], want[3])
            assert want[3].any() and (rng == 0).any()


# ------------------------------------------------------------------------------------------------ (c) by hand
@pytest.fixture(scope="module")
def box(oracle):
    return rm.exclude_bounds(default_params(oracle)[0])


def one_row(points, T, lo, hi, shift=None):
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    w = p.shape[0]
    tab = np.broadcast_to(np.asarray(T, dtype=f32), (w, 3, 4)) if np.ndim(T) == 2 else T
    return pm.point_definition(p[:, 0], p[:, 1], p[:, 2], np.ascontiguousarray(tab), w, lo, hi, shift)


def test_zeros_of_either_sign_give_plus_zeros_and_no_pose(box):
    lo, hi = box
    T = rm.general_poses(1)[0]  # a translation that would move the origin
    assert np.abs(T[:, 3]).min() > 0
    zeros = [[0.0, 0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, -0.0, 0.0], [0.0, 0.0, -0.0], [-0.0, -0.0, -0.0]]
    x, y, z, nan = one_row(zeros, T, lo, hi)
    for v in (x, y, z):
        assert (bits(v) == 0).all()  # +0: the sign bit is clear
    assert not nan.any()  # (the origin lies inside the default box: the zero rule comes first)
    assert (lo <= 0).all() and (hi >= 0).all()


def test_non_finite_coordinates_give_qnan(box):
    lo, hi = box
    pts = [[np.nan, 5.0, 1.0], [5.0, np.nan, 1.0], [5.0, 1.0, np.nan], [np.inf, 5.0, 1.0], [5.0, -np.inf, 1.0], [5.0, 1.0, np.inf], [0.0, np.nan, 0.0], [0.0, 0.0, np.inf]]
    for T in (rm.general_poses(1)[0], np.eye(3, 4, dtype=f32)):
        x, y, z, nan = one_row(pts, T, lo, hi)
        assert nan.all()
        for v in (x, y, z):
            assert (bits(v) == 0x7FC00000).all()


def test_faces_of_the_box_are_inside_one_float_outward_is_not(box):
    lo, hi = box
    pts, inside = pm.face_points(lo, hi)
    assert inside.sum() == 12 and (~inside).sum() == 12
    x, y, z, nan = one_row(pts, np.eye(3, 4, dtype=f32), lo, hi)
    np.testing.assert_array_equal(nan, inside)
    for a, v in enumerate((x, y, z)):
        assert (bits(v[inside]) == 0x7FC00000).all()
        np.testing.assert_array_equal(v[~inside], pts[~inside, a])  # identity: the point itself


def test_identity_table_returns_equal_values(box):
    lo, hi = box
    shape = pm.SHAPES["3x100"]
    h_, w_ = shape[:2]
    x, y, z, special_at, face_at, _ = pm.sample_points(shape, lo, hi, seed=1)
    for shift_kind in pm.SHIFTS:
        gx, gy, gz, nan = pm.point_definition(x, y, z, rm.identity_poses(w_), w_, lo, hi, rm.shifts(shift_kind, h_, w_))
        for got, q in zip((gx, gy, gz), (x, y, z)):
            np.testing.assert_array_equal(got[~nan], q[~nan])  # as values: 1 * q + (0 * q + (0 * q + 0)) == q, -0 == +0
            assert (bits(got[nan]) == 0x7FC00000).all()
    assert 0 < nan.sum() < x.size


def test_the_pose_is_that_of_the_measurement_column(box):
    """a table whose entry m translates by (m, 0, 0): the x of every point tells which entry it took"""
    lo, hi = box
    h_, w_ = 3, 7
    T = rm.identity_poses(w_)
    T[:, 0, 3] = np.arange(w_, dtype=f32)
    q = np.full(h_ * w_, 50.0, dtype=f32)
    shift = np.array([0, 3, -2], dtype=np.int32)
    x, _, _, _ = pm.point_definition(q, q, q, T, w_, lo, hi, shift)
    want = [(c + int(shift[r])) % w_ for r in range(h_) for c in range(w_)]
    np.testing.assert_array_equal(x - f32(50.0), np.array(want, dtype=f32))
