"""Exact raycast accumulation without a GPU (include/vofod.h, EXACT RAYCAST ACCUMULATION): the declared surface and its Python mirror,
the scale rule against the values the header lists, and the yardstick tests/test_gpu_raycast_exact.py holds k_raycast_exact to - the
oracle, one ray at a time (tests/raycast_exact_cases.py) - held to the oracle's own full float pass."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from vofod_amd import capi

import raycast_exact_cases as rx
import raycast_motion_cases as rc
from test_range_image_cpu import offset_lut

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


@pytest.fixture(scope="module")
def product():
    """the product library: it only has to load (hipcc cross-compiles gfx950 without a GPU)"""
    so = ROOT / "vofod_amd" / "csrc" / "libvofod_hip.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    return capi.Library(so, "vofod_")


# ------------------------------------------------------------------------------------------------ surface
def test_header_declares_and_library_exports_the_two_entry_points(product):
    names = capi.declared_entry_points()
    assert set(names) == set(capi._SIGS)
    text = capi.HEADER.read_text()
    assert "EXACT RAYCAST ACCUMULATION" in text
    assert "int vofod_set_raycast_exact(vofod_handle* h, int on);" in text
    assert "int vofod_raycast_units(vofod_handle* h, uint32_t* units, size_t n, int32_t* log2_units_per_m);" in text
    for n in ("set_raycast_exact", "raycast_units"):
        assert n in names and n in capi.PRODUCT_ONLY
        assert hasattr(product, n) and getattr(product, n).argtypes == capi._SIGS[n][1]
    assert capi._SIGS["set_raycast_exact"] == (C.c_int, [C.c_void_p, C.c_int])
    res, args = capi._SIGS["raycast_units"]
    assert res is C.c_int and len(args) == 4 and args[2] is C.c_size_t
    # NULL handles are refused before anything is touched (no device here)
    assert product.set_raycast_exact(None, 1) == capi.ERR_INVALID_ARG
    s = C.c_int32(0)
    assert product.raycast_units(None, None, 0, C.byref(s)) == capi.ERR_INVALID_ARG


def test_oracle_has_neither(oracle):
    assert not hasattr(oracle, "set_raycast_exact") and not hasattr(oracle, "raycast_units")


# ------------------------------------------------------------------------------------------------ the scale
def test_scale_rule_gives_the_listed_values():
    for (rows, cols, vs), want in rx.S_TABLE.items():
        s, qmax = rx.scale_rule(rows * cols, vs)
        assert s == want, (rows, cols, vs, s)
        n = rows * cols
        assert n * (qmax + 1) <= 2 ** 32 - 1 and qmax == int(np.floor(2.0 * float(f32(vs)) * 2.0 ** s))
        if s < 24:  # the largest: one more bit does not fit
            assert n * (int(np.floor(2.0 * float(f32(vs)) * 2.0 ** (s + 1))) + 1) > 2 ** 32 - 1
    # 64 lanes of QMAX fit in 32 bits (the wave's segmented sum), and so does a voxel every ray crosses
    for (rows, cols, vs) in rx.S_TABLE:
        s, qmax = rx.scale_rule(rows * cols, vs)
        assert 64 * qmax < 2 ** 32 and rows * cols * qmax < 2 ** 32
    # an in-voxel piece, sqrt(3) * vs, stays below QMAX * 2^-S ~ 2 * vs: the clamp does not bite on a rotation
    s, qmax = rx.scale_rule(100, 0.5)
    assert (s, qmax) == (24, 2 ** 24) and np.sqrt(3.0) * 0.5 < qmax * 2.0 ** -s


def test_units_round_to_nearest_even_and_clamp():
    s, qmax = 3, 20
    p = np.array([0.0, 0.0624, 0.0625, 0.0626, 0.1875, 0.3125, 1.0, 2.5, 2.56, 100.0], dtype=f32)
    # * 8:           0    0.4992  0.5     0.5008  1.5     2.5     8    20   20.48 800
    np.testing.assert_array_equal(rx.units_of(p, s, qmax), [0, 0, 0, 1, 2, 2, 8, 20, 20, 20])
    np.testing.assert_array_equal(rx.float_view(np.array([0, 1, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 32 - 1], dtype=np.uint32), 24).astype(np.float64),
                                  [0.0, 2.0 ** -24, 1.0, 1.0 + 2.0 ** -22, 256.0])


# ------------------------------------------------------------------------------------------------ the yardstick on the oracle alone
@pytest.mark.parametrize("shape_name", rx.SHAPE_NAMES)
def test_single_ray_yardstick_against_the_oracles_full_pass(oracle, shape_name):
    """The sum of the per-ray units, scaled back, lies within c_v * 2^-(S+1) + 2e-5 |want| + 2e-6 of the oracle's full float pass, with
    equal support; no piece rounds to zero units (nothing the float pass sees is lost); on the 5x20 case some voxels hold 2^24 units
    or more, where the float view has to round."""
    c0 = rx.case(shape_name)
    c, y = rx.yardstick(oracle, shape_name, "offsets_28mm_36mm", offset_lut(c0.shape))
    n = c.h * c.w
    assert y.s == rx.S_TABLE[(c.h, c.w, rx.VS)] and y.s == rx.scale_rule(n, rx.VS)[0]
    touched = int(np.count_nonzero(y.units))
    big = int((y.units >= 2 ** 24).sum())
    print(f"{shape_name}: S = {y.s}, {y.walked} rays walked, {touched} voxels touched, {big} hold U >= 2^24, {y.zero_pieces} zero-unit pieces, most pieces in a voxel {y.count.max()}")
    # the counts DESIGN.md 5.13 quotes (rays walked, voxels touched, voxels holding 2^24 units or more), pinned
    assert (y.walked, touched, big) == {"5x20": (65, 424, 30), "3x21": (35, 241, 7), "os1_16": (1481, 1872, 4)}[shape_name]
    assert y.zero_pieces == 0
    np.testing.assert_array_equal(y.units != 0, y.full != 0)
    got = y.units.astype(np.float64) * 2.0 ** -y.s
    excess = np.abs(got - y.full) - rx.view_bound(y, y.full)
    print(f"{shape_name}: largest |U 2^-S - float pass| = {np.abs(got - y.full).max():.3e} m, margin to the bound {-excess.max():.3e} m")
    assert (excess <= 0).all()
    assert y.units.max() <= n * y.qmax


def test_partition_property_is_not_vacuous_for_floats(oracle):
    """U(all) == U(even columns) + U(odd columns) holds for integers by construction; the oracle's FLOAT halves of the 5x20 case do
    not add up to its full pass bit for bit - the property the GPU test asserts of the units separates the two accumulations"""
    c = rx.case("5x20")
    ref = rc.detector(oracle, c.shape, offset_lut(c.shape), mask=c.mask, vs=rx.VS)
    try:
        gate = f32(ref.dp.raycast__min_intensity)
        col = np.arange(c.h * c.w) % c.w
        live = c.intensity >= gate
        full = rx.full_pass(ref, c).astype(f32)
        even = rx.full_pass(ref, c, np.flatnonzero(live & (col % 2 == 0))).astype(f32)
        odd = rx.full_pass(ref, c, np.flatnonzero(live & (col % 2 == 1))).astype(f32)
        n_diff = int(((even + odd).astype(f32).view(np.uint32) != full.view(np.uint32)).sum())
        print(f"5x20: float halves differ from the full float pass in {n_diff} voxels")
        assert n_diff == 6  # (the count DESIGN.md 5.13 quotes)
    finally:
        ref.close()


# ------------------------------------------------------------------------------------------------ the wire format's numpy statement
def test_wire_format_module_carries_the_units_byte():
    """byte 112 of the snapshot header: S + 1 of a pending exact pass whose units travel, else 0 - bytes -> snapshot -> the same bytes"""
    from vofod_amd import mapsync as ms

    rec = {1: (np.array([1], np.uint32), np.array([5], np.uint32)), 2: (np.array([3], np.uint32), np.array([70000], np.uint32))}
    s = ms.Snapshot(maps=6, kind=ms.KIND_FULL, map_size=(2, 2, 2), map_offset=(0.0, 0.0, 0.0), voxel_size=0.5, score_init=0.0, raycast_pending=1, raycast_log2_units=17, records=rec)
    b = ms.encode(s)
    assert b[112] == 18 and not b[113:128].any()
    d = ms.decode(b)
    assert d.raycast_log2_units == 17 and np.array_equal(ms.encode(d), b)
    s.raycast_log2_units = None
    b0 = ms.encode(s)
    assert not b0[112:128].any() and ms.decode(b0).raycast_log2_units is None
    for at, val in ((113, 1), (127, 9), (112, 26)):
        bad = b.copy()
        bad[at] = val
        with pytest.raises(ValueError):
            ms.decode(bad)
    bad = b.copy()
    bad[80:84] = 0  # raycast_pending: the byte without a pending pass
    with pytest.raises(ValueError):
        ms.decode(bad)
    for kw in (dict(raycast_pending=0), dict(maps=3)):
        with pytest.raises(ValueError):
            ms.encode(ms.Snapshot(**{**dict(maps=6, kind=ms.KIND_FULL, map_size=(2, 2, 2), map_offset=(0.0, 0.0, 0.0), voxel_size=0.5, score_init=0.0, raycast_pending=1,
                                            raycast_log2_units=17), **kw}))
