"""The handle-free entry points (vofod_amd/csrc/api_host.h) without a GPU.

1. api_host_check.cpp compiles the header alone with the host compiler under -fsanitize=address,undefined and calls every
   function of it on small inputs and at its edges; the test builds and runs it.
2. libvofod_hip.so loads without a device (tests/test_capi_symbols.py relies on that): the same functions of the product, called
   through ctypes, against the CPU oracle's on the same inputs - bit for bit, as the GPU tests compare them
   (tests/test_gpu_bench_shape.py: load_cloud; the LUTs and the mask feed tests/test_gpu_parity.py's raycast sequence, whose maps
   agree only where these do).  The oracle has no column poses and no serialisers: those are the check program's alone."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from vofod_amd import capi
from vofod_amd.detector import ScanData, check_sensor_params, load_cloud, mask_layout, ouster_lut, sim_lut

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vofod_amd" / "csrc"


def test_api_host_check_runs_clean_under_the_sanitizers():
    r = subprocess.run(["make", "-C", str(CSRC), "api_host_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = subprocess.run([str(CSRC / "api_host_check")], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands on stderr)
    assert out.stdout.strip() == "api_host_check: ok"


@pytest.fixture(scope="module")
def product():
    so = CSRC / "libvofod_hip.so"
    if not so.exists():  # hipcc cross-compiles gfx950 without a GPU
        subprocess.run(["make", "-C", str(CSRC)], check=True, capture_output=True)
    return capi.Library(so, "vofod_")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_default_params_equal_the_oracles(oracle, product):
    got = []
    for lib in (oracle, product):
        sp, dp = capi.StaticParams(), capi.DynParams()
        C.memset(C.byref(sp), 0xA5, C.sizeof(sp))  # (padding included: the call assigns whole structs)
        C.memset(C.byref(dp), 0xA5, C.sizeof(dp))
        lib.default_params(C.byref(sp), C.byref(dp))
        got.append((bytes(sp), bytes(dp)))
    assert got[0] == got[1]


@pytest.mark.parametrize("w,h,vfov", [(2, 2, 0.5), (1024, 16, np.deg2rad(33.2)), (37, 5, 1.0)])
def test_sim_lut_equals_the_oracles(oracle, product, w, h, vfov):
    np.testing.assert_array_equal(_bits(sim_lut(product, w, h, vfov)), _bits(sim_lut(oracle, w, h, vfov)))


@pytest.mark.parametrize("w,h,with_tf", [(1, 1, True), (64, 16, True), (33, 7, False)])
def test_ouster_lut_equals_the_oracles(oracle, product, w, h, with_tf):
    rng = np.random.default_rng(w * h)
    altitude = np.linspace(16.6, -16.6, h)
    azimuth = rng.uniform(-3.2, 3.2, h)
    tf = None
    if with_tf:
        tf = np.eye(4)
        tf[:3, :3] = [[-1, 0, 0], [0, -1, 0], [0, 0, 1]]
        tf[:3, 3] = [0.0, 0.0, 36.18]
    (d0, o0), (d1, o1) = (ouster_lut(lib, w, h, azimuth, altitude, origin_mm=15.806, tf=tf) for lib in (oracle, product))
    np.testing.assert_array_equal(_bits(d1), _bits(d0))
    np.testing.assert_array_equal(_bits(o1), _bits(o0))


def test_mask_layout_equals_the_oracles(oracle, product):
    w, h = 24, 6
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    shifts = [None, np.zeros(h, np.int32), np.array([0, 1, w - 1, w, w + 5, 3 * w + 2], np.int32)]  # below, at and beyond the width
    for shift in shifts:
        for mangle in (True, False):
            np.testing.assert_array_equal(mask_layout(product, img, w, h, shift, mangle), mask_layout(oracle, img, w, h, shift, mangle))
    np.testing.assert_array_equal(mask_layout(product, None, w, h, shifts[2]), mask_layout(oracle, None, w, h, shifts[2]))
    # a negative shift: the reference indexes its vector out of range there; the product refuses it
    neg = np.array([0, 0, -1, 0, 0, 0], np.int32)
    out = np.zeros(w * h, np.uint8)
    assert product.mask_layout(capi.ptr(img), w, h, capi.ptr(neg), 1, capi.ptr(out)) == capi.ERR_INVALID_ARG


def test_check_sensor_params_equals_the_oracles(oracle, product):
    """points of 48 bytes (the layout of a PCL cloud with padding), the first valid pixel the last one, then a point beside its ray"""
    w, h = 8, 4
    n = w * h
    dirs = sim_lut(oracle, w, h, 0.6)
    offs = np.tile(np.array([0.0, 0.01, 0.02], np.float32), (n, 1))
    cloud = np.zeros(n, np.dtype({"names": ["x", "y", "z", "range"], "formats": ["<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 16], "itemsize": 48}))
    cloud["range"][n - 1] = 2500
    for c, a in zip("xyz", range(3)):
        cloud[c][n - 1] = dirs[n - 1, a] * np.float32(2.5) + offs[n - 1, a]
    mask = np.ones(n, np.uint8)
    base = cloud.ctypes.data

    def scan():
        return ScanData(x=base, y=base + 4, z=base + 8, range=base + 16, width=w, height=h, stride_bytes=48)

    cases = [(offs, mask), (None, mask), (offs, None)]
    none_valid = mask.copy()
    none_valid[n - 1] = 0
    cases.append((offs, none_valid))
    for o, m in cases:
        a, b = (check_sensor_params(lib, scan(), dirs, o, m) for lib in (oracle, product))
        assert a == b, (a, b)
    assert check_sensor_params(product, scan(), dirs, offs, mask) == (True, True)
    assert check_sensor_params(product, scan(), dirs, offs, none_valid) == (True, False)
    cloud["x"][n - 1] += np.float32(0.01)
    assert check_sensor_params(product, scan(), dirs, offs, mask) == check_sensor_params(oracle, scan(), dirs, offs, mask) == (False, True)


def test_load_cloud_equals_the_oracles(oracle, product, tmp_path):
    text = "5\n1 2 3\n\n4 5\n6.5\t7.5  8.5\r\n\r\n   \t \n-1e2 0.25 9 77\r\n10 11 12"
    for name, count in (("cloud.pts", 4), ("cloud.xyz", 4)):  # (.pts: the first line is the count; elsewhere "5" is a short line)
        f = tmp_path / name
        f.write_bytes(text.encode())
        a, b = load_cloud(oracle, str(f)), load_cloud(product, str(f))
        assert a.shape == (count, 3)
        np.testing.assert_array_equal(_bits(b), _bits(a))
        # a capacity below the count: the first points, the count of all, VOFOD_ERR_CAPACITY
        for lib in (oracle, product):
            part, n = np.full((2, 3), -1, np.float32), C.c_size_t(0)
            assert lib.load_cloud(str(f).encode(), capi.ptr(part), 2, C.byref(n)) == capi.ERR_CAPACITY and n.value == count
            np.testing.assert_array_equal(_bits(part), _bits(a[:2]))
