"""vofod_detection_pixels without a GPU: the declared surface and its ctypes mirror, and the numpy statement
(detection_pixels_cases.py) on the oracle alone for every scene test_gpu_detection_pixels.py uses - with the conditions that keep
a GPU case from being empty."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import detection_pixels_cases as pxc
import tail_edges as te
from vofod_amd import capi
from vofod_amd.detector import ScanData

ROOT = Path(__file__).resolve().parent.parent


def test_declared_surface_and_mirror():
    """the header declares the call and the 16-byte span, capi mirrors both, the detector has the method"""
    from vofod_amd.detector import VoFOD

    text = capi.HEADER.read_text()
    assert "detection_pixels" in capi.declared_entry_points() and "detection_pixels" in capi.PRODUCT_ONLY
    m = re.search(r"typedef struct vofod_detection_span \{(.*?)\} vofod_detection_span;", text, flags=re.S)
    assert m and re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split() == "uint32_t id, frame; uint32_t first, count;".split()
    assert capi.DETECTION_SPAN.itemsize == 16 and [capi.DETECTION_SPAN.fields[k][1] for k in ("id", "frame", "first", "count")] == [0, 4, 8, 12]
    res, args = capi._SIGS["detection_pixels"]
    assert res is C.c_int and len(args) == 11 and args[1] is C.c_int and args[3] is C.c_size_t and args[8] is C.c_size_t and args[10] is C.c_int32
    decl = re.search(r"int vofod_detection_pixels\((.*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    assert len(decl.split(",")) == 11
    assert callable(getattr(VoFOD, "detection_pixels"))
    # stated in the header: the invariant, the in-place rule, the kernel's name
    for phrase in ("sum of the weights", "read in place", "k_det_pixels"):
        assert phrase in text, phrase


def test_hip_library_exports_detection_pixels(oracle):
    so = ROOT / "vofod_amd" / "csrc" / "libvofod_hip.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    lib = capi.Library(so, "vofod_")
    assert hasattr(lib, "detection_pixels") and not hasattr(oracle, "detection_pixels")
    # argument checks come before anything touches a device
    n = C.c_size_t(7)
    assert lib.detection_pixels(None, -1, None, 0, C.byref(n), None, None, None, 0, C.byref(n), capi.MEM_HOST) == capi.ERR_INVALID_ARG


def test_kernel_capacity_against_the_scenes():
    """PX_CAP, read from the kernel header: the 343-voxel detection stays below it, the 576- and 729-voxel ones exceed it"""
    src = (ROOT / "vofod_amd" / "csrc" / "detection_pixels.h").read_text()
    cap = int(re.search(r"constexpr\s+uint32_t\s+PX_CAP\s*=\s*(\d+)\s*;", src).group(1))
    sizes = [pxc.dpc.LARGEST[n] for n in pxc.LARGE_SCENES]
    assert sizes == [343, 576, 729] and sizes[0] < cap < sizes[1] and 2 * cap > sizes[2] > cap, (cap, sizes)


@pytest.fixture(scope="module")
def bench(oracle):
    from test_gpu_tail_edges import Bench

    b = Bench(oracle, oracle)  # the recipe of test_gpu_tail_edges.py, the oracle on both sides
    yield b
    b.close()


def _conditions(exp, gs):
    """(detections per frame, largest weight of a member voxel)"""
    per = [len(e) for e in exp]
    heavy = 0
    for e, g in zip(exp, gs):
        for epx, emem, exyz in e:
            assert len(epx) > 0 and (np.diff(epx.astype(np.int64)) > 0).all()
            heavy = max(heavy, int(np.bincount(emem).max()))
    return per, heavy


@pytest.mark.parametrize("name", pxc.ALL_SCENES)
def test_statement_holds_on_the_oracle(bench, oracle, name):
    """every hand-placed scene of the GPU file: the statement's pixels per member voxel number the oracle's weights (asserted inside
    expected_frame), every frame has a detection, frame 0 has two or more"""
    pxc.load(bench, name)
    da, pa, exp, gs = pxc.expected_batch(oracle, bench.ref, bench.scans, bench.tfs)
    per, heavy = _conditions(exp, gs)
    assert per == pa.tolist() and min(per) >= 1 and per[0] >= 2, per
    assert int(sum(len(p) for e in exp for p, _, _ in e)) >= int(da["n_points"].sum())
    if name in ("weights", "boundary"):
        assert heavy >= 2, heavy
    if name == "weights":
        assert heavy == pxc.dpc.HEAVY
    if name == "boundary":
        # target points on exact multiples of the voxel size in the world frame: listed, and on a cell boundary of the map
        xyz = np.vstack([x for _, _, x in exp[0]])
        on = pxc.boundary_fraction(xyz, te.VS, bench.off)
        assert on.sum() >= 1 and (~on).sum() >= 1, (int(on.sum()), len(on))
        print(f"\n[detection pixels] boundary: {int(on.sum())} of {len(on)} listed pixels of frame 0 on a cell boundary, {per[0]} detections")
    # the single read-only scans of the scene's scan frames
    for f in (0, 1):
        d1, g1 = bench.ref.process_scan(bench.scans[f], bench.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
        e1 = pxc.expected_frame(oracle, bench.ref, pxc.columns(bench.scans[f]), bench.tf, g1)
        assert len(e1) == len(d1) >= 1
        for (a, b, c), (a2, b2, c2) in zip(e1, exp[f]):
            np.testing.assert_array_equal(a, a2)
            np.testing.assert_array_equal(b, b2)


def test_statement_on_synthetic_frames(oracle):
    """the warmed OS1-16 pair the GPU file takes its range images and pose tables from, fed the decoded points: detections in the
    batch, member voxels of weight two and more, pixels ascending"""
    from test_gpu_range_image import warmed_pair
    from test_range_image_cpu import decode_definition

    p = warmed_pair(oracle, oracle, "os1-16", n_frames=4, max_batch=4)
    try:
        scans = [ScanData(*decode_definition(s.range, *p.lut), width=p.shape[1], height=p.shape[0]) for s in p.frames]
        da, pa, exp, gs = pxc.expected_batch(oracle, p.ref, scans, p.tfs)
        per, heavy = _conditions(exp, gs)
        assert sum(per) == len(da) >= 1 and heavy >= 2, (per, heavy)
    finally:
        p.ref.close()
        p.dev.close()
