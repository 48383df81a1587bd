"""vofod_detection_points without a GPU: the ABI (struct size, exports) and the oracle-only self-check of the expected values
test_gpu_detection_points.py holds the kernel to (detection_points_cases.py says how they are built)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import detection_points_cases as dpc
from vofod_amd import capi

ROOT = Path(__file__).resolve().parent.parent


def test_extent_struct_is_40_bytes():
    assert C.sizeof(capi.DetectionExtent) == 40 and capi.DETECTION_EXTENT.itemsize == 40
    assert [capi.DETECTION_EXTENT.fields[k][1] for k in ("id", "frame", "first", "count", "aabb_min", "aabb_max")] == [0, 4, 8, 12, 16, 28]
    assert capi.POINTS_SYNC == -1


def test_hip_library_exports_detection_points():
    so = ROOT / "vofod_amd" / "csrc" / "libvofod_hip.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    assert "detection_points" in capi.declared_entry_points() and "detection_points" in capi.PRODUCT_ONLY
    lib = capi.Library(so, "vofod_")
    assert hasattr(lib, "detection_points")
    # argument checks come before anything touches a device
    n = C.c_size_t(7)
    assert lib.detection_points(None, -1, None, 0, C.byref(n), None, None, 0, C.byref(n), capi.MEM_HOST) == capi.ERR_INVALID_ARG


def test_oracle_does_not_export_detection_points(oracle):
    assert not hasattr(oracle, "detection_points")
    with pytest.raises(AttributeError):
        getattr(oracle.cdll, "vofod_oracle_detection_points")


@pytest.fixture(scope="module")
def bench(oracle):
    from test_gpu_tail_edges import Bench

    b = Bench(oracle, oracle)  # the recipe of test_gpu_tail_edges.py, the oracle on both sides
    yield b
    b.close()


@pytest.mark.parametrize("name", list(dpc.SCENES))
def test_expected_values_hold_on_the_oracle(bench, name):
    """every scene of the GPU file: detections per frame as the placed geometry says, detections and MAV clusters in the same
    order, n_points the member count, the first index first_member, the table's AABB numpy's min / max of the members - for the
    batch's debug view and for the read-only debug view of the frames that run as single scans"""
    scene = dpc.load(bench, name)
    ref = bench.ref
    da, pa, gs = ref.process_batch(bench.scans, bench.tfs, debug=True)
    assert pa.tolist() == dpc.PER_FRAME[name], pa.tolist()
    dpc.self_check(da, pa, gs)
    sizes = [len(e[1]) for e in dpc.expected_frame(gs[0])]
    if name in dpc.LARGEST:
        assert max(sizes) == dpc.LARGEST[name], sizes
    if name == "weights":
        cells, hits = dpc.weights_hits(scene)
        from statements import map_cells

        w = gs[0]["weighted"]
        cell = map_cells(w, bench.off.astype(np.float32), dpc.te.VS)
        got = {tuple(int(v) for v in c): int(r) for c, r in zip(cell, w["range"])}
        assert got == {tuple(int(v) for v in c): int(h) for c, h in zip(cells, hits)}
        ranges = np.concatenate([e[2]["range"] for e in dpc.expected_frame(gs[0])])
        assert sorted(ranges.tolist()) == sorted(hits.tolist()) and dpc.HEAVY in ranges  # every cell of the frame is a member of a detection
    else:
        assert all((g["weighted"]["range"] == 1).all() for g in gs)
    for f in scene.scan_frames:
        d1, g1 = ref.process_scan(bench.scans[f], bench.tf, flags=capi.SCAN_NO_MAP_UPDATE, debug=True)
        dpc.self_check(d1, [len(d1)], [g1])
        assert len(d1) == dpc.PER_FRAME[name][f]
    print(f"\n[detection points] {name}: detections per frame {pa.tolist()}, largest of frame 0 {max(sizes)} voxels, {sum(sizes)} points in frame 0")
