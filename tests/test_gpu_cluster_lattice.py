"""The three general clustering implementations of the HIP library (launch_cluster, vofod_hip.hip) against the plain statement on the
adversarial lattices of tests/cluster_lattice_cases.py: labels equal scipy's connected components over FLANN's float32
`d2 < tol * tol`, label = smallest member, bit for bit - no tolerance, no oracle.  Every case runs twice, as planned and with
VOFOD_CCL=voxel (the switches are read on every call), each call is repeated on the same handle (k_brick_clear and the cached tables
leave no state behind), and the library's profiler says which family ran: k_union<2>, k_brick_link_tr or k_brick_union<1>.  The
route is asserted under the default switches only (a fallback switch in the environment reroutes the call; under
VOFOD_TEST_HARNESS_SELFCHECK `hip` is the oracle: no kernels, and no neighbour window to refuse a ratio by).
tests/test_cluster_lattice_cpu.py checks on the CPU that every case has the structure it claims."""
import ctypes as C
import os

import numpy as np
import pytest

import statements as st
from cluster_lattice_cases import ALTERNATING, BY_NAME, CACHE_SEQUENCE, CASES, WINDOW_LIMIT, lattice_inputs, reference
from test_gpu_parity import _fallback_switch_set
from test_gpu_stream_route import profiled_calls
from vofod_amd import capi
from vofod_amd.detector import cluster

pytestmark = pytest.mark.gpu

SELFCHECK = bool(os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"))
ROUTE_CHECKED = not SELFCHECK and not _fallback_switch_set()  # (read before any test sets VOFOD_CCL itself)
FAMILY_KERNEL = {"voxel": "k_union", "masks": "k_brick_link_tr", "union": "k_brick_union"}


@pytest.fixture(scope="module")
def det(hip):
    """the stateless entry points of the HIP library run on a handle's device and stream: one handle for the whole module"""
    d, *_ = st.sensor_detector(hip, "os1-16", 0.5)
    yield d
    d.close()


def families_run(ran):
    """the clustering families among the profiled kernels (instantiations carry their template argument: k_union<2>)"""
    return {f for f, k in FAMILY_KERNEL.items() if any(name.split("<")[0] == k for name in ran)}


def clustered(det, case):
    """(labels, number of clusters, families that ran) of one vofod_cluster call under the profiler"""
    pts, keys, grid, _ = lattice_inputs(case)
    det.lib.profile_enable(det.h, 1)
    try:
        labels, nc = cluster(det.lib, pts, keys, grid, case.tol, handle=det.h)
        ran = profiled_calls(det.lib, det)
    finally:
        det.lib.profile_enable(det.h, 0)
    return labels, nc, families_run(ran)


def check(det, case, family):
    want, n_want = reference(case)
    labels, nc, fams = clustered(det, case)
    np.testing.assert_array_equal(labels, want, err_msg=case.name)
    assert nc == n_want, (case.name, nc, n_want)
    if ROUTE_CHECKED:
        assert fams == {family}, (case.name, fams, family)
    return labels, nc


@pytest.mark.parametrize("forced_voxel", [False, True], ids=["planned", "ccl_voxel"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_labels_are_scipy_components(det, monkeypatch, case, forced_voxel):
    if forced_voxel:
        monkeypatch.setenv("VOFOD_CCL", "voxel")
    family = "voxel" if forced_voxel else case.family
    labels, nc = check(det, case, family)
    again, nc2 = check(det, case, family)  # the same call on the same handle: nothing of the first is left behind
    np.testing.assert_array_equal(again, labels)
    assert nc2 == nc


def test_alternating_tolerances_rebuild_the_cached_tables(det):
    """three (leaf, tolerance) pairs, one per family, on a handle that caches the tables of two (cluster_tables: two slots, filled in
    turn).  A, B, A: a hit on a slot while the other holds another case.  C evicts B's slot; A again: its slot survived the rebuild of
    its neighbour.  From then on in turn: every call evicts a slot and rebuilds it."""
    for n in CACHE_SEQUENCE:
        case = BY_NAME[ALTERNATING[n]]
        check(det, case, case.family)


@pytest.mark.parametrize("forced_voxel", [False, True], ids=["planned", "ccl_voxel"])
def test_ratio_past_the_window_limit_is_refused(det, monkeypatch, forced_voxel):
    """leaf 0.1, tolerance 3.05: R = ceil(tol / leaf) + 1 = 32 > MAX_R - VOFOD_ERR_INVALID_ARG, the caller's labels untouched; the
    handle clusters the admitted ratio right before and after"""
    if forced_voxel:
        monkeypatch.setenv("VOFOD_CCL", "voxel")
    case = BY_NAME["window_limit_30_cells"]
    family = "voxel" if forced_voxel else case.family
    check(det, case, family)
    if not SELFCHECK:
        pts, keys, grid, _ = lattice_inputs(case)
        labels = np.full(len(pts), 0xDEADBEEF, dtype=np.uint32)
        nc = C.c_size_t(0)
        status = det.lib.cluster(det.h, capi.ptr(pts), capi.ptr(keys), C.byref(grid), len(pts), WINDOW_LIMIT["refused_tol"], capi.ptr(labels), C.byref(nc))
        assert status == capi.ERR_INVALID_ARG
        assert (labels == 0xDEADBEEF).all() and nc.value == 0
        assert det.lib.last_error_string(det.h)  # ... and a message
    check(det, case, family)
