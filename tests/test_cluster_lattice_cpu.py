"""The adversarial lattices of tests/cluster_lattice_cases.py on the CPU: every case has the structure it claims under the plain
statement (statements.euclidean_components: scipy's connected components over FLANN's float32 `d2 < tol * tol`, label = smallest
member) - the condition that keeps a mis-drawn case from passing vacuously on the GPU - and the oracle's vofod_cluster equals that
statement bit for bit.  tests/test_gpu_cluster_lattice.py holds the HIP library to the same reference."""
import numpy as np
import pytest

from cluster_lattice_cases import ALTERNATING, BY_NAME, CACHE_SEQUENCE, CASES, WINDOW_LIMIT, expected_components, lattice_inputs, reference
from vofod_amd.detector import cluster


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_has_the_structure_it_claims(case):
    labels, nc = reference(case)
    assert expected_components(case, nc), (case.name, case.expect, nc, len(labels))
    if case.label_rank is not None:
        assert tuple(np.unique(labels)) == tuple(case.label_rank)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_cluster_equals_scipy_components(oracle, case):
    pts, keys, grid, _ = lattice_inputs(case)
    labels, nc = cluster(oracle, pts, keys, grid, case.tol)
    want, n_want = reference(case)
    np.testing.assert_array_equal(labels, want)
    assert nc == n_want


def test_the_table_covers_what_it_is_for():
    fams = {c.family for c in CASES}
    assert fams == {"voxel", "masks", "union"}
    assert {BY_NAME[n].family for n in ALTERNATING} == fams  # the alternating sequence: one case per family
    assert len({(BY_NAME[n].leaf, BY_NAME[n].tol) for n in ALTERNATING}) == 3
    assert CACHE_SEQUENCE[:5] == (0, 1, 0, 2, 0) and set(CACHE_SEQUENCE) == {0, 1, 2}  # hit, evict the other slot, hit again
    # boundary pairs off the origin: somewhere the float expression on the actual centres links a pair that sits exactly on the
    # tolerance, somewhere it does not - the cases do reach both answers
    far = [c for c in CASES if c.name.startswith("boundary_") and not c.name.endswith("_origin")]
    differs = 0
    for c in far:
        origin = BY_NAME[c.name.rsplit("_", 1)[0] + "_origin"]
        differs += reference(c)[1] != reference(origin)[1]
    assert differs >= 3, differs
    # centres quantised 8 km out against a tolerance a fraction of a quantum off the lattice distance: scipy links some of the 24
    # pairs and leaves others apart, on either side of the lattice distance
    quantised = [c for c in CASES if c.name.startswith("quantised_")]
    assert len(quantised) == 6
    for c in quantised:
        n_pairs = len(c.ijk) // 2
        assert n_pairs + 2 <= reference(c)[1] <= 2 * n_pairs - 2, (c.name, reference(c)[1])
    # the window limit: leaf and tolerances are what common.h's MAX_R = 31 admits and what it refuses
    leaf = float(np.float32(WINDOW_LIMIT["leaf"]))
    assert int(np.ceil(float(np.float32(WINDOW_LIMIT["tol"])) / leaf)) + 1 == 31
    assert int(np.ceil(float(np.float32(WINDOW_LIMIT["refused_tol"])) / leaf)) + 1 == 32
