"""Motion-compensated rays without a GPU (include/vofod.h, MOTION-COMPENSATED RAYS): the yardsticks tests/test_gpu_raycast_motion.py
holds k_raycast_motion to are held to each other, the numpy definition to its two exact cases, and the physical claim - a rigid
ray of a moving sensor erodes the background its own scan has just measured - is put in numbers on the yardsticks alone."""
import ctypes as C

import numpy as np

from vofod_amd import capi, synth

import range_motion_cases as rm
import raycast_motion_cases as rc
import statements
from test_range_image_cpu import offset_lut, sim_directions

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def test_header_mirror_and_wrapper():
    assert "set_raycast_motion" in capi.declared_entry_points() and "set_raycast_motion" in capi.PRODUCT_ONLY
    res, args = capi._SIGS["set_raycast_motion"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int]
    assert "int vofod_set_raycast_motion(vofod_handle* h, int on);" in capi.HEADER.read_text()


def test_oracle_has_no_switch(oracle):
    assert not hasattr(oracle, "set_raycast_motion")


# ------------------------------------------------------------------------------------------------ 1. the two yardsticks agree
def test_quarter_turn_oracle_sum_is_the_geometry_statement(oracle):
    """OS1-16 at 0.5 m, the scene, LUT with beam offsets, mask and intensity gate of the whole-scan raycast statement; a random
    quarter turn per measurement column and random shifts.  The sum of the oracle's four gated rigid passes against the float64
    geometry of the rays d', o' - the statement's own tolerances (the oracle adds nothing)."""
    st = rc.statement_setup(oracle)
    try:
        s, w = st.scan, st.w
        shift = rm.shifts("random", st.h, w, seed=5)
        k_of_m, table = rc.quarter_table(w, seed=5)
        got = rc.oracle_quarter_sum(st.det, k_of_m, w, shift, s.intensity, s.range, s.tf)
        dm, om = rc.ray_definition(st.dirs, st.offs, table, w, shift)
        want, n_cast = rc.geometry_statement(st.det, st.det.dp, s.tf, dm, om, st.mask, s.intensity, s.range)
        assert n_cast > 0.4 * st.h * w and np.count_nonzero(want) > 20_000
        rc.assert_pass_matches_statement(got, want, what="quarter-turn oracle sum against the geometry statement")
        # the table matters: the rigid pass of the same scan lies elsewhere
        assert st.det.raycast_begin(s.scan, s.tf) == capi.OK
        rigid = st.det.read_map(capi.MAP_RAYCAST).astype(np.float64).reshape(-1)
        st.det.raycast_finish(allow=(capi.ERR_RAYCAST_NO_DETECTION,))
        assert ((rigid != 0) != (got != 0)).any() and not np.allclose(rigid, got, rtol=2e-5, atol=1e-3)  # (the fan is a full turn: most of the support is shared, the lengths are not)
    finally:
        st.det.close()


# ------------------------------------------------------------------------------------------------ 2., 3. the definition's exact cases
def test_identity_table_returns_the_lut_values():
    for shape_name in ("5x20", "3x21", "os1_16"):
        shape = rm.SHAPES[shape_name]
        h, w = shape[:2]
        d, o = offset_lut(shape)
        for kind in rm.SHIFTS:
            dm, om = rc.ray_definition(d, o, rm.identity_poses(w), w, rm.shifts(kind, h, w, seed=1))
            assert np.array_equal(dm, d.reshape(-1, 3)) and np.array_equal(om, o.reshape(-1, 3))  # (as values: a zero may change sign)
        dm, om = rc.ray_definition(d, None, rm.identity_poses(w), w)
        assert np.array_equal(dm, d.reshape(-1, 3)) and not om.any()


def test_quarter_turns_are_signed_permutations_bit_for_bit():
    shape = rm.SHAPES["3x21"]
    h, w = shape[:2]
    d, o = offset_lut(shape)
    d, o = d.reshape(-1, 3), o.reshape(-1, 3)
    want = {0: lambda v: (v[:, 0], v[:, 1]), 1: lambda v: (-v[:, 1], v[:, 0]), 2: lambda v: (-v[:, 0], -v[:, 1]), 3: lambda v: (v[:, 1], -v[:, 0])}
    for kind in rm.SHIFTS:
        shift = rm.shifts(kind, h, w, seed=2)
        k_of_m, table = rc.quarter_table(w, seed=2)
        assert set(np.abs(table).reshape(-1).tolist()) <= {0.0, 1.0} and not table[:, :, 3].any()
        dm, om = rc.ray_definition(d, o, table, w, shift)
        i = np.arange(h * w)
        m = rm.measurement_column(i // w, i % w, w, shift)
        for k in range(4):
            at = k_of_m[m] == k
            assert at.any()
            for got, src in ((dm, d), (om, o)):
                x, y = want[k](src[at])
                # (x + (+0) and x * 1 are exact; only the sign of a zero may differ: none here)
                np.testing.assert_array_equal(bits(got[at, 0]), bits(x))
                np.testing.assert_array_equal(bits(got[at, 1]), bits(y))
                np.testing.assert_array_equal(bits(got[at, 2]), bits(src[at, 2]))
    # tf o T_k is exact, and R (T d) == (R T) d in the rigid pass's association (float32, the first addition commuted)
    tf = synth.make_pose(3)
    R = tf[:, :3]
    for k in range(4):
        tk = rc.compose_quarter(tf, k)
        Td = np.stack(list(want[k](d)) + [d[:, 2]], axis=1).astype(f32)
        for r in range(3):
            lhs = (((R[r, 0] * Td[:, 0]).astype(f32) + (R[r, 1] * Td[:, 1]).astype(f32)).astype(f32) + (R[r, 2] * Td[:, 2]).astype(f32)).astype(f32)
            rhs = (((tk[r, 0] * d[:, 0]).astype(f32) + (tk[r, 1] * d[:, 1]).astype(f32)).astype(f32) + (tk[r, 2] * d[:, 2]).astype(f32)).astype(f32)
            np.testing.assert_array_equal(bits(lhs), bits(rhs))
        np.testing.assert_array_equal(tk[:, 3], tf[:, 3])


# ------------------------------------------------------------------------------------------------ 4. the physical claim
def dilate26(cells, sizes):
    """flat indices of the voxels `cells` ([n, 3] integer x, y, z) and their 26 neighbours inside the map"""
    sx, sy, sz = sizes
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                c = cells + np.array([dx, dy, dz])
                ok = np.all((c >= 0) & (c < np.array(sizes)), axis=1)
                out.append((c[ok, 2] * sy + c[ok, 1]) * sx + c[ok, 0])
    return np.unique(np.concatenate(out))


def test_rigid_rays_of_a_moving_sensor_cross_the_returns_of_their_own_scan(oracle):
    """range_motion_cases.moving_frames (1 rad/s, 3 m/s over a 0.1 s scan, OS1-16) at 0.25 m: the path length the rays of a scan lay
    into the voxels that hold a compensated return of the same scan or one of their 26 neighbours, and into the return voxels
    alone.  Both passes are the float64 geometry statement (no product, no DDA): the rigid rays (identity table) and the
    compensated rays (the scan's table).  The numbers are printed and recorded in DESIGN.md 5.12; NOTHING is asserted about their
    order, because the measurement does not leave the factor of two the assertion was to wait for - it goes the other way:
        frame 0: 41 949 voxels at or beside a return: rigid 504.8 m, compensated 934.2 m;  the 3 792 return voxels alone: 64.4 m / 61.2 m
        frame 1: 52 734 voxels at or beside a return: rigid 395.7 m, compensated 950.0 m;  the 4 985 return voxels alone: 59.2 m / 57.5 m
    (of 298 312 m and 297 067 m laid in all).
    A ray ends voxel_size short of its return (vofod_nodelet.cpp:1457), so the last piece of every COMPENSATED ray lies beside its
    own return by construction, while a rigid ray ends about 2 m away from anything this scan flagged: the 26-neighbourhood counts
    the approach of a ray to its own return, which the sweep never sees (the return's voxels are flagged)."""
    det, sp, dp, h, w = statements.sensor_detector(oracle, "os1-16", 0.25)
    try:
        _, _, frames, col_tfs, shift = rm.moving_frames(n=2)
        d = sim_directions("os1-16")
        lo, hi = rm.exclude_bounds(sp)
        sizes = tuple(int(v) for v in det.map_size)
        off, vs = np.array(det.map_offset, dtype=np.float64), float(sp.voxel_size)
        for k, s in enumerate(frames):
            x, y, z, _ = rm.motion_definition(s.range, d, None, col_tfs, w, lo, hi, shift)
            p = np.stack([x, y, z], axis=1).astype(np.float64)
            p = p[np.isfinite(p).all(axis=1) & (np.asarray(s.range) != 0)]
            tf = np.asarray(s.tf, dtype=np.float64)
            world = p @ tf[:, :3].T + tf[:, 3]
            cells = np.floor((world - off) / vs).astype(np.int64)
            cells = cells[np.all((cells >= 0) & (cells < np.array(sizes)), axis=1)]
            own = np.unique((cells[:, 2] * sizes[1] + cells[:, 1]) * sizes[0] + cells[:, 0])
            near = dilate26(cells, sizes)
            assert len(own) > 1000 and len(near) > len(own)
            for name, table in (("rigid", rm.identity_poses(w)), ("compensated", col_tfs)):
                dm, om = rc.ray_definition(d, None, table, w, shift)
                acc, n_cast = rc.geometry_statement(det, dp, s.tf, dm, om, None, s.intensity, s.range)
                assert n_cast > 0.5 * h * w and np.isfinite(acc).all() and acc[near].sum() > 0
                print(f"moving frame {k}, {name} rays: {acc[near].sum():.1f} m in the {len(near)} voxels at or beside a compensated return, {acc[own].sum():.1f} m in the {len(own)} "
                      f"return voxels themselves, {acc.sum():.0f} m in all")
    finally:
        det.close()
