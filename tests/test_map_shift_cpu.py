"""vofod_map_shift without a GPU: the numpy statement (map_shift_cases.shift_statement) against cases written out by hand, and the
hand-over the GPU continuation test rests on, validated on the oracle itself - a fresh handle that receives another handle's three
maps through write_map and its latches through load_apriori with zero points continues exactly as that handle does."""
import numpy as np
import pytest

import map_shift_cases as mc
from vofod_amd import capi

I = 99  # init value of the hand-written cases


def _a():
    """S = (3, 2, 2): value 100 * iz + 10 * iy + ix + 1"""
    return np.array([[[1, 2, 3], [11, 12, 13]], [[101, 102, 103], [111, 112, 113]]], dtype=np.uint32)


HAND = {
    # new[ix] = old[ix + 1]: everything moves towards -x, the last column is new
    (1, 0, 0): [[[2, 3, I], [12, 13, I]], [[102, 103, I], [112, 113, I]]],
    (-1, 0, 0): [[[I, 1, 2], [I, 11, 12]], [[I, 101, 102], [I, 111, 112]]],
    (0, 1, 0): [[[11, 12, 13], [I, I, I]], [[111, 112, 113], [I, I, I]]],
    (0, -1, 0): [[[I, I, I], [1, 2, 3]], [[I, I, I], [101, 102, 103]]],
    (0, 0, 1): [[[101, 102, 103], [111, 112, 113]], [[I, I, I], [I, I, I]]],
    (0, 0, -1): [[[I, I, I], [I, I, I]], [[1, 2, 3], [11, 12, 13]]],
    # S - 1 on x: one column survives
    (2, 0, 0): [[[3, I, I], [13, I, I]], [[103, I, I], [113, I, I]]],
    (-2, 0, 0): [[[I, I, 1], [I, I, 11]], [[I, I, 101], [I, I, 111]]],
    # S: nothing survives
    (3, 0, 0): [[[I] * 3] * 2] * 2,
    (0, -2, 0): [[[I] * 3] * 2] * 2,
    (0, 0, 2): [[[I] * 3] * 2] * 2,
    (0, 0, 0): [[[1, 2, 3], [11, 12, 13]], [[101, 102, 103], [111, 112, 113]]],
    # all three axes at once
    (1, -1, 1): [[[I, I, I], [102, 103, I]], [[I, I, I], [I, I, I]]],
}


@pytest.mark.parametrize("s", list(HAND), ids=[str(s) for s in HAND])
def test_statement_against_hand_written_cases(s):
    got = mc.shift_statement(_a(), s, I)
    np.testing.assert_array_equal(got, np.array(HAND[s], dtype=np.uint32))
    assert got.dtype == np.uint32


def test_statement_is_the_definition_element_by_element():
    """the slices against the header's sentence, voxel by voxel, on an odd-sized array with every kind of shift"""
    rng = np.random.default_rng(3)
    a = mc.random_bits(rng, (4, 5, 7))
    for s in [(1, 0, 0), (-3, 2, 1), (6, -4, 3), (7, 0, 0), (0, 0, -4), (2, -3, 1), (-5, 4, -2), (0, 0, 0), (100, -100, 3)]:
        want = np.full_like(a, 0xDEAD)
        for iz in range(4):
            for iy in range(5):
                for ix in range(7):
                    jx, jy, jz = ix + s[0], iy + s[1], iz + s[2]
                    if 0 <= jx < 7 and 0 <= jy < 5 and 0 <= jz < 4:
                        want[iz, iy, ix] = a[jz, jy, jx]
        np.testing.assert_array_equal(mc.shift_statement(a, s, 0xDEAD), want, err_msg=str(s))


def test_shifted_offsets_do_not_drift():
    """base + k * voxel_size from an integer k: 1000 shifts there and 1000 back end on the bits they started from, and every
    offset on the way is the correctly rounded one"""
    base, vs = (40.0, 20.0, -1.25), 0.1
    k = np.zeros(3, dtype=np.int64)
    for step in [(3, -1, 0)] * 1000 + [(-3, 1, 0)] * 1000:
        k += step
        off = mc.shifted_offset(base, k, vs)
        assert off == tuple(float(np.float32(b + int(kk) * vs)) for b, kk in zip(base, k))
    assert mc.shifted_offset(base, k, vs) == tuple(float(np.float32(b)) for b in base)


def test_hand_over_continues_bit_for_bit(oracle):
    """Handle A runs the warm-up and goes on; handle B is fresh, takes A's maps and latches and runs the same scans: maps and
    flags are bit-equal after every scan and the detections equal but for the ids, which B counts from zero."""
    tgt = mc.TARGET_IN_AREA
    a = mc.make_det(oracle)
    warm_dets = mc.warm(a, tgt)
    id_shift = int(a.status().last_detection_id)
    assert id_shift == sum(len(d) for d in warm_dets) and id_shift > 0  # (the box behind the vehicle: B's ids really lag)
    b = mc.hand_over(oracle, {w: a.read_map(w) for w in mc.MAPS})
    sa, sb = a.status(), b.status()
    assert (sb.background_pts_sufficient, sb.sure_background_sufficient, sb.raycast_pending) == (1, 1, 0)
    assert (sa.background_pts_sufficient, sa.sure_background_sufficient, sa.raycast_pending) == (1, 1, 0)
    n_det = 0
    for k, s in enumerate(mc.continuation_scans(tgt)):
        da = a.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        db = b.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        mc.assert_detections_equal_mod_id(db, da, id_shift)
        np.testing.assert_array_equal(da["id"].astype(np.int64) - db["id"], np.full(len(da), id_shift))
        for which in (capi.MAP_VOXELS, capi.MAP_FLAGS):
            np.testing.assert_array_equal(mc.read_bits(a, which), mc.read_bits(b, which), err_msg=f"map {which} after scan {k}")
        assert a.status().raycast_pending == b.status().raycast_pending
        n_det += int((np.abs(da["position"] - np.array(tgt)).max(axis=1) < 1.0).sum()) if len(da) else 0
    assert n_det >= 1  # the box that appeared after the hand-over is detected


def test_continuation_at_the_new_offset_detects_the_box_in_the_new_strip(oracle):
    """the oracle's half of the GPU continuation test: handle B at the shifted offset, the statement applied to A's maps, sees
    the box that floats where the area only reaches after the shift"""
    tgt = mc.TARGET_IN_NEW_STRIP
    a = mc.make_det(oracle)
    mc.warm(a, tgt)
    off = mc.shifted_offset(tuple(a.sp.oparea_offset), mc.SHIFT, mc.VS)
    x_end_before = a.map_offset[0] + a.map_size[0] * mc.VS
    assert tgt[0] - mc.TARGET_SIZE / 2 > x_end_before  # the whole box lies beyond the last voxel of the unshifted map
    maps = {w: mc.shift_statement(mc.read_bits(a, w), mc.SHIFT, mc.init_bits(a, w)).view(np.float32) for w in mc.MAPS}
    b = mc.hand_over(oracle, maps, oparea_offset=off)
    np.testing.assert_array_equal(np.float32(b.map_offset), np.float32(a.map_offset) + np.float32(mc.VS) * np.float32(mc.SHIFT))
    n_det = 0
    for s in mc.continuation_scans(tgt):
        d = b.process_scan(s.scan, s.tf, flags=capi.SCAN_AUTO_RAYCAST)
        n_det += int((np.abs(d["position"] - np.array(tgt)).max(axis=1) < 1.0).sum()) if len(d) else 0
    assert n_det >= 1


def test_entry_point_is_declared_bound_and_exported():
    """include/vofod.h declares vofod_map_shift, the ctypes mirror binds it as a product-only call and the product library
    exports it (no device is touched: the library only has to load)"""
    from pathlib import Path

    assert "map_shift" in capi.declared_entry_points() and "map_shift" in capi._SIGS and "map_shift" in capi.PRODUCT_ONLY
    so = Path(capi.__file__).resolve().parent / "csrc" / "libvofod_hip.so"
    if not so.exists():  # hipcc cross-compiles gfx950 without a GPU
        import subprocess

        subprocess.run(["make", "-C", str(so.parent)], check=True, capture_output=True)
    lib = capi.Library(so, "vofod_")
    assert lib.map_shift(None, None, None) == capi.ERR_INVALID_ARG  # null handle: refused before anything is touched
