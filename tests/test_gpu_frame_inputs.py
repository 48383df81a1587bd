"""The frame kernel (k_frame_lds, kernels_frame.h) on the input layouts and operation areas the other batch tests never hand
over.  Those tests give it 4-byte-stride host columns of w*h % 4 == 0 points on the default area: the PACKED input pass and one
reference lattice (482 x 402 x 102 cells, eps 0.0017).  Here:

A. input layouts - arrays of structs, interleaved xyz, device memory, misaligned columns, point counts that are no multiple of
   four, the smallest sensors, frames full of fragile points: the strided input pass (profile label `*_strided`), or the
   per-column gather where a layout cannot be read in place;
B. the geometry table - a numpy float32 mirror of fill_ref_lattice (vofod_hip.hip) on thirteen areas at either side of each
   capacity condition and of eps < 0.05 (tests/frame_geometry.py; its CPU test is in tests/test_properties.py);
C. every row of that table on the GPU, with scene frames and with frames that fill the area up to its corners (the upper ends
   of the 9+2 / 9+2 / 6+2-bit cell-code fields);
D. areas 3-5 km from the origin, where eps reaches 0.036-0.047 and about half of the points take the fragile route, with
   adversarial frames just inside and just outside the eps band.

Every comparison is HIP against the CPU oracle fed the same points as plain host columns: bit-exact on the weighted cloud,
labels, cluster tables, is_close and classes, the helpers' tolerances on OBB floats, positions and confidences - in three views:
the full debug view (k_frame_lds_full*), the far-only view (k_frame_lds_far*) and the production call without debug output,
synchronous and as two tickets in flight."""
import ctypes as C
import os

import numpy as np
import pytest

from vofod_amd import capi, synth
from vofod_amd.detector import ScanData, VoFOD, default_params

from frame_geometry import FALLBACK_SWITCHES, TABLE, area_bounds, capacities, ref_lattice
from helpers import assert_detections_equal, assert_scan_debug_equal, far_view

pytestmark = pytest.mark.gpu
f32 = np.float32
SELFCHECK = bool(os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"))  # oracle against oracle: no kernels, no device memory
DEFAULT_AREA = ((40.0, 20.0, -1.25), (120.0, 100.0, 25.0))
OS1_16 = (16, 1024, 33.2, 120.0)


# ------------------------------------------------------------------------------------------------ detectors, frames, views
def make_area_pair(oracle, hip, area=DEFAULT_AREA, vs=0.25, shape=OS1_16, max_batch=8, **dyn):
    """an oracle detector and a HIP detector on the operation area `area` for a sensor of `shape` = (vrays, hrays, vfov_deg, range)"""
    dets = []
    for lib in (oracle, hip):
        sp, dp = default_params(lib)
        sp.voxel_size = vs
        sp.sensor_hrays, sp.sensor_vrays = shape[1], shape[0]
        sp.sensor_vfov = f32(np.deg2rad(shape[2]))
        sp.max_batch_frames = max_batch
        sp.oparea_offset[:] = area[0]
        sp.oparea_size[:] = area[1]
        for k, v in dyn.items():
            setattr(dp, k, v)
        dets.append(VoFOD(lib, sp, dp))
    return dets


def pose_at(seed, xy, z=None):
    tf = synth.make_pose(seed, xy=xy)
    if z is not None:
        tf[2, 3] = z  # (make_pose flies at 4-10 m: the tall areas set their own height)
    return tf


def scene_frames(area, sensor_xy, n, shape=OS1_16, scene_seed=3, seed0=40, n_targets=6, z=None):
    """(scene without targets, n scans of the same scene with floating targets) seen from `sensor_xy`"""
    warm_scene = synth.make_scene(scene_seed, area[0], area[1], n_targets=0, sensor_xy=sensor_xy)
    scene = synth.make_scene(scene_seed, area[0], area[1], n_targets=n_targets, sensor_xy=sensor_xy)
    np.testing.assert_array_equal(scene.boxes[: scene.n_static], warm_scene.boxes)  # same buildings (drawn first from the seed)
    frames = [synth.make_scan(scene, pose_at(seed0 + k, sensor_xy, z), shape, seed=seed0 + k) for k in range(n)]
    return warm_scene, scene, frames


def survey_free_space(det):
    """Stand-in for a long raycast history (the raycast role is out of scope here, as the range finder is for synth.seed_ground):
    every voxel the warm-up left unknown becomes sure air.  A target that appears afterwards is then not connected to the ground
    through unknown voxels (VoxelMap::exploreToGround): it is classified as floating and detected - 16 rings alone leave unknown
    gaps between the rays at any range, and a batch, which never updates the map, would report nothing."""
    m = det.read_map(capi.MAP_VOXELS)
    m[m == np.float32(det.sp.score_init)] = np.float32(det.dp.voxel_map__thresholds__frontiers)
    det.write_map(capi.MAP_VOXELS, m)


def warm_both(ref, dev, warm_scene, sensor_xy, shape=OS1_16, n_scans=2, z=None, seed0=900):
    """the same warm-up on both sides: surveyed background (apriori: sets both latches), the ground patch below the sensor and a
    few map-updating scans of the scene before the targets appear"""
    ap = synth.apriori_points(warm_scene, float(ref.sp.voxel_size))
    for d in (ref, dev):
        d.load_apriori(ap)
        synth.seed_ground(d, xy=sensor_xy)
    for k in range(n_scans):
        s = synth.make_scan(warm_scene, pose_at(seed0 + k, sensor_xy, z), shape, seed=seed0 + k)
        for d in (ref, dev):
            d.process_scan(s.scan, s.tf)
    for d in (ref, dev):
        survey_free_space(d)
    st = ref.status()
    assert st.background_pts_sufficient and st.sure_background_sufficient


def _rebase(got, want):
    got = got.copy()
    if len(got) and len(want):
        got["id"] = (got["id"].astype(np.int64) + int(want["id"][0]) - int(got["id"][0])).astype(got["id"].dtype)
    return got


def _profiled(dev, call):
    from test_gpu_stream_route import profiled_calls

    dev.lib.profile_enable(dev.h, 1)
    try:
        out = call()
        names = profiled_calls(dev.lib, dev)
    finally:
        dev.lib.profile_enable(dev.h, 0)
    return out, names


def _switches():
    """the switches of tools/run_fallback_matrix.sh that are set (FALLBACK_SWITCHES: tests/test_properties.py holds the list to the
    script): each turns a fast path off and may move a batch, or a part of it, to other kernels.  No other variable
    (VOFOD_TRACE, ...) loosens a route assertion."""
    return sorted(k for k in FALLBACK_SWITCHES if k in os.environ)


def assert_route(names, want, exact=None, rerun_ok=False):
    """`names`: kernels one call launched.  want = "strided" / "packed": a frame-kernel label of that input pass ran and none of
    the other; "general": no frame kernel, k_bbox (the general voxelisation) ran.  `exact`: the label itself, asserted where no
    environment switch reroutes the batch.  Unless `rerun_ok`, k_bbox did not run beside the frame kernel: no frame overflowed it,
    the batch was not run again on the general kernels - what was compared is the frame kernel's own output.  Nothing to assert
    oracle against oracle, or with the LDS kernels switched off."""
    if SELFCHECK:
        return
    fam = [n for n in names if n.startswith("k_frame_lds")]
    if os.environ.get("VOFOD_CCL") == "voxel" or os.environ.get("VOFOD_BRICK_LDS") == "0":  # (tools/run_fallback_matrix.sh: no frame kernel at all)
        assert not fam and "k_bbox" in names, names
        return
    if want == "general":
        assert not fam and "k_bbox" in names, names
        return
    assert fam, names
    if not rerun_ok and not _switches():
        assert "k_bbox" not in names, names
    strided = [n for n in fam if n.endswith("_strided")]
    assert (strided == fam) if want == "strided" else (not strided), (want, names)
    if exact and not _switches():
        assert exact + ("_strided" if want == "strided" else "") in names, (exact, names)


def three_views(ref, dev, scans_ref, scans_dev, tfs, want, case, min_crop, min_vox, expect_far=True, clusters_cap=8192, chunk=32, rerun_ok=False):
    """HIP (`scans_dev`: the layout under test) against the oracle (`scans_ref`: the same points as plain host columns, in chunks
    of `chunk` frames): full debug view, far-only view, production call and two tickets.  Floors on the oracle's own output."""
    n = len(scans_ref)
    (db, pb, gb), names_full = _profiled(dev, lambda: dev.process_batch(scans_dev, tfs, debug=True, clusters_cap=clusters_cap))
    (_, pf, gf), names_far = _profiled(dev, lambda: dev.process_batch(scans_dev, tfs, debug=True, clusters_cap=clusters_cap, far_only=True))
    (dc, pc), names_prod = _profiled(dev, lambda: dev.process_batch(scans_dev, tfs))
    tickets = [dev.batch_submit(scans_dev, tfs) for _ in range(2)]
    collected = [dev.batch_collect(t) for t in tickets]
    n_det = 0
    crops, voxels = [], []
    for f0 in range(0, n, chunk):
        f1 = min(f0 + chunk, n)
        da, pa, ga = ref.process_batch(scans_ref[f0:f1], tfs[f0:f1], debug=True, clusters_cap=clusters_cap)
        n_det += len(da)
        crops += [g["n_input_after_crop"] for g in ga]
        voxels += [len(g["weighted"]) for g in ga]
        for per in (pb, pf, pc, collected[0][1], collected[1][1]):
            np.testing.assert_array_equal(per[f0:f1], pa)
        for dets in (db, dc, collected[0][0], collected[1][0]):
            sel = dets[(dets["frame"] >= f0) & (dets["frame"] < f1)].copy()
            sel["frame"] -= f0
            assert_detections_equal(da, _rebase(sel, da))
        for k, (x, y, yf) in enumerate(zip(ga, gb[f0:f1], gf[f0:f1])):
            try:
                assert_scan_debug_equal(x, y)
            except AssertionError as e:
                raise AssertionError(f"{case}: full view, frame {f0 + k}: {e}") from e
            try:
                assert_scan_debug_equal(far_view(x), yf)
            except AssertionError as e:
                raise AssertionError(f"{case}: far view, frame {f0 + k}: {e}") from e
    print(f"{case}: after crop {min(crops)}..{max(crops)}, voxels {min(voxels)}..{max(voxels)}, detections {n_det}")
    assert min(crops) >= min_crop and min(voxels) >= min_vox, (crops, voxels)
    assert n_det > 0, case  # (every case: classification and the tail work on something)
    views = {"full": names_full, "far": names_far, "production": names_prod}
    print(f"{case}: route " + ", ".join(f"{v}: {sorted(n for n in nm if n.startswith('k_frame_lds') or n == 'k_bbox')}" for v, nm in views.items()))
    assert_route(names_full, want, "k_frame_lds_full", rerun_ok)
    assert_route(names_far, want, "k_frame_lds_far" if expect_far else None, rerun_ok)
    assert_route(names_prod, want, "k_frame_lds_far" if expect_far else None, rerun_ok)
    return gb


# ------------------------------------------------------------------------------------------------ layouts
AOS48 = np.dtype({"names": ["x", "y", "z", "intensity", "range"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 16, 36], "itemsize": 48})  # ouster_ros::Point


def _xyz(s):
    return np.asarray(s.x, f32), np.asarray(s.y, f32), np.asarray(s.z, f32)


def lay_aos48(s, with_columns=False):
    """-> (bytes of the block, offsets of x / y / z, stride, offsets of intensity / range or None)"""
    x, y, z = _xyz(s)
    a = np.zeros(x.size, dtype=AOS48)
    a["x"], a["y"], a["z"] = x, y, z
    a["intensity"] = 7.0 if s.intensity is None else s.intensity
    a["range"] = 1000 if s.range is None else s.range
    return a.view(np.uint8).reshape(-1), (0, 4, 8), 48, ((16, 36) if with_columns else None)


def lay_interleaved(s, stride):
    x, y, z = _xyz(s)
    a = np.full((x.size, stride // 4), 9.5, dtype=f32)
    a[:, 0], a[:, 1], a[:, 2] = x, y, z
    return a.view(np.uint8).reshape(-1), (0, 4, 8), stride, None


def lay_packed_struct(s, offsets, itemsize):
    """a packed struct of `itemsize` bytes with x, y, z at `offsets` (no float of it need be aligned in host memory)"""
    x, y, z = _xyz(s)
    dt = np.dtype({"names": ["x", "y", "z"], "formats": ["<f4", "<f4", "<f4"], "offsets": list(offsets), "itemsize": itemsize})
    a = np.zeros(x.size, dtype=dt)
    a["x"], a["y"], a["z"] = x, y, z
    return a.view(np.uint8).reshape(-1), tuple(offsets), itemsize, None


def lay_columns(s, shift=0):
    """three 4-byte-stride columns, each `shift` bytes behind a 16-byte boundary of the block"""
    x, y, z = _xyz(s)
    pitch = (x.size * 4 + 16 + 15) // 16 * 16
    b = np.zeros(3 * pitch, dtype=np.uint8)
    for c, v in enumerate((x, y, z)):
        b[c * pitch + shift : c * pitch + shift + v.size * 4] = v.view(np.uint8)
    return b, (shift, pitch + shift, 2 * pitch + shift), 4, None


def host_scan(s, lay):
    """ScanData over a host block laid out by one of the lay_* functions (16-byte aligned base); the block rides along as .keep"""
    raw, offs, stride, cols = lay
    buf = np.zeros(raw.size + 16, dtype=np.uint8)
    o = (-buf.ctypes.data) % 16
    blk = buf[o : o + raw.size]
    blk[:] = raw
    base = blk.ctypes.data
    sd = ScanData(x=base + offs[0], y=base + offs[1], z=base + offs[2], width=s.scan.width, height=s.scan.height, stride_bytes=stride,
                  intensity=None if cols is None else base + cols[0], range=None if cols is None else base + cols[1])
    sd.keep = buf
    return sd


class DeviceBlocks:
    """device memory from the HIP runtime through ctypes (the runtime the product already loaded); frees what it allocated"""

    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so")
        self.rt.hipMalloc.argtypes, self.rt.hipMemcpy.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.rt.hipFree.argtypes = [C.c_void_p]
        self.ptrs = []

    def scan(self, s, lay):
        raw, offs, stride, _ = lay
        raw = np.ascontiguousarray(raw)
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), raw.size) == 0
        self.ptrs.append(p)
        assert p.value % 16 == 0
        assert self.rt.hipMemcpy(p, raw.ctypes.data_as(C.c_void_p), raw.size, 1) == 0  # hipMemcpyHostToDevice
        return ScanData(x=p.value + offs[0], y=p.value + offs[1], z=p.value + offs[2], width=s.scan.width, height=s.scan.height, stride_bytes=stride, memspace=capi.MEM_DEVICE)

    def free(self):
        for p in self.ptrs:
            assert self.rt.hipFree(p) == 0
        self.ptrs = []


# ------------------------------------------------------------------------------------------------ A. input layouts
@pytest.fixture(scope="module")
def default_case(oracle, hip):
    """one warmed pair on the default area for OS1-16 frames and the frames every layout case hands over (batches are read-only:
    the map stays as warmed)"""
    ref, dev = make_area_pair(oracle, hip, max_batch=8)
    warm_scene, _, frames = scene_frames(DEFAULT_AREA, (0.0, 0.0), 6, scene_seed=5, seed0=70)
    warm_both(ref, dev, warm_scene, (0.0, 0.0))
    return ref, dev, frames


DEFAULT_FLOORS = (3000, 2000)  # OS1-16 frames of default_case: 3 719..8 738 points after the crops, 2 325..4 160 voxels (the oracle's own output)


HOST_LAYOUTS = {
    "aos48": (lambda s: lay_aos48(s), "strided"),
    "aos48_with_intensity_range": (lambda s: lay_aos48(s, True), "strided"),
    "xyz12": (lambda s: lay_interleaved(s, 12), "strided"),
    "xyz16": (lambda s: lay_interleaved(s, 16), "strided"),
    "odd20_x_at_1": (lambda s: lay_packed_struct(s, (1, 5, 9), 20), "strided"),
    "odd20_skewed_gathered": (lambda s: lay_packed_struct(s, (1, 6, 11), 20), "packed"),
    "packed13_gathered": (lambda s: lay_packed_struct(s, (1, 5, 9), 13), "packed"),
    "columns": (lambda s: lay_columns(s), "packed"),
}


@pytest.mark.parametrize("layout", list(HOST_LAYOUTS))
def test_host_layouts(default_case, layout):
    """Host layouts of a whole batch.  aos48 (x, y, z of a 48-byte ouster_ros::Point, no other column): one copy of the block,
    read in place - strided.  aos48_with_intensity_range (the pointers the nodelet holds): a batch never reads those two
    columns, stage_inputs hands stage_cloud NULL for them, so the frames take the same one-copy path - strided.  xyz12 / xyz16:
    interleaved points, one copy - strided.  odd20_x_at_1 (a packed 20-byte struct, x / y / z at +1 / +5 / +9): no float is aligned
    in HOST memory, but the one copy starts at x, so on the device the three members lie at +0 / +4 / +8 of a 256-byte aligned block
    at a stride of 20 - read in place, strided (stage_cloud tests the members' distances, not their addresses; nothing is
    dereferenced on the host).  odd20_skewed (+1 / +6 / +11) and packed13 (a 13-byte struct): distances or stride that are no
    multiples of 4 cannot be read in place on the device - gathered column by column into the packed staging block, packed.
    columns: the layout of every other test, the converse - packed and no strided label."""
    ref, dev, frames = default_case
    make, want = HOST_LAYOUTS[layout]
    scans_dev = [host_scan(s, make(s)) for s in frames]
    tfs = np.stack([s.tf for s in frames])
    three_views(ref, dev, [s.scan for s in frames], scans_dev, tfs, want, f"A/{layout}", *DEFAULT_FLOORS)


def test_mixed_batch_one_unpacked_frame_makes_the_batch_strided(oracle, hip):
    """frame 0 at stride 16 sizes the staging block; the frames at stride 48 do not fit its pitch and are gathered into packed
    columns, the frames at stride 4 are copied as columns: one frame read in place at stride 16 and the whole batch takes the
    strided pass (which then reads the gathered frames at stride 4).  A pair of its own: a workspace that has staged 48-byte
    structs before keeps a block they fit."""
    ref, dev = make_area_pair(oracle, hip, max_batch=6)
    warm_scene, _, frames = scene_frames(DEFAULT_AREA, (0.0, 0.0), 6, scene_seed=5, seed0=70)
    warm_both(ref, dev, warm_scene, (0.0, 0.0))
    lays = [lay_interleaved(frames[0], 16)] + [lay_aos48(frames[1]), lay_columns(frames[2]), lay_aos48(frames[3]), lay_columns(frames[4]), lay_aos48(frames[5], True)]
    scans_dev = [host_scan(s, l) for s, l in zip(frames, lays)]
    tfs = np.stack([s.tf for s in frames])
    three_views(ref, dev, [s.scan for s in frames], scans_dev, tfs, "strided", "A/mixed_16_48_4", *DEFAULT_FLOORS)


@pytest.mark.skipif(SELFCHECK, reason="device memory: the oracle reads host memory only")
@pytest.mark.parametrize("layout", ["aos48", "columns_plus_4", "columns_plus_8", "columns_plus_12", "columns_aligned"])
def test_device_layouts(default_case, layout):
    """VOFOD_MEM_DEVICE inputs are read where they lie.  aos48: strided.  Columns at stride 4 whose bases are 4-byte but not
    16-byte aligned (every column 4, 8, 12 bytes behind a 16-byte boundary): the 16-byte loads of the packed pass would be
    misaligned - strided.  Aligned device columns: packed (the converse)."""
    ref, dev, frames = default_case
    blocks = DeviceBlocks()
    try:
        if layout == "aos48":
            scans_dev, want = [blocks.scan(s, lay_aos48(s)) for s in frames], "strided"
        else:
            shift = {"columns_plus_4": 4, "columns_plus_8": 8, "columns_plus_12": 12, "columns_aligned": 0}[layout]
            scans_dev, want = [blocks.scan(s, lay_columns(s, shift)) for s in frames], "strided" if shift else "packed"
            assert all(sd.x % 16 == shift and sd.y % 16 == shift and sd.z % 16 == shift for sd in scans_dev)
        tfs = np.stack([s.tf for s in frames])
        three_views(ref, dev, [s.scan for s in frames], scans_dev, tfs, want, f"A/device_{layout}", *DEFAULT_FLOORS)
    finally:
        blocks.free()


@pytest.mark.parametrize("vrays,hrays", [(17, 1021), (15, 1022), (15, 1021)])
def test_point_counts_that_are_no_multiple_of_four(oracle, hip, vrays, hrays):
    """w*h % 4 = 1, 2, 3 (17 357, 15 330, 15 315 points): plain host columns, staged as they are, but the packed pass
    reads four points per 16-byte load and takes whole quads only: launch_frames asks (n & 3) == 0 of every frame - strided.  The counts end inside an input round of 8 192 points: the n_pts-1 clamp of the loads
    and the i0 + j < n_pts test drop the round's tail."""
    shape = (vrays, hrays, 33.2, 120.0)
    n = vrays * hrays
    assert n % 4 == {(17, 1021): 1, (15, 1022): 2, (15, 1021): 3}[(vrays, hrays)] and n % 8192 not in (0, 8191)
    ref, dev = make_area_pair(oracle, hip, shape=shape, max_batch=6)
    warm_scene, _, frames = scene_frames(DEFAULT_AREA, (0.0, 0.0), 6, shape=shape, scene_seed=5, seed0=70)
    warm_both(ref, dev, warm_scene, (0.0, 0.0), shape=shape)
    scans = [s.scan for s in frames]
    assert all(sd.x.size == n for sd in scans)
    three_views(ref, dev, scans, scans, np.stack([s.tf for s in frames]), "strided", f"A/n_mod4_{n % 4}", 3000, 2000)


@pytest.mark.parametrize("vrays,hrays,want", [(2, 2, "packed"), (2, 3, "strided")])
def test_smallest_sensors_hand_placed_points(oracle, hip, vrays, hrays, want):
    """n = 4: the packed pass's only quad is the cloud itself (the n_pts - 4 clamp is 0); n = 6: strided, a thread's 8 loads run
    past the cloud and are clamped to point 5.  Hand-placed points: a small object 3 m above the surveyed ground 12 m in front of
    the sensor (a far cluster: a detection per frame) and, where the sensor has six rays, one point in the exclude box and one
    outside the area - different per frame.  The object lies inside one 1 m brick of the area's lattice: the full clustering keeps
    5 hit-list words per voxel of the sensor and needs 14 per occupied brick, so a 4-point sensor carries one brick (two raise the
    retry status and the batch runs on the general kernels - seen on the GPU, with equal results)."""
    n = vrays * hrays
    ref, dev = make_area_pair(oracle, hip, shape=(vrays, hrays, 33.2, 120.0), max_batch=4)
    warm_scene = synth.make_scene(5, n_targets=0)
    ap = synth.apriori_points(warm_scene, 0.25)
    for d in (ref, dev):
        d.load_apriori(ap)
        synth.seed_ground(d)
        survey_free_space(d)
    scans, tfs = [], []
    for f in range(4):
        obj = [(12.1 + f, 1.1, -2.0), (12.4 + f, 1.1, -2.0), (12.1 + f, 1.4, -2.0), (12.4 + f, 1.4, -1.7)]  # four voxels of ONE brick
        rest = [(0.1, 0.1, 0.0), (500.0, 0.0, 0.0)]  # inside the exclude box, outside the area
        p = np.array(obj if n == 4 else obj + rest, dtype=f32)
        scans.append(ScanData(x=np.ascontiguousarray(p[:, 0]), y=np.ascontiguousarray(p[:, 1]), z=np.ascontiguousarray(p[:, 2]), width=hrays, height=vrays, stride_bytes=4))
        tfs.append(f32([[1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, 5.0]]))
    three_views(ref, dev, scans, scans, np.stack(tfs), want, f"A/smallest_{vrays}x{hrays}", 4, 3)


def _nudged(p, nudge):
    """every coordinate moved by `nudge` (-3..3) float32 steps"""
    for _ in range(3):
        up = np.nextafter(p, f32(1e9))
        dn = np.nextafter(p, f32(-1e9))
        p = np.where(nudge > 0, up, np.where(nudge < 0, dn, p))
        nudge = nudge - np.sign(nudge)
    return p


def boundary_frames(voxel_size, n, n_frames=6, seed=17, extent=(30.0, 30.0, 6.0), free_box=((-18, -25, -1.2), (40, 30, 8)), floating=0):
    """the generator of test_single_pass_input_points_on_cell_boundaries (test_gpu_bench_shape.py): cell corners of a lattice
    shifted per frame, nudged by -3..3 ulps and tiny offsets; a fifth of the points anywhere.  world = sensor frame.
    `floating`: so many of the points, at indices spread over the frame, form a small object 4 m above the block instead - corners of
    3 x 3 x 3 cells of the same shifted lattice, nudged by -3..3 ulps as the others: a far cluster of fragile points that is not
    connected to the ground, a detection."""
    rng = np.random.default_rng(seed)
    vs = f32(voxel_size)
    out = []
    for f in range(n_frames):
        base = f32([-15.0 + 3.1 * f, -20.0 + 1.7 * f, -1.0])
        k = np.stack([rng.integers(0, int(extent[0] / voxel_size), n), rng.integers(0, int(extent[1] / voxel_size), n), rng.integers(0, int(extent[2] / voxel_size), n)], axis=1)
        p = (base + k.astype(f32) * vs).astype(f32)
        p = _nudged(p, rng.integers(-3, 4, (n, 3)))
        tiny = rng.choice(f32([0, 0, 1e-6, -1e-6, 1e-5, -1e-5, 3e-4, -3e-4, 0.01]), (n, 3))
        p = (p + tiny).astype(f32)
        free = rng.random(n) < 0.2
        lo_f = base if free_box is None else f32(free_box[0])
        hi_f = base + f32(extent) if free_box is None else f32(free_box[1])
        p[free] = rng.uniform(lo_f, hi_f, (int(free.sum()), 3)).astype(f32)
        if floating:
            at = rng.choice(n, floating, replace=False)
            corner = (base + f32([extent[0] / 2, extent[1] / 2, extent[2] + 4.0])).astype(f32)
            p[at] = _nudged((corner + rng.integers(0, 3, (floating, 3)).astype(f32) * vs).astype(f32), rng.integers(-3, 4, (floating, 3)))
        out.append(p)
    return out


def in_band(q, rl):
    """per point: some axis of the reference-lattice expression (q - off) * inv lies within eps of a cell boundary - the kernel's
    `fragile` (max |fr - 0.5| > 0.5 - eps), in host float32 arithmetic"""
    t = ((q.astype(f32) - rl["off"]) * rl["inv"]).astype(f32)
    g = np.abs((t - (np.floor(t) + f32(0.5))).astype(f32))
    return g.max(axis=1) > f32(f32(0.5) - f32(rl["eps"]))


def survivors(p, tf, area, exclude=True, dev=None):
    """world points (float32, the se3 association of the kernels) and the mask of the points both crops keep"""
    p = p.astype(f32)
    q = np.stack([(tf[r, 0] * p[:, 0] + (tf[r, 1] * p[:, 1] + (tf[r, 2] * p[:, 2] + tf[r, 3]).astype(f32)).astype(f32)).astype(f32) for r in range(3)], axis=1)
    lo, hi = area_bounds(*area)
    keep = ((q >= lo) & (q <= hi)).all(axis=1)
    if exclude and dev is not None:
        sp = dev.sp
        ec = f32([sp.exclude_offset[0], sp.exclude_offset[1], f32(sp.exclude_offset[2]) + f32(sp.exclude_size[2]) / f32(2)])
        half = f32([sp.exclude_size[0], sp.exclude_size[1], sp.exclude_size[2]]) / f32(2)
        keep &= ~((p >= ec - half) & (p <= ec + half)).all(axis=1)
    return q, keep


@pytest.mark.parametrize("variant,layout", [("wide", "aos48"), ("compact", "aos48"), ("compact", "columns")])
def test_frames_full_of_fragile_points(default_case, variant, layout):
    """frames of points a few ulps around cell boundaries at stride 48: most of a thread's 8 consecutive points are fragile, the
    first leaves from registers, every further one is loaded again at a.stride (kernels_frame.h, the `rest` loop; as plain columns:
    the packed pass's re-load at stride 4).
    wide: the generator of test_single_pass_input_points_on_cell_boundaries as it is.  Its frames occupy more bricks than the LDS
    clustering takes (LB_MAX; counted below on the host), so the strided frame kernel runs its input pass, raises the retry status
    and the batch is run again on the general kernels - the result compared is theirs.  compact: the same points inside
    16 x 16 x 4 m, ~1 400 bricks: the frame kernel's own output is compared (no k_bbox).  That block is one cluster on the ground
    and no detection, so 64 of its points form a small object of boundary points 4 m above it: a detection per frame, classified
    and reported from fragile points alone.  (wide: its free points give hundreds of detections.)"""
    ref, dev, _ = default_case
    h, w = OS1_16[:2]
    n = h * w
    pts = boundary_frames(0.25, n) if variant == "wide" else boundary_frames(0.25, n, extent=(16.0, 16.0, 4.0), free_box=None, floating=64)
    rl = ref_lattice(*DEFAULT_AREA, 0.25)
    tf = f32([[1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, 0.0]])
    shares, groups, bricks = [], 0, []
    for p in pts:
        q, keep = survivors(p, tf, DEFAULT_AREA, dev=dev)
        frag = keep & in_band(q, rl)
        shares.append(frag.sum() / max(keep.sum(), 1))
        groups += int((frag.reshape(-1, 8).sum(axis=1) >= 2).sum())  # a thread's 8 consecutive input indices
        k = np.floor(((q[keep] - rl["off"]) * rl["inv"]).astype(f32)).astype(np.int64)
        bricks.append(len(np.unique(k // 4, axis=0)))
    print(f"A/fragile_{layout}_{variant}: fragile share per frame {np.round(shares, 3).tolist()}, groups of 8 with two or more fragile points {groups}, bricks {bricks}")
    assert min(shares) > 0.6  # the generator puts four fifths of the points on boundaries
    assert groups >= 1000  # (one would do: nearly every one of the 6 x 2 048 groups has several)
    lb_max = capacities()["LB_MAX"]
    overflow = min(bricks) > lb_max + 200  # (+-200: a fragile point may land in the neighbouring brick)
    assert overflow if variant == "wide" else max(bricks) < lb_max - 200, bricks

    class S:  # (lay_aos48 / host_scan read these)
        pass

    frames = []
    for p in pts:
        s = S()
        s.x, s.y, s.z, s.intensity, s.range = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), None, None
        s.scan = ScanData(x=s.x, y=s.y, z=s.z, width=w, height=h, stride_bytes=4)
        frames.append(s)
    scans_dev = [host_scan(s, lay_aos48(s) if layout == "aos48" else lay_columns(s)) for s in frames]
    tfs = np.stack([tf] * len(frames))
    three_views(ref, dev, [s.scan for s in frames], scans_dev, tfs, "strided" if layout == "aos48" else "packed", f"A/fragile_{layout}_{variant}", 8000, 2000, expect_far=False, clusters_cap=16384, rerun_ok=overflow)


def test_bench_shape_32_frames_os1_128_at_stride_48(oracle, hip):
    """the nodelet's layout at the benchmarked shape: 32 OS1-128 frames of the bench scene as 48-byte structs"""
    F = 32
    shape = synth.SENSORS["os1-128"]
    ref, dev = make_area_pair(oracle, hip, shape=shape, max_batch=F)
    warm_scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=0)
    scene = synth.make_scene(synth.BENCH_SCENE_SEED, n_targets=12)
    warm_both(ref, dev, warm_scene, (0.0, 0.0), shape="os1-128", n_scans=4, seed0=synth.BENCH_WARM_SEED0)
    frames = synth.bench_frames(scene, "os1-128", F)
    scans_dev = [host_scan(s, lay_aos48(s)) for s in frames]
    three_views(ref, dev, [s.scan for s in frames], scans_dev, np.stack([s.tf for s in frames]), "strided", "A/bench_os1_128_aos48", 30_000, 8_000, expect_far=False)


# ------------------------------------------------------------------------------------------------ C. every row on the GPU
def filled_frames(area, vs, n, n_frames, dev, seed=11):
    """points spread over the whole operation area in world coordinates (identity transform): 2 500 uniform ones, points in the
    first and in the last cell of every axis, the eight corners of the area, the rest in four dense blobs (few occupied bricks:
    the frames stay within the LDS clustering's LB_MAX bricks, or the batch would leave the frame kernel)"""
    rng = np.random.default_rng(seed)
    lo, hi = area_bounds(*area)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    out = []
    for f in range(n_frames):
        uni = rng.uniform(lo64, hi64, (2500, 3))
        edge = []
        for a in range(3):
            for end in (0, 1):
                e = rng.uniform(lo64, hi64, (8, 3))
                e[:, a] = lo64[a] + rng.uniform(0.01, 0.2, 8) * vs if end == 0 else hi64[a] - rng.uniform(0.01, 0.2, 8) * vs
                edge.append(e)
        corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], dtype=np.float64)
        m = n - 2500 - 48 - 8
        centres = rng.uniform(lo64 + 0.2 * (hi64 - lo64), hi64 - 0.2 * (hi64 - lo64), (4, 3))
        blobs = np.clip(centres[rng.integers(0, 4, m)] + rng.normal(0.0, 0.8, (m, 3)), lo64, hi64)
        p = np.concatenate([uni, np.concatenate(edge), corners, blobs]).astype(f32)
        p = np.clip(p, lo, hi)  # (float32 rounding of a coordinate next to a face)
        p = p[rng.permutation(n)]
        out.append(p)
    return out


def run_row(oracle, hip, row, n_frames=4):
    off, size, vs, dims, _, _, fails, sensor_xy, z = TABLE[row]
    area = (tuple(map(float, off)), tuple(map(float, size)))
    sensor_xy = tuple(map(float, sensor_xy))
    cap = capacities()
    rl = ref_lattice(off, size, vs, cap)
    want = "general" if fails else "packed"
    ref, dev = make_area_pair(oracle, hip, area=area, vs=vs, max_batch=max(n_frames, 6))  # (the far rows hand over six adversarial frames)
    assert ref.map_size == dev.map_size
    warm_scene, _, frames = scene_frames(area, sensor_xy, n_frames, z=z)
    warm_both(ref, dev, warm_scene, sensor_xy, z=z)
    scans = [s.scan for s in frames]
    tfs = np.stack([s.tf for s in frames])
    three_views(ref, dev, scans, scans, tfs, want, f"C/{row}/scene", 500, 400)  # (the oracle's own output: 605 points / 540 voxels on the narrow long areas, 4 900 / 3 500 on the wide ones)
    # frames that reach both ends of every axis of the cell-code fields
    n = OS1_16[0] * OS1_16[1]
    # world coordinates handed over under an identity rotation.  Clusters further than classification__max_distance (50 m) from
    # the sensor are never reported, so on the areas kilometres away the sensor stands at the scene's sensor position and the
    # points are handed over relative to it: integer metres, so that fl(p + t) is the world point itself (asserted)
    t = f32([sensor_xy[0], sensor_xy[1], 0.0]) if row.startswith("far_") else f32([0.0, 0.0, 0.0])
    tf = np.concatenate([np.eye(3, dtype=f32), t[:, None]], axis=1).astype(f32)
    world = filled_frames(area, vs, n, n_frames, dev)
    pts = [(w.astype(np.float64) - t.astype(np.float64)).astype(f32) for w in world]
    for p, w in zip(pts, world):
        q, keep = survivors(p, tf, area, dev=dev)
        np.testing.assert_array_equal(q, w)
        k = np.floor(((q[keep] - rl["off"]) * rl["inv"]).astype(f32)).astype(np.int64)
        for a in range(3):
            assert k[:, a].max() >= dims[a] - 3 and k[:, a].min() <= 1, (row, a, k[:, a].min(), k[:, a].max(), dims)
        bricks = len(np.unique(k // 4, axis=0))
        assert bricks < cap["LB_MAX"] - 500, bricks  # (the fragile points' own-lattice cells may add a few bricks)
        assert keep.sum() > n - 200
    fscans = [ScanData(x=np.ascontiguousarray(p[:, 0]), y=np.ascontiguousarray(p[:, 1]), z=np.ascontiguousarray(p[:, 2]), width=OS1_16[1], height=OS1_16[0], stride_bytes=4) for p in pts]
    three_views(ref, dev, fscans, fscans, np.stack([tf] * n_frames), want, f"C/{row}/filled", n - 200, 2500, expect_far=False, clusters_cap=16384)
    return ref, dev, rl, frames


@pytest.mark.parametrize("row", [r for r in TABLE if not r.startswith("far_")])
def test_rows_of_the_geometry_table(oracle, hip, row):
    """"on" rows take the frame kernel (and never k_bbox: no frame overflows it), "off" rows the general kernels; scene frames
    and filled frames equal the oracle on both"""
    run_row(oracle, hip, row)


# ------------------------------------------------------------------------------------------------ D. far from the origin
def lattices_disagree(q, rl, area, vs):
    """per surviving world point: its cell in the frame's OWN lattice (the oracle's: offset from the frame's lowest point,
    oracle/algorithms.hpp) is not its cell in the reference lattice moved by the whole-cell shift between the two - host float32
    arithmetic.  These are the points the fragile route exists for: taken from the reference lattice they land in the wrong voxel."""
    lo, _ = area_bounds(*area)
    leaf = f32(vs)
    inv = f32(1) / leaf
    own = []
    for a in range(3):
        aco = f32(np.fmod(f32(f32(f32(0.5) * leaf) + lo[a] - leaf / f32(2)), leaf))
        aco = f32(aco + leaf) if aco < 0 else aco
        own.append(f32(f32(f32(np.floor(f32(q[:, a].min() * inv))) * leaf) - aco))
    own = np.array(own, dtype=f32)
    c_own = np.floor(((q - own) * inv).astype(f32)).astype(np.int64)
    c_ref = np.floor(((q - rl["off"]) * inv).astype(f32)).astype(np.int64)
    shift = np.rint((own.astype(np.float64) - rl["off"].astype(np.float64)) / vs).astype(np.int64)
    return ((c_own + shift) != c_ref).any(axis=1)


def adversarial_frames(area, vs, rl, sensor, n, n_frames, seed=23, floating=64, n_boundary=0):
    """Sensor-frame points under a pure translation `sensor` (float32): world = fl(x + t), ONE rounding.  Every point sits, on
    one, two or three axes, at a distance d in [0.8 eps, 1.25 eps] cells from a boundary of the reference lattice, on either
    side of it; its other axes lie mid-cell (0.2..0.8).  d < eps: fragile, re-encoded with the frame's own offset; d > eps:
    solid, its cell is the reference lattice's.  Uniform d: 4/9 of the near axes fall inside the band, so of the points with 1 / 2 /
    3 near axes 56 / 31 / 17 % are solid - a third of all points, two thirds fragile; the one rounding of x + t moves a point by at
    most 2^-12 m = 0.001 cells at 4 km, a twentieth of the interval's width.  Frame f fills a box of cells whose lower corner moves
    by (5, 3, 1) cells per frame: the frames' own lattices differ by non-multiples of 4 cells.  The box is one cluster on the
    ground; the last `floating` points, placed by the same rule in 3 x 3 x 3 cells 4 m above it and 6 m from the sensor, are an
    object of their own: a detection per frame, from points at the edge of the band.
    The last `n_boundary` frames put the near axes ON the boundary instead (d = 0), moved by -3..3 float32 steps of the world
    coordinate and by -3..3 steps of the sensor-frame coordinate (the finer of the two where the translation is small: z): the few
    ulps within which the reference lattice and a frame's own lattice really disagree (lattices_disagree) - eps is a bound with a
    margin, the points at its edge test the classification, these test that the fragile route gives the oracle's cell."""
    rng = np.random.default_rng(seed)
    eps = rl["eps"]
    off64 = rl["off"].astype(np.float64)
    t = f32(sensor)
    c0 = np.floor((t.astype(np.float64) - off64) / vs).astype(np.int64)  # the sensor's cell
    out = []
    for f in range(n_frames):
        lowc = c0 + np.array([-60 + 5 * f + 1, -50 + 3 * f + 2, -int(c0[2]) + 2 + f])
        k = lowc + np.stack([rng.integers(0, 120, n), rng.integers(0, 100, n), rng.integers(0, 30, n)], axis=1)
        if floating:
            k[-floating:] = c0 + np.array([20, 10, -int(c0[2]) + 50 + f]) + rng.integers(0, 3, (floating, 3))
        frac = rng.uniform(0.2, 0.8, (n, 3))
        n_near = rng.integers(1, 4, n)
        order = np.argsort(rng.random((n, 3)), axis=1)
        near = np.zeros((n, 3), dtype=bool)
        for j in range(3):
            near[np.arange(n), order[:, j]] |= j < n_near
        d = rng.uniform(0.8 * eps, 1.25 * eps, (n, 3))
        side = rng.random((n, 3)) < 0.5
        on_boundary = f >= n_frames - n_boundary
        frac = np.where(near, 0.0 if on_boundary else np.where(side, d, 1.0 - d), frac)
        world = off64 + (k + frac) * vs
        if on_boundary:
            world = np.where(near, _nudged(world.astype(f32), rng.integers(-3, 4, (n, 3))), world.astype(f32)).astype(np.float64)
            p = (world - t.astype(np.float64)).astype(f32)
            out.append(np.where(near, _nudged(p, rng.integers(-3, 4, (n, 3))), p).astype(f32))
        else:
            out.append((world - t.astype(np.float64)).astype(f32))
    return out


def run_far_row(oracle, hip, row):
    """scene frames and filled frames of the row (as C), the fragile share of the scene frames, then the adversarial frames"""
    off, size, vs, _, _, _, fails, sensor_xy, _ = TABLE[row]
    area = (tuple(map(float, off)), tuple(map(float, size)))
    ref, dev, rl, frames = run_row(oracle, hip, row)
    shares = []
    for s in frames:
        q, keep = survivors(np.stack([s.x, s.y, s.z], axis=1), s.tf, area, dev=dev)
        keep &= (np.stack([s.x, s.y, s.z], axis=1) != 0).any(axis=1)
        shares.append(float(in_band(q[keep], rl).mean()))
    print(f"D/{row}: eps {rl['eps']:.4f}, share of surviving points inside the eps band per frame {np.round(shares, 3).tolist()}")
    assert min(shares) >= 0.30, shares
    n = OS1_16[0] * OS1_16[1]
    sensor = f32([sensor_xy[0] + 0.5, sensor_xy[1] + 0.25, 3.0])
    pts = adversarial_frames(area, vs, rl, sensor, n, 6, n_boundary=2)
    tf = np.concatenate([np.eye(3, dtype=f32), sensor[:, None]], axis=1).astype(f32)
    for f, p in enumerate(pts):
        q, keep = survivors(p, tf, area, dev=dev)
        band = in_band(q[keep], rl)
        differ = lattices_disagree(q[keep], rl, area, vs)
        print(f"D/{row}/adversarial: frame {f}: inside the band {band.mean():.3f}, points whose own-lattice cell is not the reference lattice's {int(differ.sum())}")
        assert keep.sum() > 0.9 * n
        if f < 4:
            # floor: the generator alone gives 1/3 solid and 2/3 fragile (docstring of adversarial_frames); a quarter of each is asked
            assert band.mean() >= 0.25 and (~band).mean() >= 0.25, band.mean()
        else:
            # every point has a near axis within 3 + 3 steps of a boundary, far inside the band; and the frames hold points on
            # which the two lattices disagree (a step of z + 1.25 against a step of z + offset, or of x at 4 km: a few in a
            # thousand of 16 384 points; one would do, ten are asked)
            assert band.mean() >= 0.99 and differ.sum() >= 10, (band.mean(), differ.sum())
            assert not (differ & ~band).any()  # (no solid point may disagree: that would be the product's error bound broken)
        # the box of 120 x 100 x 30 cells starts at no multiple of 4 cells and spans up to 31 x 26 x 9 = 7 254 bricks, more than
        # LB_MAX: the 16 384 points leave a tenth of them empty.  Over LB_MAX the batch would leave the frame kernel (as C)
        k = np.floor(((q[keep] - rl["off"]) * rl["inv"]).astype(f32)).astype(np.int64)
        bricks = len(np.unique(k // 4, axis=0))
        assert bricks < capacities()["LB_MAX"] - 200, bricks  # (a fragile point's own-lattice cell may lie in the next brick)
    ascans = [ScanData(x=np.ascontiguousarray(p[:, 0]), y=np.ascontiguousarray(p[:, 1]), z=np.ascontiguousarray(p[:, 2]), width=OS1_16[1], height=OS1_16[0], stride_bytes=4) for p in pts]
    three_views(ref, dev, ascans, ascans, np.stack([tf] * len(pts)), "general" if fails else "packed", f"D/{row}/adversarial", int(0.9 * n), 5000, expect_far=False, clusters_cap=16384)


@pytest.mark.parametrize("row", ["far_3000", "far_4000", "far_5000"])
def test_areas_far_from_the_origin(oracle, hip, row):
    """eps 0.036 / 0.047: a third to a half of all surviving points are fragile (3 % on the default area); at 5 000 m eps passes
    0.05 and the same frames run on the general kernels.  Bit-equal weighted clouds, labels and far views on all three."""
    run_far_row(oracle, hip, row)
