/*
 * vofod.h — C-ABI drop-in boundary for VoFOD's per-scan point-cloud hot path.
 *
 * The reference (ctu-mrs/vofod) exposes no C/FFI interface: its only plugin
 * surface is the pluginlib nodelet vofod::VoFOD (nodelets.xml:1-5,
 * src/vofod_nodelet.cpp:141-145).  This header declares the seam a maintainer
 * would cut inside that nodelet: every entry point replaces the *body* of one
 * member function of vofod::VoFOD (cited per function as file:line, relative
 * to the reference tree).  INTEGRATION.md shows the ~60-line shim that calls
 * these from processMsg()/raycast_cloud()/updateSeparatedBGClusters().
 *
 * Two libraries implement exactly this interface:
 *   - libvofod_hip.so    (vofod_amd/csrc, symbols vofod_*)         the product:
 *                         hand-written gfx950 HIP kernels + C++ host driver.
 *   - libvofod_oracle.so (oracle/,        symbols vofod_oracle_*)  the checker:
 *                         CPU restatement of the reference algorithm; test
 *                         infrastructure only, never linked by the product.
 *
 * Conventions
 *   - plain pointers + sizes only; caller owns every in/out buffer, the handle
 *     owns device memory; nothing allocated on one side is freed on the other.
 *   - every function returns a vofod_status (0 = ok) and never throws.
 *   - a handle is thread-safe: calls are serialised on an internal mutex in the
 *     order m_voxels_mtx would order them (vofod_nodelet.cpp:712,943,1146,1210,1530).
 *   - transforms are float[12], row-major 3x4 [R|t] (Eigen::Affine3f s2w_tf,
 *     vofod_nodelet.cpp:913-922).
 */
#ifndef VOFOD_H
#define VOFOD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */

typedef enum vofod_status {
  VOFOD_OK = 0,
  VOFOD_ERR_INVALID_ARG = 1,
  VOFOD_ERR_SIZE_MISMATCH = 2,        /* cloud size != LUT size: vofod_nodelet.cpp:895-899, 1407-1411 */
  VOFOD_ERR_SENSOR_OUTSIDE_MAP = 3,   /* vofod_nodelet.cpp:1432, 1523-1526 (map left untouched by the DDA) */
  VOFOD_ERR_INDEX_OVERFLOW = 4,       /* voxel_grid_weighted.cpp:61-69 (output left empty) */
  VOFOD_ERR_CAPACITY = 5,             /* caller buffer too small; n_out holds the required size */
  VOFOD_ERR_DEVICE = 6,               /* HIP runtime error; see vofod_last_error_string */
  VOFOD_ERR_RAYCAST_NO_DETECTION = 7, /* no detection iteration since begin: vofod_nodelet.cpp:1531-1537 */
  VOFOD_ERR_RAYCAST_EMPTY = 8,        /* max raycast value is zero: vofod_nodelet.cpp:1542-1548 */
  VOFOD_ERR_PAUSED = 9,               /* raycast__pause / sepclusters__pause: :1400-1404, :1128-1132 */
  VOFOD_ERR_NOT_PENDING = 10,         /* *_finish without a matching *_begin */
  VOFOD_ERR_EMPTY = 11,               /* sepclusters: thresholded map cloud empty: :1155-1159 */
  VOFOD_ERR_MAP_RANGE = 12,           /* a weighted point fell outside the voxel map (vector::at would throw: voxel_map.cpp:116-117) */
  VOFOD_ERR_BUSY = 13,                /* a submitted batch (vofod_batch_submit) still reads the state this call would overwrite: collect it first */
  VOFOD_ERR_DELTA_BASE = 14           /* map delta: does not follow the snapshot last applied (replica) / no chain for the maps mask (owner) */
} vofod_status;

typedef struct vofod_handle vofod_handle;

/* ------------------------------------------------------------ parameters */

/* Static parameters: the block loaded once in onInit (vofod_nodelet.cpp:168-230)
 * plus the sensor description (initialize_sensor_rosparam :422-438).
 * Offsets' z components are the *bottom* of the box exactly as in the yaml
 * files; the library adds size_z/2 as :204 and :212 do. */
typedef struct vofod_static_params {
  float voxel_size;                         /* voxel_map/voxel_size            (detection_params.yaml:17) */
  float score_init;                         /* voxel_map/scores/init           (:21) */
  float background_sufficient_points_ratio; /* (:9), used as vofod_nodelet.cpp:228-230 */
  float oparea_offset[3];                   /* operation_area/offset (sim.yaml:8-11) */
  float oparea_size[3];                     /* operation_area/size   (sim.yaml:12-15) */
  float exclude_offset[3];                  /* exclude_box/offset    (detection_params.yaml:76-79) */
  float exclude_size[3];                    /* exclude_box/size      (:80-83) */
  int32_t sensor_hrays;                     /* sensor/horizontal_rays = cloud width  */
  int32_t sensor_vrays;                     /* sensor/vertical_rays   = cloud height */
  float sensor_vfov;                        /* sensor/vertical_fov_angle, radians */
  const float* lut_directions;              /* 3*w*h floats, xyz interleaved, index row*w+col (xyz_lut_t :77-81, :1447);
                                               NULL -> simulated LUT of initialize_sensor_lut_simulation :374-420 */
  const float* lut_offsets;                 /* same layout; NULL -> zeros (:416) */
  const uint8_t* mask;                      /* w*h bytes, non-zero = ray may be cast when range==0 (load_mask :506-560);
                                               NULL -> all ones (:558) */
  int32_t device;                           /* HIP device ordinal (ignored by the oracle) */
  int32_t max_batch_frames;                 /* frames a single vofod_process_batch call may carry (>=1) */
} vofod_static_params;

/* Dynamic parameters: one field per key of DetectionParams.cfg:16-44 (the
 * "__" spelling is dynamic_reconfigure's for "/").  May be changed between any
 * two calls, as m_drmgr_ptr->config may. */
typedef struct vofod_dyn_params {
  double ground_points_max_distance;
  double output__position_sigma;
  double voxel_map__scores__point;
  double voxel_map__scores__unknown;
  double voxel_map__scores__ray;
  double voxel_map__thresholds__apriori_map;
  double voxel_map__thresholds__new_obstacles;
  double voxel_map__thresholds__sure_obstacles;
  double voxel_map__thresholds__frontiers;
  int32_t classification__min_points;
  double classification__max_size;
  double classification__max_distance;
  double classification__max_explore_distance;
  int32_t raycast__pause;
  int32_t raycast__new_update_rule;
  double raycast__max_distance;
  double raycast__min_intensity;
  double raycast__weight_coefficient;
  int32_t sepclusters__pause;
  double sepclusters__max_bg_distance;
  int32_t sepclusters__min_sure_points;
} vofod_dyn_params;

/* Fills both structs with config/detection_params.yaml + config/apriori_maps/sim.yaml
 * + config/sensors/os1-128.yaml (the values the reference's simulation demo runs with). */
void vofod_default_params(vofod_static_params* sp, vofod_dyn_params* dp);

/* ------------------------------------------------------------------ types */

enum { VOFOD_MEM_HOST = 0, VOFOD_MEM_DEVICE = 1 };

/* One organised LiDAR scan: pcl::PointCloud<ouster_ros::Point> (types.h:7-8),
 * height = vrays, width = hrays (vofod_nodelet.cpp:1407).  Columns are given as
 * base pointer + common byte stride, so the 48-byte ouster_ros::Point AoS
 * (x at +0, y +4, z +8, intensity +16, range +36 in ouster_ros >= 0.10) and a
 * packed SoA (stride 4) both work without a copy on the caller's side. */
/* RANGE IMAGES.  A vofod_scan with x == y == z == NULL and range != NULL is a range image: what the sensor itself delivers,
 * width * height uint32 millimetres at stride_bytes, pixel i = row * width + col in the order of the handle's LUT
 * (vofod_static_params::lut_*), in either memspace.  The product library rebuilds the points on the device; the point of pixel i
 * is DEFINED as (every operation IEEE float32, each rounded once, no fused multiply-add)
 *     r    = float(range[i]) * 0.001f                          (uint32 -> float32 round-to-nearest-even, then one multiply)
 *     p[a] = (lut_directions[3i+a] * r) + lut_offsets[3i+a]     a = 0, 1, 2
 *     p    = (+0, +0, +0)  when range[i] == 0                   (what ouster_ros publishes for a pixel without a return)
 * - the sensor model check_sensor_params holds a cloud to (vofod_nodelet.cpp:1869-1917).  It is NOT bit-identical to the cloud
 * ouster_ros publishes: ouster_ros evaluates in double with the unnormalised LUT and casts afterwards; the two differ by about
 * one float32 ulp of the coordinate, far inside the 1e-3 of that check.
 * vofod_process_scan, vofod_process_batch and vofod_batch_submit accept range images (a batch may mix them with point scans);
 * `intensity` stays optional there and is still required by vofod_raycast_begin and VOFOD_SCAN_AUTO_RAYCAST.  Exactly one or two
 * of x, y, z NULL is VOFOD_ERR_INVALID_ARG, and so is all three NULL without `range`.  A device-resident range column needs a
 * base and a stride that are multiples of 4 bytes.  vofod_check_sensor_params compares points against the LUT and takes no
 * range image.  The CPU oracle has no range input: it returns VOFOD_ERR_INVALID_ARG for one. */
/* MOTION COMPENSATION.  A spinning sensor takes a whole period for one scan and delivers a timestamp per measurement column; a
 * range image may carry one pose per column, `col_tfs` (vofod_column_poses builds the table from two poses).  Pixel i = row * width
 * + col of the handle's LUT order was measured in column m = (col + shift_by_row[row]) mod width (vofod_set_column_shift; the mod is
 * mathematical, m in [0, width)), and the point of the pixel is DEFINED as (IEEE float32, each operation rounded once, nothing fused)
 *     r     = float(range[i]) * 0.001f
 *     q[a]  = (lut_directions[3i+a] * r) + lut_offsets[3i+a]                     (the definition above)
 *     p     = (+0, +0, +0)                          when range[i] == 0           (no pose applied: as above)
 *     p     = (qNaN, qNaN, qNaN), bits 0x7fc00000   when lo[a] <= q[a] <= hi[a] on all three axes, lo / hi = the bounds of the
 *                                                   exclude box as the first crop uses them (vofod_nodelet.cpp:626-629)
 *     p[k]  = T[k][0]*q[0] + (T[k][1]*q[1] + (T[k][2]*q[2] + T[k][3]))           otherwise, T = col_tfs[m]
 * - PCL's association, the one the pipeline's own transform uses.  The call's `tf` is applied afterwards by the unchanged pipeline;
 * the two matrices are never multiplied together.  The NaN rule keeps the airframe out: a return from the vehicle's own body lies
 * inside the exclude box in the frame of the instant it was measured, and after compensation it need not; both crops drop
 * non-finite points.  A return that enters the box only through the compensation is removed by the unchanged first crop.
 * vofod_process_scan, vofod_process_batch, vofod_batch_submit and vofod_range_to_points accept such scans (a batch may mix them with
 * plain range images and point scans); the caller may overwrite its pose tables when the call returns, as it may its scans.
 * vofod_raycast_begin and the raycast half of VOFOD_SCAN_AUTO_RAYCAST IGNORE col_tfs unless vofod_set_raycast_motion has switched
 * the compensated rays on (below): by default they cast the rigid rays the reference casts, from `range` and the LUT.  col_tfs on a
 * point scan (x, y, z given) is VOFOD_ERR_INVALID_ARG unless vofod_set_point_motion has switched it on (MOTION COMPENSATION OF POINT
 * SCANS below), and so is a device-resident table that is not 4-byte aligned.  sizeof(vofod_scan) is 80 (72 before the field): callers recompile; a zero-initialised scan
 * (`vofod_scan s{}`) is rigid.  The CPU oracle has no motion input: it rejects range images as before and ignores the field. */
/* MOTION COMPENSATION OF POINT SCANS.  With vofod_set_point_motion(h, 1) a point scan (x, y, z given: what the nodelet holds) may
 * carry col_tfs too, and the product library applies the poses on the device in front of the unchanged pipeline (k_point_deskew).
 * Pixel i = row * width + col was measured in column m = (col + shift_by_row[row]) mod width as above, T = col_tfs[m], q = (x[i],
 * y[i], z[i]) as given, and the point of the pixel is DEFINED as (IEEE float32, each operation rounded once, nothing fused; the rules
 * apply in this order)
 *     p     = (+0, +0, +0)                          when q[0] == 0 && q[1] == 0 && q[2] == 0  (either sign of zero: ouster_ros' "no
 *                                                   return"; no pose applied)
 *     p     = (qNaN, qNaN, qNaN), bits 0x7fc00000   when any q[a] is not finite
 *     p     = (qNaN, qNaN, qNaN)                    when lo[a] <= q[a] <= hi[a] on all three axes (the closed exclude box of the
 *                                                   first crop, as above)
 *     p[k]  = T[k][0]*q[0] + (T[k][1]*q[1] + (T[k][2]*q[2] + T[k][3]))           otherwise
 * The call's `tf` follows in the unchanged pipeline; the two matrices are never multiplied together.  The `range` and `intensity`
 * columns of the scan are not read by this step.  Fed the points vofod_range_to_points returns for a range image WITHOUT poses, this
 * definition yields bit for bit what MOTION COMPENSATION yields for that range image with the same table: a pixel without a return
 * decodes to (+0, +0, +0) and stays, every other q is the same float triple in both.
 * With the switch on vofod_process_scan, vofod_process_batch and vofod_batch_submit accept such scans (a batch may mix them with plain
 * point scans, plain range images and compensated range images); vofod_range_to_points stays range-image only.  With the switch off
 * (the state after vofod_create) every call behaves as before: col_tfs on a point scan is VOFOD_ERR_INVALID_ARG.  Device-resident
 * columns of such a scan are read in place and never written; their bases and their stride must be multiples of 4 bytes
 * (VOFOD_ERR_INVALID_ARG), the table 4-byte aligned as above.  The caller may overwrite scans and tables when the call returns.
 * VOFOD_SCAN_AUTO_RAYCAST on such a scan: the raycast half does what vofod_raycast_begin does with the same scan - rigid rays unless
 * vofod_set_raycast_motion is on, compensated rays from the same table when it is. */
/* MOTION-COMPENSATED RAYS.  With vofod_set_raycast_motion(h, 1) the raycast role casts the ray of every pixel of a scan that carries
 * col_tfs from that pixel's own pose.  For pixel i = row * width + col, with m = (col + shift_by_row[row]) mod width as above,
 * T = col_tfs[m], d = lut_directions[3i..] and o = lut_offsets[3i..] (zeros when the handle has none), the beam is DEFINED as (IEEE
 * float32, each operation rounded once, nothing fused)
 *     d'[k] = ((T[k][0]*d[0]) + (T[k][1]*d[1])) + (T[k][2]*d[2])
 *     o'[k] = (((T[k][0]*o[0]) + (T[k][1]*o[1])) + (T[k][2]*o[2])) + T[k][3]                 k = 0, 1, 2
 * and everything else is the rigid pass with d', o' in place of the LUT entries: dir = R d' and start = (R o') + t with the call's
 * `tf` in the same association, the intensity gate and the `!mask && range == 0` rule, length = range == 0 ? max_distance :
 * min(range * 0.001f - voxel_size, max_distance), the in-limits test of each ray's own start, VOFOD_ERR_SENSOR_OUTSIDE_MAP decided
 * by the origin of the call's `tf`, and the walk of VoxelMap::forEachRay with its running tmax.  The two matrices are never
 * multiplied together.  The association is the rigid pass's own, so an identity table gives d' == d and o' == o as values (a zero
 * may change its sign; the walk reads only the magnitude of a zero component and compares it) - the rigid rays.  No exclude-box rule
 * applies: the reference casts the airframe's short rays too, and length <= 0 stops them.  The rotation part of T is taken as
 * given: a T that is not orthonormal scales d' and with it the walk's parameter (lengths are then measured in units of |d'|).
 * The table lives in the scan's memspace; a device-resident table must be 4-byte aligned (VOFOD_ERR_INVALID_ARG).  With the switch on
 * vofod_raycast_begin accepts col_tfs on a point scan too - the role reads `range` and `intensity` only, and a caller that deskews
 * its own points still wants the rays; vofod_process_scan keeps rejecting col_tfs on point scans.  A scan without col_tfs, and any
 * scan while the switch is off, is cast rigidly exactly as before. */
/* EXACT RAYCAST ACCUMULATION.  With vofod_set_raycast_exact(h, 1) a raycast pass sums the in-voxel path lengths as fixed-point units
 * in uint32 instead of floats, in the raycast map's own buffer: the sum does not depend on the order in which the rays arrive, so two
 * passes of one scan - and the passes of two handles fed the same scans - end with the same bits.  The rays, their gates and their
 * walk are those of the pass the other switches select (rigid, or MOTION-COMPENSATED RAYS); only what is added changes.
 *   Scale.  S = log2(units per metre) is fixed per handle at vofod_create: the largest integer in [0, 24] with
 *             n_pixels * (floor(2 * vs * 2^S) + 1) <= 2^32 - 1,     n_pixels = sensor_hrays * sensor_vrays,
 *           vs = the float voxel_size widened to double, the rule evaluated in double on the host.  QMAX = floor(2 * vs * 2^S).
 *           (OS1-128 at 0.25 m: S = 15; at 0.5 m: 14; 128 x 2048 at 0.1 m: 16; OS1-16 at 0.5 m: 17; a sensor of a hundred pixels: 24.)
 *   Piece.  dd = the float min(dist, length) - prev of the walk's step (VoxelMap::forEachRay with its running tmax), unchanged.  Its
 *           units are q = min(rint(dd * 2^S), QMAX): the product is exact (2^S is a power of two), rint rounds to nearest, ties to
 *           even.  A piece with q == 0 leaves no trace.  The clamp can only bite when a pose table of the motion pass is not a
 *           rotation (the walk's parameter is then not metres): an in-voxel piece stays below sqrt(3) * vs plus the drift of tmax.
 *           It exists so that no voxel can overflow: every ray lays at most one piece into a voxel.
 *   Sum.    U[v] = the sum of q over the pieces laid into voxel v, as uint32: exact, independent of order and grouping.
 *   View.   r[v] = float(U[v]) * 2^-S: the uint32 -> float conversion rounds to nearest even, the scaling is exact.  While an exact
 *           pass is pending vofod_read_map(VOFOD_MAP_RAYCAST) returns r (converted in the caller's copy; the device keeps U), and
 *           vofod_raycast_finish sweeps with the same r, the old update rule's max_val being float(max U) * 2^-S.
 *           VOFOD_ERR_RAYCAST_EMPTY means that all of U is zero.
 * The representation belongs to the PASS: vofod_raycast_begin records the switch, vofod_raycast_finish sweeps what begin laid, and
 * VOFOD_SCAN_AUTO_RAYCAST inherits both.  While an exact pass is pending, vofod_write_map and vofod_voxels_as_pc on
 * VOFOD_MAP_RAYCAST return VOFOD_ERR_BUSY (the buffer holds units, not floats); vofod_map_shift refuses any pending pass already.
 * Units never outlive their pass: a vofod_raycast_finish that abandons an exact pass (VOFOD_ERR_RAYCAST_NO_DETECTION) clears the
 * raycast map to zeros, where an abandoned float pass leaves its lengths readable until the next begin; after
 * VOFOD_ERR_RAYCAST_EMPTY the map is zero in both.  So outside a pending exact pass vofod_read_map, vofod_voxels_as_pc and
 * vofod_map_export always see floats.
 * Snapshots: the raycast map's bits travel as they are; byte 0 of the header's 16 reserved bytes holds S + 1 when the snapshot
 * carries a pending exact pass with the raycast map in its mask, and 0 otherwise (such snapshots are byte for byte what they were).
 * vofod_map_apply adopts the pass's representation with the bits and returns VOFOD_ERR_SIZE_MISMATCH when S is not the applying
 * handle's own; the other 15 reserved bytes must be zero.  Against the float pass the view differs by at most 2^-(S+1) m per piece
 * (the rounding of q) plus the float pass's own summation error.  With the switch off every launch and every bit is as before. */
typedef struct vofod_scan {
  const void* x;          /* float */
  const void* y;          /* float */
  const void* z;          /* float */
  const void* intensity;  /* float    (raycast only: vofod_nodelet.cpp:1446); may be NULL for process_scan */
  const void* range;      /* uint32 mm (raycast only: :1449, :1455-1456);     may be NULL for process_scan */
  size_t stride_bytes;
  int32_t width, height;
  int32_t memspace;       /* VOFOD_MEM_HOST or VOFOD_MEM_DEVICE (device pointers on the handle's device) */
  double stamp;           /* seconds; carried through, not interpreted */
  const float* col_tfs;   /* NULL: the scan is rigid (everything as today).  Otherwise width * 12 floats in the scan's memspace:
                             col_tfs[12*m ..] is the row-major 3x4 [R|t] that takes a point from the sensor frame at the time of
                             measurement column m into the scan's reference sensor frame - the frame the call's `tf` starts from.
                             Range images, and point scans under vofod_set_point_motion; see MOTION COMPENSATION above */
} vofod_scan;

/* payload of vofod::PointXYZR (point_types.h:51-56): voxel centre + weight */
typedef struct vofod_point_xyzr {
  float x, y, z;
  uint32_t range;
} vofod_point_xyzr;

/* pcl::PointXYZI payload of the debug clouds (voxel_map.h pt_t) */
typedef struct vofod_point_xyzi {
  float x, y, z;
  float intensity;
} vofod_point_xyzi;

/* vofod/Detection (msgs/Detection.msg:1-12), filled as vofod_nodelet.cpp:972-985 */
typedef struct vofod_detection {
  uint32_t id;
  uint32_t frame;                /* index of the scan inside a batch (0 for process_scan) */
  uint64_t n_points;
  double confidence;
  double detection_probability;
  double position[3];
  double covariance[9];
} vofod_detection;

enum { VOFOD_CLASS_MAV = 0, VOFOD_CLASS_UNKNOWN = 1, VOFOD_CLASS_INVALID = 2, VOFOD_CLASS_NONE = -1 };

/* One Euclidean cluster of the weighted cloud.  Canonical order:
 * size descending (extract_clusters' reverse sort), ties by smallest member. */
typedef struct vofod_cluster_info {
  uint32_t first_member;   /* smallest member index into the weighted cloud == label */
  uint32_t n_points;
  int32_t is_close;        /* findCloseFarClusters: vofod_nodelet.cpp:727-748 */
  int32_t cclass;          /* classify_cluster :1648-1730; VOFOD_CLASS_NONE for close clusters */
  float aabb_min[3];
  float aabb_max[3];
  float obb_center[3];     /* NaN when not evaluated */
  float obb_size;
} vofod_cluster_info;

/* Optional per-scan debug/parity outputs; every array is caller-allocated. */
typedef struct vofod_scan_debug {
  vofod_point_xyzr* weighted;   /* cloud_weighted of filterAndTransform :659-668 */
  uint32_t* labels;             /* per weighted point: label (= first_member of its cluster) */
  size_t weighted_cap;
  size_t n_weighted;
  vofod_cluster_info* clusters;
  size_t clusters_cap;
  size_t n_clusters;
  uint64_t n_input_after_crop;  /* points entering VoxelGridWeighted (:657) */
  uint64_t n_bg_voxels;         /* nVoxelsOver(new_obstacles) :715 */
  int32_t background_pts_sufficient;
  int32_t sure_background_sufficient;
  /* host wall-clock per stage, ms, reference ScopeTimer names (:924-964):
   * [0] filtering [1] clusterization [2] close X far [3] vmap update [4] classification */
  double stage_ms[8];
  /* INPUT, batches only (read from dbg[0]): non-zero asks for the view of the production path of a read-only batch, which
   * clusters close first - only far clusters are ever used (:727-748, :946-963): `clusters` lists the far clusters only
   * (is_close = 0, canonical order) and `labels` is VOFOD_LABEL_NONE for every voxel outside them.
   * The struct carries inputs (the buffers, their capacities and this field): ZERO-INITIALISE it (`vofod_scan_debug d = {0}`)
   * before filling in what is wanted - garbage here silently switches the view. */
  int32_t far_only;
  int32_t reserved_;
} vofod_scan_debug;
#define VOFOD_LABEL_NONE 0xffffffffu

typedef struct vofod_status_info {
  int32_t detection_its;               /* m_detection_its */
  uint32_t last_detection_id;          /* m_last_detection_id */
  int32_t background_pts_sufficient;   /* m_background_pts_sufficient */
  int32_t sure_background_sufficient;  /* m_sure_background_sufficient */
  int32_t raycast_pending;             /* m_raycast_running */
  int32_t map_size[3];                 /* VoxelMap::sizesIdx */
  float map_offset[3];                 /* VoxelMap::origin */
} vofod_status_info;

enum { VOFOD_MAP_VOXELS = 0, VOFOD_MAP_FLAGS = 1, VOFOD_MAP_RAYCAST = 2 };

/* process_scan flags */
enum {
  VOFOD_SCAN_DEFAULT = 0,
  VOFOD_SCAN_NO_MAP_UPDATE = 1,  /* read-only map: skip updateVMaps/++its and keep exploreToGround's
                                    frontier writes in a per-scan overlay (batched mode) */
  VOFOD_SCAN_AUTO_RAYCAST = 2    /* emulate the detached raycast thread :951-957 deterministically: after ++its EITHER
                                    finish the pending raycast OR (none pending) begin one for this scan - as in the
                                    reference, where a new thread starts only when none runs, a pass covers every other scan */
};

/* --------------------------------------------------------------- lifecycle */

/* onInit parameter block :168-230 + reset() :1610-1632.  Allocates the three
 * voxel maps (m_voxel_map := score_init, m_voxel_flags := 0, m_voxel_raycast := 0). */
int vofod_create(const vofod_static_params* sp, const vofod_dyn_params* dp, vofod_handle** out);
void vofod_destroy(vofod_handle* h);
/* reset() :1610-1632 (also re-zeroes the latches like onInit :283-284 and the detection id :296) */
int vofod_reset(vofod_handle* h);
int vofod_set_dynamic_params(vofod_handle* h, const vofod_dyn_params* dp);
const char* vofod_last_error_string(vofod_handle* h);
int vofod_get_status(vofod_handle* h, vofod_status_info* out);

/* initialize_apriori_map :339-345: every point inside the map limits sets its
 * voxel to +inf; both background latches are set.  xyz interleaved, world frame,
 * already transformed/downsampled by the caller (rows N2 of SURVEY 8f). */
int vofod_load_apriori(vofod_handle* h, const float* xyz, size_t n);

/* The whole of initialize_apriori_map (:214-226, :306-345) from a point-cloud file (row N2 of SURVEY 8f): load_cloud
 * -> rigid transform (apriori_map/tf/{x,y,z,yaw} + sim_correction) -> stock pcl::VoxelGrid centroid filter at the map's
 * voxel size -> vofod_load_apriori.  Init-time host work in the reference and here. */
int vofod_ingest_apriori(vofod_handle* h, const char* filename, const float tf_xyz[3], double yaw_deg, const float sim_correction[3],
                         size_t* n_loaded, size_t* n_voxels);

/* VoxelMap::voxelsAsPC (voxel_map.cpp:157-183): the voxels with ((value > threshold) == greater_than) of map `which` as
 * world-frame centres + value, in the reference's order (x outer, y, z inner).  The nodelet's debug clouds
 * (vofod_nodelet.cpp:999-1013): background = (VOFOD_MAP_VOXELS, new_obstacles, 1), sure air = (VOFOD_MAP_VOXELS, frontiers, 0).
 * VOFOD_ERR_CAPACITY: *n_out holds the required number of points. */
int vofod_voxels_as_pc(vofod_handle* h, int which, float threshold, int greater_than, vofod_point_xyzi* out, size_t cap, size_t* n_out);

/* processMsg(sensor_msgs::Range) :581-613 (row N4 of SURVEY 8f): the height range-finder marks the voxel it hits as
 * background-ish: p = tf * (range, 0, 0); if inLimits(p): map(p) = (map(p) + voxel_map/scores/point) / 2.0.
 * The reference's validity test `range <= min_range && range >= max_range` is kept as written.
 * Returns VOFOD_ERR_MAP_RANGE when the point is outside the operation area (map untouched). */
int vofod_update_ground(vofod_handle* h, float range, float min_range, float max_range, const float tf[12]);

/* test/visualisation access to the three maps (x-fastest, idx = ix + iy*sx + iz*sx*sy: voxel_map.cpp:81) */
int vofod_read_map(vofod_handle* h, int which, float* dst, size_t n);
int vofod_write_map(vofod_handle* h, int which, const float* src, size_t n);

/* ---------------------------------------------------------------- hot path */

/* Body of processMsg(pc_t::ConstPtr,int) between :926 and :965:
 * filterAndTransform :621-684 -> clusterCloud :689-698 -> findCloseFarClusters :703-750
 * -> updateVMaps :943-950 -> classifyClusters :819-830 -> extractDetections :834-879. */
int vofod_process_scan(vofod_handle* h, const vofod_scan* scan, const float tf[12], int flags,
                       vofod_detection* out, size_t cap, size_t* n_out, vofod_scan_debug* dbg);

/* Batched mode (new): n independent scans against the handle's current map,
 * each with VOFOD_SCAN_NO_MAP_UPDATE semantics.  Detections of all frames are appended to
 * `out` in frame order, `n_out_per_frame[f]` counts them.  dbg: NULL or an array of n. */
int vofod_process_batch(vofod_handle* h, const vofod_scan* scans, const float* tfs, size_t n,
                        vofod_detection* out, size_t cap, uint32_t* n_out_per_frame, size_t* n_out,
                        vofod_scan_debug* dbg);

/* The same, pipelined: submit enqueues the kernels of a batch and returns a ticket (0..7; at most eight batches in flight:
 * streaming kernels, frame kernels and classification tails of consecutive batches run as a three-stage pipeline on the
 * device; batches of fewer than 128 frames run side by side on streams of their own, tails included - see INTEGRATION.md on GPU_MAX_HW_QUEUES), collect waits for it and returns the detections.  Submitting batch k+1 (and k+2) before collecting batch k keeps
 * the pipeline full.  Read-only map only (VOFOD_SCAN_NO_MAP_UPDATE semantics); collect in submit order for deterministic
 * detection ids.  The scans' host buffers need not outlive submit.  collect with an `out` too small for the batch returns
 * VOFOD_ERR_CAPACITY with *n_out = the detections to make room for; the ticket then stays pending and no ids are handed out
 * (batches of >= 4 frames; a batch that had to take the host tail is consumed by the failing call). */
int vofod_batch_submit(vofod_handle* h, const vofod_scan* scans, const float* tfs, size_t n, int* ticket);
/* Allocates now what the first `tickets` (1..8) batches in flight would otherwise allocate inside their first
 * vofod_batch_submit (workspaces of max_batch_frames slots, flood-fill buffers of the device tail: hundreds of ms of
 * allocation in a real-time caller's first calls).  Optional; the reference has no counterpart (its buffers are
 * std::vectors grown on use). */
int vofod_reserve(vofod_handle* h, int tickets);
int vofod_batch_collect(vofod_handle* h, int ticket, vofod_detection* out, size_t cap, uint32_t* n_out_per_frame, size_t* n_out);

/* raycast_cloud :1397-1605 split where the reference thread blocks on m_detection_cv (:1530-1537):
 *   begin  = guards :1400-1423, start_detection_its :1425, clear + DDA accumulation :1430-1492
 *   finish = detection_its_diff :1539, max :1542, update sweep :1550-1601, flags clear :1602 */
int vofod_raycast_begin(vofod_handle* h, const vofod_scan* scan, const float tf[12]);
int vofod_raycast_finish(vofod_handle* h);

/* updateSeparatedBGClusters :1126-1277 split at the second lock (:1210):
 *   begin  = snapshot :1146-1150, voxelsAsVoxelPC :1153, VoxelGridCounted :1162-1167,
 *            clusterCloud :1171, sure counts :1175-1183, latch :1188-1206
 *   finish = detection_its_diff :1212, stencil :1219-1237, erase :1239-1272
 * `sure_background_sufficient` (nullable) receives the latch. */
int vofod_sepclusters_begin(vofod_handle* h, int* sure_background_sufficient);
int vofod_sepclusters_finish(vofod_handle* h);

/* --------------------------------------------- stateless L4 entry points */

typedef struct vofod_cloud_view {
  const void* x; const void* y; const void* z;
  const void* intensity;   /* VoxelGridCounted only */
  size_t stride_bytes;
  size_t n;
  int32_t memspace;
} vofod_cloud_view;

/* Lattice of a voxel-grid output: centre = (ijk + 0.5) * leaf + offset,
 * key = i + j*div[0] + k*div[0]*div[1] (voxel_grid_weighted.cpp:109-113,136,178-180) */
typedef struct vofod_grid_desc {
  float leaf[3];
  float offset[3];
  int32_t min_b[3];
  int32_t div_b[3];
} vofod_grid_desc;

/* VoxelGridWeighted::filter (voxel_grid_weighted.cpp:28-190).  align != 0 reproduces
 * setVoxelAlign(align_center) :22-26.  keys (nullable) receives each output voxel's key. */
int vofod_voxel_grid_weighted(vofod_handle* h, const vofod_cloud_view* in, float leaf,
                              int align, const float align_center[3],
                              vofod_point_xyzr* out, uint32_t* keys, size_t cap, size_t* n_out,
                              vofod_grid_desc* grid);

/* VoxelGridCounted::filter (voxel_grid_counted.cpp:36-196), including the positional
 * count range of :185-187. */
int vofod_voxel_grid_counted(vofod_handle* h, const vofod_cloud_view* in, float leaf, float threshold,
                             vofod_point_xyzr* out, uint32_t* keys, size_t cap, size_t* n_out,
                             vofod_grid_desc* grid);

/* clusterCloud (vofod_nodelet.cpp:689-698) on a voxel-grid output.  labels[i] = smallest
 * member index of i's cluster.  keys/grid describe the lattice the points sit on (the HIP
 * implementation clusters on the lattice; the oracle ignores them and uses the coordinates). */
int vofod_cluster(vofod_handle* h, const vofod_point_xyzr* pts, const uint32_t* keys,
                  const vofod_grid_desc* grid, size_t n, float tolerance,
                  uint32_t* labels, size_t* n_clusters);

/* load_cloud (pc_loader.cpp:17-90): whitespace-separated "x y z" text (".pts": count on the
 * first line).  xyz interleaved; returns VOFOD_ERR_CAPACITY with *n_out = required points. */
int vofod_load_cloud(const char* filename, float* xyz, size_t cap, size_t* n_out);

/* simulated sensor LUT of initialize_sensor_lut_simulation (vofod_nodelet.cpp:374-420) */
int vofod_sim_lut(int32_t w, int32_t h, float vfov, float* directions /* 3*w*h */);

/* initialize_sensor_lut (vofod_nodelet.cpp:358-372) from the Ouster metadata (row N1 of SURVEY 8f): [3P] ouster::make_xyz_lut
 * restated, then cast to float and directions normalised.  tf16 = lidar_to_sensor_transform, row-major 4x4, NULL = identity;
 * azimuth / altitude: beam angles in degrees, one per row.  Output layout as vofod_static_params::lut_*. */
int vofod_ouster_lut(int32_t w, int32_t h, double range_unit, double lidar_origin_to_beam_origin_mm, const double* tf16,
                     const double* azimuth_deg, const double* altitude_deg, float* directions /* 3*w*h */, float* offsets /* 3*w*h */);

/* load_mask (:506-560) after the image is decoded: plain copy or "mangling" into the packets' staggered column-major order
 * (:527-541, pixel_shift_by_row from the metadata, NULL = zeros); image NULL = no usable file -> all ones (:558). */
int vofod_mask_layout(const uint8_t* image /* w*h, row-major */, int32_t w, int32_t h, const int32_t* pixel_shift_by_row /* h */,
                      int32_t mangle, uint8_t* mask /* w*h */);

/* check_sensor_params (vofod_nodelet.cpp:1869-1917): the first valid pixel (mask set, range != 0; rows outer) of an organised
 * host-resident cloud against the sensor model: direction of (point - beam offset) vs the LUT direction, its length vs
 * range * 0.001 m, unit length of the LUT direction, each within 1e-3.  *checked (nullable) = a valid pixel was found
 * (m_sensor_params_checked).  VOFOD_OK: the parameters fit or nothing could be checked; VOFOD_ERR_SIZE_MISMATCH: they do not
 * (m_sensor_params_ok = false: the nodelet then refuses to raycast, :1413-1418).  lut_offsets and mask may be NULL. */
int vofod_check_sensor_params(const vofod_scan* scan, const float* lut_directions /* 3*w*h */, const float* lut_offsets /* 3*w*h */, const uint8_t* mask /* w*h */,
                              int32_t* checked);

/* ------------------------------------------------------------ diagnostics */

/* Per-kernel device time, measured with HIP events on the handle's own stream (the reference analogue is
 * mrs_lib::ScopeTimer, vofod_nodelet.cpp:887,1135,1426).  While enabled every kernel launch is bracketed by
 * two events; vofod_profile_read drains them: names[64*i..] = kernel name, ms[i] = summed time, calls[i] =
 * launches.  Returns the number of distinct kernels.  No-ops in the oracle. */
int vofod_profile_enable(vofod_handle* h, int on);
size_t vofod_profile_read(vofod_handle* h, char* names, double* ms, uint64_t* calls, size_t cap);

/* ------------------------------------------------- outgoing messages (product library only)
 *
 * The nodelet's publications in the ROS 1 wire format (little endian; strings / arrays carry a uint32 length; a
 * std_msgs/Header is seq, stamp.sec, stamp.nsec, frame_id), for hosts without ROS: vofod/Detections
 * (msgs/Detections.msg + Detection.msg:1-12, vofod_nodelet.cpp:968-988), vofod/Status (msgs/Status.msg, :1379-1385),
 * vofod/ProfilingInfo (msgs/ProfilingInfo.msg, :2178-2201; event_type 1 = start, 2 = end).  buf may be NULL to ask for the
 * size; VOFOD_ERR_CAPACITY when cap is too small (*n_bytes = bytes needed). */
typedef struct vofod_msg_header {
  uint32_t seq;
  uint32_t stamp_sec, stamp_nsec;
  const char* frame_id; /* world frame (m_world_frame_id) */
} vofod_msg_header;
int vofod_serialize_detections(const vofod_msg_header* header, const vofod_detection* dets, size_t n, uint8_t* buf, size_t cap, size_t* n_bytes);
int vofod_serialize_status(const vofod_msg_header* header, int detection_enabled, int detection_active, uint8_t* buf, size_t cap, size_t* n_bytes);
int vofod_serialize_profiling_info(uint32_t stamp_sec, uint32_t stamp_nsec, uint32_t routine_id, uint64_t event_sequence, uint8_t event_type, uint8_t* buf, size_t cap,
                                   size_t* n_bytes);

/* ------------------------------------------------- range images (product library only)
 *
 * The points of a range image (see vofod_scan) as the hot path sees them: decoded on the device with the handle's LUT by the
 * kernel the per-scan entry points use (k_range_decode), into three packed columns of width * height floats in `out_memspace`
 * (VOFOD_MEM_HOST or VOFOD_MEM_DEVICE).  For debug clouds and for holding the kernel to the definition.
 * VOFOD_ERR_INVALID_ARG: `scan` is no range image; VOFOD_ERR_SIZE_MISMATCH: its width or height differ from the handle's. */
int vofod_range_to_points(vofod_handle* h, const vofod_scan* scan, float* x, float* y, float* z, int32_t out_memspace);

/* ------------------------------------------------- motion compensation of range images (product library only)
 *
 * See MOTION COMPENSATION at vofod_scan.  With scan->col_tfs vofod_range_to_points returns the compensated cloud, decoded by the
 * kernel the per-scan entry points use for such scans (k_range_decode_motion).
 *
 * vofod_set_column_shift: a sensor property, set once after vofod_create.  Pixel (row, col) of the handle's LUT order was measured
 * in column m = (col + shift_by_row[row]) mod width; any int32 shift is legal.  shift_by_row: sensor_vrays ints, NULL = zeros (the
 * state after vofod_create).  This is the direction of the reference's mask mangling (vofod_nodelet.cpp:537) for a DESTAGGERED
 * image - pixel_shift_by_row of the sensor's metadata; a staggered image (columns are measurement columns) needs zeros.  Kept
 * across vofod_reset, vofod_map_apply and vofod_map_shift.  VOFOD_ERR_BUSY while a submitted batch is pending. */
int vofod_set_column_shift(vofod_handle* h, const int32_t* shift_by_row /* height ints; NULL = zeros */);
/* vofod_set_raycast_motion: a handle property like the column shifts; `on` is taken as on != 0.  Off after vofod_create: the raycast
 * role ignores col_tfs.  On: vofod_raycast_begin and the raycast half of VOFOD_SCAN_AUTO_RAYCAST cast a scan that carries col_tfs
 * ray by ray from the columns' poses (MOTION-COMPENSATED RAYS at vofod_scan; profiled as k_raycast_motion).  Kept across vofod_reset,
 * vofod_map_apply and vofod_map_shift.  VOFOD_ERR_BUSY while a submitted batch or a raycast pass is pending. */
int vofod_set_raycast_motion(vofod_handle* h, int on);
/* vofod_set_point_motion: a handle property like the column shifts; `on` is taken as on != 0.  Off after vofod_create: col_tfs on a
 * point scan is VOFOD_ERR_INVALID_ARG.  On: vofod_process_scan, vofod_process_batch and vofod_batch_submit compensate such scans on the
 * device (MOTION COMPENSATION OF POINT SCANS at vofod_scan; profiled as k_point_deskew, one launch per batch that holds such frames).
 * Kept across vofod_reset, vofod_map_apply and vofod_map_shift.  VOFOD_ERR_BUSY while a submitted batch is pending. */
int vofod_set_point_motion(vofod_handle* h, int on);
/* vofod_deskew_points: the compensated cloud of ONE point scan with col_tfs as the hot path sees it - the counterpart of
 * vofod_range_to_points: three packed columns of width * height floats in `out_memspace`, computed by the kernel and through the
 * staging the per-scan entry points use (frame slot 0 of the synchronous workspace).  Needs no switch.  For debug clouds and for
 * holding the kernel to the definition.  VOFOD_ERR_INVALID_ARG: a range image, a scan without col_tfs, a device-resident table that
 * is not 4-byte aligned, device-resident columns whose base or stride is no multiple of 4; VOFOD_ERR_SIZE_MISMATCH: width or height
 * differ from the handle's; VOFOD_ERR_BUSY while ticket 0 is pending. */
int vofod_deskew_points(vofod_handle* h, const vofod_scan* scan, float* x, float* y, float* z, int32_t out_memspace);
/* vofod_set_raycast_exact: a handle property with the rules of vofod_set_raycast_motion; `on` is taken as on != 0.  Off after
 * vofod_create: raycast passes sum floats.  On: the passes vofod_raycast_begin and VOFOD_SCAN_AUTO_RAYCAST begin from now on sum
 * fixed-point units (EXACT RAYCAST ACCUMULATION at vofod_scan; profiled as k_raycast_exact, k_ray_sweep_exact).  Kept across vofod_reset,
 * vofod_map_apply and vofod_map_shift.  VOFOD_ERR_BUSY while a submitted batch or a raycast pass is pending;
 * VOFOD_ERR_INDEX_OVERFLOW when no S in [0, 24] satisfies the rule (a voxel size of hundreds of thousands of kilometres). */
int vofod_set_raycast_exact(vofod_handle* h, int on);
/* vofod_raycast_units: the raw U of the pending exact pass (n = the map's voxel count, x fastest as vofod_read_map) and S.
 * VOFOD_ERR_NOT_PENDING: no exact pass is pending (none at all, or a float one); VOFOD_ERR_SIZE_MISMATCH: a wrong n. */
int vofod_raycast_units(vofod_handle* h, uint32_t* units, size_t n, int32_t* log2_units_per_m);
/* Host helper (no handle, no device): the pose table of a scan from two sensor->world poses.
 *     col_tfs[m] = tf_ref^-1 o P(frac[m]),   m = 0 .. n-1,   frac == NULL: frac[m] = m / (n - 1) (0 when n == 1)
 * P(f) interpolates tf_begin (f = 0) and tf_end (f = 1): translation linear, rotation R0 * exp(f * log(R0^T R1)) on the shortest
 * arc; f outside [0, 1] extrapolates (constant twist).  tf_ref is the pose the call's `tf` will be (usually tf_end, or the pose at
 * the scan's stamp).  Computed in double, cast to float at the end.  Rotation parts are taken as orthonormal: each is replaced
 * by the rotation nearest to it (a float matrix is orthonormal to 1e-7 only), the inverse is the transpose.  n <= 0 or a NULL pointer (frac excepted) is
 * VOFOD_ERR_INVALID_ARG. */
int vofod_column_poses(const float tf_begin[12], const float tf_end[12], const float tf_ref[12],
                       const double* frac /* n, NULL = m / (n - 1) */, int32_t n, float* col_tfs);
/* Host helper (no handle, no device): a lattice of candidate poses around `tf` for vofod_map_match.  Candidate
 *     k = ((iyaw * n[2] + iz) * n[1] + iy) * n[0] + ix,       i_a in [0, n[a]), iyaw in [0, n_yaw)
 * with d[a] = (i_a - (n[a] - 1) / 2.0) * step[a] and psi = (iyaw - (n_yaw - 1) / 2.0) * yaw_step (radians) is [R_k | t_k]:
 *     t_k = t + d;      rows of R_k:  cos(psi) R0 - sin(psi) R1,   sin(psi) R0 + cos(psi) R1,   R2
 * - a shift along the world's axes and a yaw about the vertical through the sensor's own origin.  Evaluated in double, each entry
 * rounded to float once; the centre candidate of odd counts is `tf` itself.  tfs_out holds n[0] * n[1] * n[2] * n_yaw poses of 12
 * floats.  VOFOD_ERR_INVALID_ARG, with nothing written: a NULL pointer, any count below 1, a product of the counts above 65535, a
 * step or yaw_step that is not finite. */
int vofod_pose_lattice(const float tf[12], const float step[3], const int32_t n[3], float yaw_step, int32_t n_yaw,
                       float* tfs_out /* n[0]*n[1]*n[2]*n_yaw * 12 */);

/* ------------------------------------------------- member voxels and AABB of the detections (product library only)
 *
 * What the reference keeps beside a detection's position: detection_t::aabb (vofod_nodelet.cpp:121-130) and the cluster's points
 * cluster_t::pc / pc_indices (:110-119), for a tracker, a camera cue or a logger downstream.  Gathered on the device (k_det_points)
 * from what the production paths leave in the workspace the frames ran in - no debug view, no read-back of the weighted cloud.
 *
 * source     VOFOD_POINTS_SYNC, or a ticket 0..7 whose vofod_batch_collect has returned its detections.
 * ext        one record per detection, in the order of the detections returned; always host memory.
 * points     the members of detection 0, then those of detection 1, and so on.  Within a detection they ascend by the member's
 *            index in the frame's weighted cloud - the order of vofod_scan_debug::weighted and the order the labels of the debug
 *            view define.  Each record is the voxel's record bit for bit: centre and weight.
 * index      optional: that weighted-cloud index per point.
 * points and index live in points_memspace: VOFOD_MEM_HOST, or VOFOD_MEM_DEVICE on the handle's device with 4-byte alignment.
 *
 * Size query: with ext == NULL && points == NULL the call sets *n_ext and *n_points, launches nothing and returns VOFOD_OK (both
 * numbers are known on the host from the collected detections).  A NULL ext or a NULL points alone leaves that output out.
 * VOFOD_ERR_CAPACITY: ext_cap or points_cap is too small; both counts are set and nothing is written to any buffer.
 *
 * Validity: the answer belongs to the workspace the frames ran in.  It is valid from the return of that collect, or of the
 * synchronous call, until the next call on the handle that runs frames or stages inputs in the same workspace: ticket 0 shares its
 * workspace with the synchronous entry points and with vofod_range_to_points; vofod_reset and vofod_map_apply end the validity of
 * every source.  A call that did not return VOFOD_OK leaves nothing valid - in particular a collect that returned
 * VOFOD_ERR_CAPACITY and left its ticket pending - and so does a vofod_process_batch of more frames than max_batch_frames (its
 * launch groups overwrite each other).  The library tracks all this itself: when the source is not valid the call returns
 * VOFOD_ERR_NOT_PENDING, never stale data.  VOFOD_ERR_INVALID_ARG: a source outside -1..7, a bad memspace or alignment, NULL
 * count pointers, index without points.  VOFOD_ERR_DEVICE: a HIP error, or a cluster whose member list does not hold n_points
 * entries (vofod_last_error_string names the detection).
 * The call only reads the workspace and may run beside other batches in flight; it takes the handle's mutex like every call, runs
 * on the workspace's own chain stream and waits for that stream only.  With zero detections there is no launch. */
enum { VOFOD_POINTS_SYNC = -1 };   /* source: the last synchronous vofod_process_scan / vofod_process_batch */
typedef struct vofod_detection_extent {   /* 40 bytes, one per detection, in the order of the detections returned */
  uint32_t id, frame;          /* as in the vofod_detection it belongs to */
  uint32_t first, count;       /* its members are points[first .. first + count); count == vofod_detection::n_points */
  float aabb_min[3], aabb_max[3];   /* float min / max of the members' centres: cluster_t::aabb, getMinMax3D */
} vofod_detection_extent;
int vofod_detection_points(vofod_handle* h, int source,
                           vofod_detection_extent* ext, size_t ext_cap, size_t* n_ext,
                           vofod_point_xyzr* points, uint32_t* index /* nullable */, size_t points_cap, size_t* n_points,
                           int32_t points_memspace);

/* ------------------------------------------------- raw returns of the detections: their scan pixels (product library only)
 *
 * vofod_detection_points stops at voxel centres.  This call hands out the sensor returns themselves: for every detection the
 * pixels i = row * width + col of its frame's organised scan that fell into its member voxels - for a tracker that re-fits the
 * target, a camera cue that needs (row, col) in the range image, a logger, a classifier fed the cut-out points.  Answered on the
 * device (k_det_pixels, vofod_amd/csrc/detection_pixels.h) from what the production call left in the workspace.
 *
 * Definition.  Pixel i of frame f belongs to detection d iff (1) the pipeline kept its point: finite, outside the closed exclude
 * box, inside the closed operation area after the transform with the frame's tf (pcl association, every op rounded), and (2) its
 * VoxelGridWeighted cell - floor((q - offset) * inv_leaf) per axis in float32 with the FRAME'S OWN lattice offset
 * (voxel_grid_weighted.cpp:131-136) - is the cell of a member voxel of d.  The point is the one the pipeline consumed: the decoded
 * point of a range image, the compensated point of a scan with col_tfs.
 *
 * source, validity, refusals: exactly as vofod_detection_points (VOFOD_POINTS_SYNC or a collected ticket; VOFOD_ERR_NOT_PENDING
 * when the source is not valid, never stale data; VOFOD_ERR_INVALID_ARG for a source outside -1..7, a bad memspace or alignment,
 * NULL count pointers, member or xyz without pixels).
 * span       one record per detection, in the order of the detections returned; always host memory.
 * pixels     the pixel indices of detection 0, then those of detection 1, and so on; within a detection they ascend.
 * member     optional: per pixel, the position of its voxel in that detection's list as vofod_detection_points returns it
 *            (points[ext.first + member] is the voxel the return fell into).
 * xyz        optional: per pixel the transformed point q, 3 floats, bit for bit what the voxel grid consumed.
 * pixels, member and xyz live in memspace: VOFOD_MEM_HOST, or VOFOD_MEM_DEVICE on the handle's device with 4-byte alignment.
 *
 * Invariant: span.count is the sum of the weights (vofod_point_xyzr::r bits, the returns per voxel) of the detection's member
 * voxels, and every member voxel gets exactly its weight in pixels.  The library holds every answer to the first half: a
 * detection whose returns do not number the sum of its weights makes the call return VOFOD_ERR_DEVICE with nothing written to any
 * output; vofod_last_error_string names the detection.
 * One rule of its own: device-resident scan columns (memspace VOFOD_MEM_DEVICE of the scan) are read in place, once more, by
 * this call - the caller leaves them unchanged from the production call until it has asked.  Host-resident scans, range images
 * and scans with col_tfs are answered from the library's staging slot and need nothing kept.
 *
 * Size query: span == NULL && pixels == NULL sets *n_span and *n_pixels and returns VOFOD_OK; the first query after a production
 * call launches the small sizing kernel (one workgroup per detection sums the weights), never the pixel walk.  A NULL span or a
 * NULL pixels alone leaves that output out.  VOFOD_ERR_CAPACITY: span_cap or pixels_cap is too small; both counts are set and
 * nothing is written.  The call only reads the workspace, runs on the workspace's own chain stream and waits for that stream
 * only.  With zero detections there is no launch. */
typedef struct vofod_detection_span {   /* 16 bytes, one per detection, in the order of the detections returned */
  uint32_t id, frame;                   /* as in the vofod_detection it belongs to */
  uint32_t first, count;                /* its returns are pixels[first .. first + count) */
} vofod_detection_span;
int vofod_detection_pixels(vofod_handle* h, int source,
                           vofod_detection_span* span, size_t span_cap, size_t* n_span,
                           uint32_t* pixels, uint32_t* member /* nullable */, float* xyz /* nullable, 3 per pixel */,
                           size_t pixels_cap, size_t* n_pixels, int32_t memspace);

/* ------------------------------------------------- batched mode: the collective (product library only)
 *
 * one process per GPU runs vofod_process_batch / vofod_batch_submit+collect on its own block of frames; the only
 * exchange is one all-gather of fixed-size slots - d_max 128-byte vofod_detection records (msgs/Detection.msg:1-12 + frame)
 * and a count word per frame - with RCCL over xGMI.  The communicator is RCCL's: one rank asks for an id
 * (ncclGetUniqueId), the host program ships its 128 bytes to the other ranks by whatever means it has (MPI, a socket,
 * torch.distributed), every rank creates its vofod_comm from it (ncclCommInitRank).  RCCL is loaded at run time.
 * The CPU oracle does not export these (it has no device to gather on). */
#define VOFOD_COMM_ID_BYTES 128
typedef struct vofod_comm vofod_comm;
int vofod_comm_unique_id(uint8_t id[VOFOD_COMM_ID_BYTES]);
int vofod_comm_create(const uint8_t id[VOFOD_COMM_ID_BYTES], int32_t rank, int32_t n_ranks, int32_t device, vofod_comm** out);
void vofod_comm_destroy(vofod_comm* comm);
const char* vofod_comm_last_error(vofod_comm* comm);
/* The exchange's wire format as plain host functions (no device, no communicator): a caller with a transport of its own (MPI,
 * gloo) packs, all-gathers `frames * vofod_detection_slot_bytes(d_max)` bytes per rank and unpacks.  Slot of a frame: d_max
 * records of 128 bytes (the frame's first detections in order, zero padded) followed by the frame's true count (8 bytes). */
size_t vofod_detection_slot_bytes(size_t d_max);
int vofod_pack_detection_slots(const vofod_detection* local, const uint32_t* n_per_frame, size_t frames, size_t d_max, void* slots);
int vofod_unpack_detection_slots(const void* slots, size_t frames_total, size_t d_max, vofod_detection* all, uint32_t* all_counts);
/* local: this rank's detections in frame order (what vofod_process_batch / vofod_batch_collect returned), n_per_frame: their
 * count per frame.  all: n_ranks * frames_per_rank * d_max records, slot (rank, frame) holds min(count, d_max) records;
 * all_counts: n_ranks * frames_per_rank counts (a count above d_max tells that the slot was truncated). */
int vofod_allgather_detections(vofod_comm* comm, const vofod_detection* local, const uint32_t* n_per_frame, size_t frames_per_rank, size_t d_max, vofod_detection* all,
                               uint32_t* all_counts);

/* ------------------------------------------------- map snapshots and deltas (product library only)
 *
 * Moving a map between handles, processes and GPUs: checkpoints at shutdown / restore in onInit, and replicas of a live map
 * for the batched mode.  The reference has no counterpart: it can reload only its a-priori cloud (:306-355).
 *
 * `maps` is a bitmask of (1 << VOFOD_MAP_VOXELS) | (1 << VOFOD_MAP_FLAGS) | (1 << VOFOD_MAP_RAYCAST).
 *   VOFOD_SNAPSHOT_FULL   every voxel of each selected map whose 32-bit pattern differs from that map's init state (score_init
 *                         for the voxel map, 0.0f for flags and raycast); applying it resets the selected maps to init first.
 *                         Applies to any handle with the same map size, offset, voxel size and score_init; starts a chain.
 *   VOFOD_SNAPSHOT_DELTA  the voxels whose bits differ from what this handle last exported with the same mask.  Applies only on
 *                         a handle whose last applied snapshot (full or delta) has generation == the delta's base_gen and the
 *                         same mask; otherwise VOFOD_ERR_DELTA_BASE and nothing is written.  Exporting a delta without a chain
 *                         for the mask (one chain per handle: a full export of another mask replaces it) is VOFOD_ERR_DELTA_BASE.
 *                         vofod_reset / vofod_write_map on the owner do not break the chain.
 * Records are sorted by strictly ascending idx = ix + iy*sx + iz*sx*sy.  The export keeps a shadow copy of each exported map:
 * 4 * M bytes per map (78 MB at 0.25 m, 1.2 GB at 0.1 m), allocated on its first export and freed by vofod_destroy.
 *
 * Wire format (little endian; the same bytes in memory, over RCCL and in a file): a 128-byte header
 *   0 u32 magic 0x444D4656 ("VFMD") | 4 u32 version = 1 | 8 u32 maps | 12 u32 kind (0 delta, 1 full) | 16 i32[3] map size |
 *   28 f32[3] map offset (as vofod_status_info) | 40 f32 voxel size | 44 f32 score_init | 48 u64 base_gen (0 for full) |
 *   56 u64 new_gen | 64 i32 detection_its, u32 last_detection_id, i32 background_pts_sufficient, i32 sure_background_sufficient |
 *   80 i32 raycast_pending, i32 raycast_start_its | 88 u64[3] records per map (voxels, flags, raycast; 0 when not selected) |
 *   112 u8 S + 1 of a pending exact raycast pass that travels with the raycast map (EXACT RAYCAST ACCUMULATION at vofod_scan: the
 *       raycast records are then uint32 units, 2^S per metre), else 0 | 113 15 zero bytes
 * followed, per selected map in that order, by u32 idx[n] and u32 bits[n].  Size = 128 + 8 * sum(n).
 *
 * Apply always restores detection_its, last_detection_id and both background latches; raycast_pending and raycast_start_its
 * only when the snapshot holds both FLAGS and RAYCAST (the next vofod_raycast_finish then does what the owner's would).  A
 * pending sepclusters pass is not carried (its cluster list lives in the owner's workspace) and the applying handle's own
 * pending pass is dropped.  Derived state (occupancy images, nVoxelsOver) is rebuilt on next use, as after vofod_write_map.
 * Apply checks everything before it writes: format (VOFOD_ERR_INVALID_ARG), geometry (VOFOD_ERR_SIZE_MISMATCH), chain
 * (VOFOD_ERR_DELTA_BASE), record indices ascending and < M (VOFOD_ERR_INVALID_ARG, checked on the device); VOFOD_ERR_BUSY
 * while a submitted batch is pending.  Export only reads the maps and may run beside batches in flight. */
enum { VOFOD_SNAPSHOT_DELTA = 0, VOFOD_SNAPSHOT_FULL = 1 };
/* buf == NULL && cap == 0: size query (*n_bytes set, nothing changes).  cap too small: VOFOD_ERR_CAPACITY with *n_bytes = the
 * size, generation and shadow untouched.  memspace: VOFOD_MEM_HOST or VOFOD_MEM_DEVICE (4-byte aligned, the handle's device). */
int vofod_map_export(vofod_handle* h, int32_t maps, int32_t kind, void* buf, size_t cap, int32_t memspace, size_t* n_bytes);
int vofod_map_apply(vofod_handle* h, const void* buf, size_t n_bytes, int32_t memspace);
/* Collective over comm (every rank calls it with the same arguments; comm and h on the same device): the root exports `kind`
 * of `maps` into a device staging buffer of h, broadcasts a 16-byte control word (status, bytes) and then the payload with
 * RCCL; the other ranks apply it from device memory.  *n_bytes = the snapshot's size on every rank.  The outcome is
 * collective: every rank returns the same status - the root's when its export fails (nobody applies), otherwise the largest
 * of the receiving ranks' statuses (staging allocation, VOFOD_ERR_BUSY, and the apply: VOFOD_ERR_DELTA_BASE when a replica
 * missed a delta), VOFOD_OK when every rank applied.  So a recovery such as "on VOFOD_ERR_DELTA_BASE broadcast a full
 * snapshot" runs on all ranks together.  Any other export by the root (vofod_map_export, a checkpoint) starts a new chain:
 * the next delta broadcast then returns VOFOD_ERR_DELTA_BASE everywhere.  Only a failing HIP runtime or RCCL call
 * (VOFOD_ERR_DEVICE) can end the call on one rank alone. */
int vofod_broadcast_map(vofod_comm* comm, vofod_handle* h, int32_t root, int32_t maps, int32_t kind, size_t* n_bytes);

/* ------------------------------------------------- rolling operation area (product library only)
 *
 * Moves the operation area by a whole number of voxels and keeps what the maps hold about the overlap: for a vehicle that leaves
 * the box the maps were allocated for.  The reference has no counterpart (its maps are sized once, in onInit).  Afterwards the
 * handle behaves exactly like a handle created with the same static parameters except oparea_offset = new_oparea_offset, whose
 * three maps hold, with s = shift_voxels, sizes S and x fastest as everywhere,
 *     new[ix, iy, iz] = old[ix + s0, iy + s1, iz + s2]   where every i + s lies in [0, S),
 *     the map's init value elsewhere (score_init for the voxel map, +0.0f for flags and raycast).
 * Values move as 32-bit patterns (+inf, -0.0f and NaN payloads survive bit for bit).  |s[a]| >= S[a] on any axis is legal and
 * leaves all three maps at init; s == 0 with an unchanged offset is a no-op that returns VOFOD_OK.  One streaming pass per map on
 * the device (k_map_shift), out of place into a spare buffer of 4 * M bytes that is allocated by the first shift and freed by
 * vofod_destroy; map sizes do not change.
 *
 * Geometry: the library derives everything from new_oparea_offset with the expressions vofod_create uses, then checks per axis
 *     | map_offset_new[a] - (map_offset_old[a] + s[a] * voxel_size) | < voxel_size / 4
 * (map_offset as in vofod_status_info) and returns VOFOD_ERR_INVALID_ARG with nothing changed when shift and offset disagree - a
 * wrong sign or axis is off by a voxel or more.  Offsets chosen as base + k * voxel_size from an INTEGER k that the caller keeps
 * (k += s per shift) do not drift: every offset is then one rounding away from the exact value, however many shifts led to it,
 * whereas offset += s * voxel_size accumulates a rounding per shift.
 *
 * State: VOFOD_ERR_BUSY, with nothing changed, while a submitted batch is pending, a raycast pass is pending (raycast_pending of
 * vofod_status_info: finish it first) or a sepclusters pass is pending between begin and finish.  Kept: detection_its,
 * last_detection_id, both background latches, the dynamic parameters, workspaces, streams and tickets' buffers.  Derived state
 * (occupancy images, nVoxelsOver) is rebuilt on next use, as after vofod_write_map.  vofod_detection_points answers
 * VOFOD_ERR_NOT_PENDING for every source until the next production call.  The snapshot chain ends on both sides: the next
 * VOFOD_SNAPSHOT_DELTA export or apply answers VOFOD_ERR_DELTA_BASE, a full export starts a new chain, and a snapshot taken
 * before the shift is refused by apply's geometry check (VOFOD_ERR_SIZE_MISMATCH: the header carries the offset).  A replica
 * shifts first and then takes a full snapshot. */
int vofod_map_shift(vofod_handle* h, const int32_t shift_voxels[3], const float new_oparea_offset[3]);

/* ------------------------------------------------- MAP RENDER (product library only)
 *
 * MAP RENDER.  The expected range image: the voxel map rendered through the handle's own LUT from a pose - standing here, looking
 * there, what does the map say I should see?  One uint32 millimetre value per pixel, in the sensor's own format: it compares
 * pixel by pixel with a measured scan, it goes back into vofod_process_scan / vofod_raycast_begin as a range image, it answers
 * line-of-sight queries for many poses in one call, and it turns any map into a scan generator.  Answered on the device
 * (k_map_render, vofod_amd/csrc/map_render.h); the CPU oracle does not have it.
 *
 * Pixel and ray.  For view v and pixel i = row * width + col the ray is the rigid ray of the raycast role:
 *     d = lut_directions[3i..], o = lut_offsets[3i..] (zeros when the handle has none), [R | t] = tfs[12v .. 12v + 12) row-major
 *     dir[k]   = ((R[k][0]*d[0]) + (R[k][1]*d[1])) + (R[k][2]*d[2])
 *     start[k] = (((R[k][0]*o[0]) + (R[k][1]*o[1])) + (R[k][2]*o[2])) + t[k]
 * IEEE float32, each operation rounded once, nothing fused.  No mask, no intensity gate, no exclude box and no col_tfs apply:
 * every pixel is cast.  The map read is VOFOD_MAP_VOXELS as it stands when the call is serialised.
 *
 * Walk.  VoxelMap::forEachRay (voxel_map.cpp:229-263) with length = max_distance, vs the voxel size, off the map's origin:
 *     cur[a]    = (int) floorf((start[a] - off[a]) * (1.0f / vs))                  the start's voxel
 *     step[a]   = sign(dir[a]) (0 for a zero),  last[a] = step[a] > 0 ? size[a] - 1 : 0
 *     tdelta[a] = (1.0f / |dir[a]|) * vs
 *     ctr[a]    = (((float) cur[a] + 0.5f) * vs) + off[a]
 *     tmax[a]   = ((vs / 2.0f) + ((float) step[a] * (ctr[a] - start[a]))) / |dir[a]|
 *     if cur is outside the map                    -> what = NOT_CAST
 *     prev = 0
 *     loop:
 *         a = the axis of the smallest tmax, the first one on ties;  dist = tmax[a]
 *         if map[cur] > threshold                  -> what = HIT,  t_in = prev, t_out = min(dist, length); stop
 *         if !(dist < length)                      -> what = END;  stop      (the length ran out inside cur)
 *         if cur[a] == last[a]                     -> what = LEFT; stop      (the next step would leave the map)
 *         cur[a] += step[a]; tmax[a] = tmax[a] + tdelta[a]; prev = dist
 * `>` is the float compare: a NaN voxel is never a hit, +inf (an a-priori voxel) is, a voxel equal to the threshold is not.
 *
 * Outputs, each n_views * width * height values indexed (v * height + row) * width + col, each nullable:
 *     what      one of VOFOD_RENDER_*
 *     voxel     HIT: the linear index (z * sy + y) * sx + x of the hit voxel (the order of vofod_read_map); otherwise 0xffffffff
 *     t_in_out  two floats per pixel.  HIT: (t_in, t_out), the piece of the ray inside the hit voxel in metres from start;
 *               END, LEFT: (prev, min(dist, length)) of the last voxel looked at; NOT_CAST: (0, 0)
 *     range     HIT: max(1, (uint32) rintf(((t_in + t_out) * 0.5f) * 1000.0f)) - the middle of that piece in the sensor's
 *               millimetres, ties to even, never the 0 that means "no return" (the float is clamped to 2^32 - 256 before the
 *               conversion); otherwise 0
 * They live in out_memspace: VOFOD_MEM_HOST, or VOFOD_MEM_DEVICE on the handle's device, written in place - range and voxel
 * 4-byte aligned, t_in_out 8-byte aligned.
 *
 * Refusals.  VOFOD_ERR_INVALID_ARG: n_views == 0 or above 65535, tfs == NULL, all four outputs NULL, !(max_distance > 0), a NaN
 * threshold, an unknown memspace, a misaligned device output.  VOFOD_ERR_SENSOR_OUTSIDE_MAP, with nothing written, when the origin
 * t of any view lies outside the map - the rule vofod_raycast_begin applies to its one tf.  VOFOD_ERR_DEVICE as everywhere.
 *
 * The call reads the voxel map only and uses a workspace of its own: it is admitted with tickets in flight and with a raycast
 * pass (float or exact) or a sepclusters pass pending, runs on the handle's stream behind what was enqueued, returns after one
 * synchronisation and changes nothing another call can observe - maps, latches, ids, detections, tickets, snapshot chains.
 * World store: the window is rendered; a ray that reaches the window's face is LEFT.  Rendering through the store's tiles is out
 * of scope, and so is the occupancy image as a shortcut for its own threshold.  A pose per column (col_tfs): SCANS AGAINST THE MAP. */
enum { VOFOD_RENDER_NOT_CAST = 0, VOFOD_RENDER_HIT = 1, VOFOD_RENDER_END = 2, VOFOD_RENDER_LEFT = 3 };
int vofod_map_render(vofod_handle* h, const float* tfs /* n_views * 12, host */, size_t n_views,
                     float threshold, float max_distance,
                     uint32_t* range /* n_views * w * h, nullable */,
                     uint32_t* voxel /* same, nullable */,
                     uint8_t* what   /* same, nullable */,
                     float* t_in_out /* n_views * w * h * 2, nullable */,
                     int32_t out_memspace);

/* ------------------------------------------------- SCANS AGAINST THE MAP (product library only)
 *
 * SCANS AGAINST THE MAP.  MAP RENDER with SCANS as its views: every ray is cast the way the scan measured it - from the pose of its
 * measurement column where the scan carries col_tfs - and every measured return is compared with what the map says the ray should
 * have met: a verdict per pixel, and the number of pixels of each verdict per scan.  Which returns lie in space the map holds
 * free?  Which share of this scan agrees with the map under this pose?  Answered on the device by the walk of MAP RENDER
 * (k_map_render_scans, vofod_amd/csrc/map_render.h: the same kernel template); the CPU oracle does not have it.
 *
 * Views.  View v is scans[v] under [R | t] = tfs[12v .. 12v + 12).  Of a scan the call reads width, height, memspace, col_tfs, and
 * range with stride_bytes - range only when verdict or counts is asked for; x, y, z and intensity are never read.  Device-resident
 * range columns and pose tables are read in place, host-resident ones are staged in the call's own workspace; the caller may
 * overwrite every input when the call returns.
 *
 * Ray of pixel i = row * width + col of view v.
 *     col_tfs == NULL   the rigid ray of MAP RENDER: every output is bit for bit what vofod_map_render gives for tfs[v].
 *     col_tfs != NULL   d', o' exactly as MOTION-COMPENSATED RAYS defines them: m = (col + shift_by_row[row]) mod width with the
 *                       handle's column shifts (vofod_set_column_shift), T = col_tfs[m], in that section's association, nothing
 *                       fused; then dir = R d' and start = (R o') + t in MAP RENDER's association.  This holds whatever
 *                       vofod_set_raycast_motion says: that switch belongs to the raycast role.
 * The two matrices are never multiplied together.  A ray whose own start lies outside the map is NOT_CAST.
 *
 * Walk and outputs.  The walk and the outputs range, voxel, what and t_in_out are MAP RENDER's, word for word, with
 * length = max_distance.
 *
 * Verdict.  With r = range[i] of the scan (uint32 millimetres), rm = (float) r * 0.001f (the decode's expression),
 * tol = tolerance, (what, t_in, t_out) the render of the same pixel and mask the handle's mask - every operation float32, rounded
 * once, the comparisons the float compares (a NaN makes them false):
 *     what == NOT_CAST                          -> NONE
 *     r == 0 && mask[i] == 0                    -> NONE      (the reference casts no ray there either: vofod_nodelet.cpp:1449)
 *     r == 0:   what == HIT -> MISSING          else -> EMPTY
 *     r  > 0, what == HIT:  (rm + tol) < t_in   -> NEARER    (a return in space the map holds free, in front of its surface)
 *                           rm > (t_out + tol)  -> THROUGH   (a return behind the surface the map expects)
 *                           otherwise           -> AGREES
 *     r  > 0, what == END or LEFT:
 *                           (rm + tol) < t_out  -> NEARER
 *                           otherwise           -> BEYOND    (beyond the rendered length or the map's face: nothing to compare)
 * verdict holds n_scans * width * height of them, indexed as the render outputs, in out_memspace (no alignment asked).
 *
 * Counts.  counts[8v + c] is the number of pixels of view v with verdict c; slot 7 is 0; the eight slots of a view sum to
 * width * height.  Integers: exact, whatever the order they were counted in.  counts is ALWAYS host memory.
 *
 * Refusals, with nothing written to any output.  VOFOD_ERR_INVALID_ARG: n_scans == 0 or above 65535, scans or tfs NULL, all six
 * outputs NULL, !(max_distance > 0), a NaN threshold, a tolerance that is NaN or negative, an unknown memspace of the outputs or of
 * any scan, a misaligned device output (MAP RENDER's rule), verdict or counts asked for with a scan whose range is NULL, a
 * device-resident range whose base or stride is no multiple of 4, a device-resident col_tfs that is not 4-byte aligned.
 * VOFOD_ERR_SIZE_MISMATCH: a scan whose width or height is not the handle's.  VOFOD_ERR_SENSOR_OUTSIDE_MAP: the origin t of any
 * tfs[v] lies outside the map.  VOFOD_ERR_DEVICE as everywhere.
 *
 * Admission is MAP RENDER's: the call reads the voxel map only, uses its own workspace, makes one launch on the handle's stream
 * and one synchronisation, is admitted with tickets in flight and with a raycast or sepclusters pass pending, and changes nothing
 * another call can observe.  Out of scope: shortening a walk by the measured range, rendering through the world store's tiles,
 * a signed residual output (range gives it). */
enum { VOFOD_VERDICT_NONE = 0, VOFOD_VERDICT_AGREES = 1, VOFOD_VERDICT_EMPTY = 2, VOFOD_VERDICT_NEARER = 3,
       VOFOD_VERDICT_THROUGH = 4, VOFOD_VERDICT_MISSING = 5, VOFOD_VERDICT_BEYOND = 6 };
int vofod_map_render_scans(vofod_handle* h, const vofod_scan* scans, const float* tfs /* n_scans * 12, host */, size_t n_scans,
                           float threshold, float max_distance, float tolerance,
                           uint32_t* range, uint32_t* voxel, uint8_t* what, float* t_in_out,   /* as vofod_map_render, nullable */
                           uint8_t* verdict /* n_scans * w * h, nullable, out_memspace */,
                           uint32_t* counts /* n_scans * 8, nullable, ALWAYS host */,
                           int32_t out_memspace);

/* ------------------------------------------------- MAP MATCH (product library only)
 *
 * MAP MATCH.  Candidate poses scored against the map: where do this scan's returns land under pose k?  One map look-up per return
 * and candidate - not a ray walk - for up to 65535 candidates of one scan in one call: the tool a caller needs when the counts of
 * SCANS AGAINST THE MAP say that the pose has drifted.  Answered on the device (k_match_bits, k_match_points, k_match_score,
 * vofod_amd/csrc/map_match.h); the CPU oracle does not have it.  Every operation is IEEE float32, rounded once, nothing fused.
 *
 * The scan's point.  For pixel i = row * width + col, p is
 *     range image (x == y == z == NULL, range given)   the p of RANGE IMAGES
 *     range image with col_tfs                         the p of MOTION COMPENSATION, with the handle's column shifts and that
 *                                                      section's NaN rule for q inside the exclude box
 *     point scan (x, y, z given, no col_tfs)           p = (x[i], y[i], z[i]) as given; range and intensity are not read
 *
 * SKIPPED.  A pixel is SKIPPED when any of these holds, and live otherwise; it does not depend on the candidate:
 *     range[i] == 0 on a range image;  all three coordinates zero, of either sign, on a point scan;
 *     any p[a] is not finite;
 *     lo[a] <= p[a] <= hi[a] on all three axes - the closed exclude box as the first crop uses it (vofod_nodelet.cpp:626-629).
 *
 * Candidate k.  [R | t] = tfs[12k .. 12k + 12) row-major, and for a live pixel
 *     w[a] = R[a][0]*p[0] + (R[a][1]*p[1] + (R[a][2]*p[2] + t[a]))         (PCL's association, the pipeline's own transform)
 *     f[a] = floorf((w[a] - off[a]) * (1.0f / vs))                          (the voxel coordinate, before any conversion)
 * with off the map's origin, vs the voxel size and size the map's size in voxels.
 *
 * Class of a live pixel.  OUTSIDE unless f[a] >= 0.0f && f[a] < (float) size[a] on all three axes - compared as floats before the
 * conversion, so a NaN or infinite w is OUTSIDE and no out-of-range float is ever converted.  Inside, with (x, y, z) = (int) f and
 * v = (z * sy + y) * sx + x: OCCUPIED when map[v] > threshold, FREE otherwise - the float compare of MAP RENDER: a NaN voxel is
 * FREE, a +inf voxel is OCCUPIED, a voxel equal to the threshold is FREE.  The map is VOFOD_MAP_VOXELS as it stands when the call
 * is serialised.
 *
 * Outputs.  counts[4k + c] is the number of pixels of class c under candidate k (host memory); the four slots of a candidate sum to
 * width * height, and slot 0 (SKIPPED) is the same for every k.  Integers: exact, whatever the order they were counted in.
 * *best (nullable) is the smallest k with the largest counts[4k + 3].
 *
 * Refusals, decided before the lock, with nothing written.  VOFOD_ERR_INVALID_ARG: h, scan, tfs or counts NULL; n_poses == 0 or
 * above 65535; a NaN threshold; an unknown memspace; exactly one or two of x, y, z NULL; all three NULL without range; a point scan
 * that carries col_tfs (whatever vofod_set_point_motion says); a device-resident column or range whose base or stride is no
 * multiple of 4; a device-resident col_tfs that is not 4-byte aligned.  VOFOD_ERR_SIZE_MISMATCH: the scan's width or height is not
 * the handle's.  There is no SENSOR_OUTSIDE_MAP rule: a candidate may lie anywhere, and its points are then OUTSIDE.
 * VOFOD_ERR_DEVICE as everywhere.
 *
 * Admission is MAP RENDER's: the call reads the voxel map only, stages host inputs in a workspace of its own, runs on the handle's
 * stream, returns after one synchronisation, is admitted beside tickets in flight and beside a pending raycast (float or exact) or
 * sepclusters pass, and changes nothing another call can observe.  World store: the window is matched.  What the score says: how
 * many returns fall into voxels the map holds occupied - a correlation, high where the scan's surfaces lie on the map's.  What it
 * does not say: a likelihood, or anything about free space the rays crossed (SCANS AGAINST THE MAP answers that).  Out of scope: a
 * NEAR class, several scans per call, a search loop (the caller owns coarse-to-fine; vofod_pose_lattice builds the candidates),
 * matching through the world store's tiles. */
enum { VOFOD_MATCH_SKIPPED = 0, VOFOD_MATCH_OUTSIDE = 1, VOFOD_MATCH_FREE = 2, VOFOD_MATCH_OCCUPIED = 3 };
int vofod_map_match(vofod_handle* h, const vofod_scan* scan,
                    const float* tfs /* n_poses * 12, host */, size_t n_poses, float threshold,
                    uint32_t* counts /* n_poses * 4, host */, int32_t* best /* one value, host, nullable */);

/* ------------------------------------------------- MAP DISTANCE (product library only)
 *
 * MAP DISTANCE.  The Euclidean distance transform of the voxel map - for every voxel, how far away is the nearest occupied one -
 * and candidate poses scored by it.  MAP MATCH counts hits, a step function of the pose; the distance gives the score a slope: a
 * likelihood field for a scan matcher, clearance for a planner, "how far from the background does this detection float" for a
 * consumer.  Answered on the device (k_match_bits, k_dist_x, k_dist_y, k_dist_z, k_match_points, k_match_field;
 * vofod_amd/csrc/map_distance.h); the CPU oracle does not have it.  Squared voxel distances are integers: both calls are exact,
 * whatever the order anything was computed in.
 *
 * vofod_map_distance.  A voxel u is occupied when map[u] > threshold - the float compare of MAP MATCH: a NaN voxel is free, a +inf
 * voxel is occupied, a voxel equal to the threshold is free; an infinite threshold is allowed.  With R = radius and
 * v = (z * sy + y) * sx + x,
 *     d2[v] = min(R * R,  min over occupied u of (dx * dx + dy * dy + dz * dz))          (dx, dy, dz: the voxel offsets from v to u)
 * in voxels, an integer: an occupied voxel holds 0, a map with nothing occupied holds R * R everywhere.  Only voxels inside the box
 * count, nothing wraps; with the world store on, the window is transformed.  The clamp at R * R is what lets a windowed search be
 * exact - a true d2 <= R * R has every axis offset <= R - and it is the truncated-quadratic robust cost a matcher wants.
 * R <= VOFOD_DIST_MAX_RADIUS = 255 keeps R * R <= 65025 within uint16_t.  The map is VOFOD_MAP_VOXELS as it stands when the call
 * is serialised; d2 holds sx * sy * sz values in `memspace`.
 * Refusals, decided before the lock, with nothing written.  VOFOD_ERR_INVALID_ARG: h or d2 NULL; a NaN threshold; radius < 1 or
 * radius > 255; an unknown memspace; a device d2 that is not 2-byte aligned.  VOFOD_ERR_SIZE_MISMATCH: n is not the map's voxel
 * count.  VOFOD_ERR_DEVICE as everywhere.
 * Admission is MAP RENDER's: the call reads the voxel map only, keeps a workspace of its own on the handle, runs on the handle's
 * stream, returns after one synchronisation, is admitted beside tickets in flight and beside a pending raycast (float or exact) or
 * sepclusters pass, and changes nothing another call can observe.  The work grows with the radius where the map is empty
 * (O(N * R) at worst; DESIGN.md 5.22 has the times).
 *
 * vofod_map_match_field.  The scan's point, SKIPPED, candidate k, the float bounds test and v are MAP MATCH's, word for word (that
 * section; not restated here).  An inside pixel is NEAR when d2[v] <= near2 and FAR otherwise, and
 *     cost[k] = (sum of d2[v] over the inside pixels) + outside_cost * OUTSIDE_k                           (64 bits, exact)
 * counts[4k + c] is the number of pixels of class VOFOD_FIELD_* c under candidate k; the four slots of a candidate sum to
 * width * height, slot 0 is the same for every k.  *best (nullable) is the smallest k with the smallest cost[k].  The field is an
 * INPUT: any uint16_t values, sx * sy * sz of them in field_memspace - what vofod_map_distance wrote, or anything else.  The caller
 * owns how fresh it is (a field a few scans old is what a matcher uses); the call reads d2 and the scan, not the voxel map.  With
 * near2 = 0 and the field of vofod_map_distance, NEAR is MAP MATCH's OCCUPIED at the same threshold.  counts and cost are host
 * memory.
 * Refusals: all of MAP MATCH's but the threshold's, and VOFOD_ERR_INVALID_ARG also for d2 or cost NULL, an unknown field_memspace,
 * a device d2 that is not 2-byte aligned, outside_cost > 65535; VOFOD_ERR_SIZE_MISMATCH also when n is not the map's voxel count.
 * near2 is never refused: a value above the field's maximum makes every inside pixel NEAR.  Admission is MAP MATCH's; a host field
 * is staged in the call's workspace, a device field is read in place.
 *
 * Out of scope: a feature transform (the nearest voxel's index: ties make it order-dependent), distances through the world store's
 * tiles, a field patched incrementally by the map update, sub-voxel interpolation, a search loop, several scans per call. */
enum { VOFOD_DIST_MAX_RADIUS = 255 };
int vofod_map_distance(vofod_handle* h, float threshold, int32_t radius,
                       uint16_t* d2 /* sx*sy*sz, memspace */, size_t n, int32_t memspace);
enum { VOFOD_FIELD_SKIPPED = 0, VOFOD_FIELD_OUTSIDE = 1, VOFOD_FIELD_FAR = 2, VOFOD_FIELD_NEAR = 3 };
int vofod_map_match_field(vofod_handle* h, const vofod_scan* scan,
                          const float* tfs /* n_poses*12, host */, size_t n_poses,
                          const uint16_t* d2 /* sx*sy*sz */, size_t n, int32_t field_memspace,
                          uint32_t near2, uint32_t outside_cost,
                          uint32_t* counts /* n_poses*4, host */, uint64_t* cost /* n_poses, host */,
                          int32_t* best /* nullable */);

/* ------------------------------------------------- WORLD STORE (product library only)
 *
 * vofod_map_shift alone forgets what leaves the box.  With the world store enabled the handle is a WINDOW onto a map larger than
 * the box: a sparse, tiled store on the device that the shift writes what leaves into and reads what enters from.  Off after
 * vofod_create; while it is off every call behaves, launch for launch and bit for bit, as it does without this section.
 *
 * World indices.  While enabled the handle keeps an integer origin K[3], the world index of the window's voxel (0, 0, 0).  K = 0 at
 * enable, and every successful vofod_map_shift adds its shift_voxels to K (the value given, also where |s| >= S).  A shift that would
 * take a component of K outside +-2^30 is VOFOD_ERR_INVALID_ARG with nothing changed (store enabled only).
 * World box.  Fixed at enable: lo = -margin_lo, hi = S + margin_hi (exclusive), S the map sizes; all in world indices.
 * Tiles.  VOFOD_WORLD_TILE voxels per edge (2 KiB of uint32), the tile grid anchored at lo.  A dense directory of one word per tile of
 * the box and a pool of max_tiles tiles are allocated by vofod_world_enable and by nothing else: a shift never allocates.  Tiles are
 * never freed before vofod_reset or vofod_world_disable.
 * The store holds the VOXEL MAP only.  Flags and the raycast map are per-pass state: no pass can be pending at a shift, and their rim
 * enters as init, as without the store.
 *
 * The world view W maps a world index g to a 32-bit pattern:
 *     g inside the window:                            the voxel map's voxel g - K,
 *     otherwise g inside the box, its tile allocated: the stored pattern,
 *     otherwise:                                      the bits of score_init.
 *
 * vofod_map_shift with the store enabled (every refusal stays and still changes nothing):
 *   1. write back: every window voxel whose g lies outside the new window.  g in the box and its tile exists: the pattern is stored -
 *      a pattern equal to init too (the voxel may have been stored as something else on an earlier trip).  g in the box, no tile, the
 *      pattern differs from init: the tile is WANTED.  If all wanted tiles fit into the free part of the pool, all are allocated,
 *      filled with init, and take their patterns; if they do not fit NONE is allocated - the shift goes through all the same (the
 *      vehicle must not lose its box) and shifts_short_of_tiles goes up by one.  voxels_forgotten counts every leaving voxel that
 *      differs from init and found no place: outside the box, or in a tile that was not allocated.
 *   2. the maps move as stated at vofod_map_shift;
 *   3. read in: every voxel of the new window without a source in the old one takes the stored pattern where its tile exists and
 *      keeps the init value elsewhere;
 *   4. K += shift_voxels.
 * Consequence: with enough tiles and inside the box, W is the same function before and after any shift - only the window moves.
 *
 * vofod_load_apriori (and vofod_ingest_apriori through it) with the store enabled: the window is stamped as ever.  A point outside
 * the window goes to g[a] = K[a] + int(floor((p[a] - map_offset[a]) * (1 / voxel_size))) - the window's own float32 expression without
 * the in-limits cut; points whose floor is not finite or beyond +-2^30 are skipped.  g in the box: W(g) = +inf, allocating tiles.  The
 * call counts the tiles it needs before it changes anything: if they do not fit it returns VOFOD_ERR_CAPACITY with window, store and
 * latches untouched (unlike the shift: an a-priori load is init-time work, and the caller can enable a larger pool).  The world
 * remembers VOXELS, not points: the cell of a far point is decided by the window's geometry at load time.
 *
 * vofod_reset: W is init everywhere - the directory is emptied, the pool is free, the counters are zero; K, the box and the switch
 * are kept (the reference's reset(), which forgets the a-priori map too).  vofod_write_map, vofod_map_apply, vofod_map_export and
 * vofod_broadcast_map see and change the window only: the map snapshots do not carry the store (WORLD SNAPSHOTS below does). */
#define VOFOD_WORLD_TILE 8
typedef struct vofod_world_info {
  int32_t enabled, tile_edge;
  int32_t origin[3];                /* K */
  int32_t box_lo[3], box_hi[3];
  uint64_t tiles_used, tiles_cap;
  uint64_t shifts_short_of_tiles, voxels_forgotten;   /* cumulative since enable / reset */
} vofod_world_info;
/* VOFOD_ERR_INVALID_ARG: a negative margin, max_tiles == 0 (or above 2^32 - 16), a directory of more than 2^31 words, the store
 * already enabled.  VOFOD_ERR_BUSY, as for the shift: a submitted batch, a raycast pass or a sepclusters pass pending.
 * VOFOD_ERR_DEVICE: an allocation failed; nothing is kept.  tiles_cap = min(max_tiles, tiles of the box): more can never be used. */
int vofod_world_enable(vofod_handle* h, const int32_t margin_lo[3], const int32_t margin_hi[3], uint64_t max_tiles);
/* frees directory and pool; VOFOD_ERR_NOT_PENDING when not enabled; VOFOD_ERR_BUSY while a submitted batch is pending */
int vofod_world_disable(vofod_handle* h);
/* enabled = 0 and zeros when off */
int vofod_world_status(vofod_handle* h, vofod_world_info* out);
/* W over a box of world indices, x fastest, into host memory; n == size[0] * size[1] * size[2] (VOFOD_ERR_SIZE_MISMATCH otherwise).
 * VOFOD_ERR_NOT_PENDING when not enabled; VOFOD_ERR_INVALID_ARG: a size below 1, lo or lo + size beyond +-2^31. */
int vofod_world_read(vofod_handle* h, const int32_t lo[3], const int32_t size[3], float* dst, size_t n);

/* ------------------------------------------------- WORLD SNAPSHOTS (product library only)
 *
 * The store's counterpart of vofod_map_export / vofod_map_apply: a checkpoint keeps the world outside the box, and a ground station
 * or a second process holds a copy of it to answer vofod_world_read.  The map snapshots above still carry the window only; a restore is
 *     vofod_create at the checkpoint's offset, vofod_world_enable with the same margins, vofod_world_apply of the chain in order
 *     (a full snapshot, then its deltas), vofod_map_apply of a full window snapshot.
 * vofod_world_apply touches none of the three maps.  Both calls answer VOFOD_ERR_NOT_PENDING while the store is off.
 *
 * Wire format (little endian; the same bytes in memory and in a file): a 128-byte header
 *   0 u32 magic 0x44574656 ("VFWD") | 4 u32 version = 1 | 8 u32 kind (0 delta, 1 full) | 12 u32 tile edge (8) | 16 i32[3] map size |
 *   28 f32[3] map offset (as vofod_status_info) | 40 f32 voxel size | 44 f32 score_init | 48 u64 base_gen (0 for full) | 56 u64 new_gen |
 *   64 i32[3] K | 76 i32[3] box_lo | 88 i32[3] box_hi | 100 u32 zero | 104 u64 n tiles | 112 u64 shifts_short_of_tiles |
 *   120 u64 voxels_forgotten
 * followed by u32 tile[n4], n4 = n rounded up to a multiple of 4: the carried tiles' directory indices (tz * T1 + ty) * T0 + tx
 * (T = tiles of the box per axis), strictly ascending, the padding entries 0xFFFFFFFF; then n tiles of 512 u32 words, each as the pool
 * holds it (x fastest inside the tile; the padding voxels beyond box_hi travel verbatim).  Tile words start 16-byte aligned.
 * Size = 128 + 4 * n4 + 2048 * n.
 *
 * Export.  VOFOD_SNAPSHOT_FULL carries every allocated tile - one whose words all equal init too: allocation is state (tiles_used, and
 * every later all-or-nothing decision, depend on it) - and starts a chain (new_gen).  VOFOD_SNAPSHOT_DELTA carries every tile allocated
 * since this handle's last export and every tile with any of its 512 words different from what that export carried; without a chain
 * it is VOFOD_ERR_DELTA_BASE.  The comparison is against a shadow pool as large as the pool (2 KiB per tile of tiles_cap), allocated
 * by the first export and freed by vofod_world_disable / vofod_destroy; vofod_map_shift and vofod_load_apriori launch what they
 * launched before.  The owner's chain survives vofod_map_shift and vofod_load_apriori - those are what it records - and ends with
 * vofod_reset, vofod_world_disable and a vofod_world_apply on the same handle.  Export only reads the store and is admitted like
 * vofod_map_export (beside batches in flight too).  buf == NULL && cap == 0: size query (*n_bytes set, nothing changes).  cap too
 * small: VOFOD_ERR_CAPACITY with *n_bytes = the size, generation and shadow untouched.  memspace: VOFOD_MEM_HOST (staged through a
 * device buffer of the handle) or VOFOD_MEM_DEVICE on the handle's device, 16-byte aligned (VOFOD_ERR_INVALID_ARG otherwise).
 * VOFOD_ERR_DEVICE: the shadow pool or the staging buffer could not be allocated (the first export asks for as much memory again as
 * the pool holds); store, generation and chain are as before, and the call may be repeated.
 *
 * Apply checks everything before it writes anything, in this order:
 *   1. format, VOFOD_ERR_INVALID_ARG: magic, version, kind, tile edge, the zero word; the length against n; on the device: indices
 *      strictly ascending and below this handle's directory length, padding entries 0xFFFFFFFF;
 *   2. geometry, VOFOD_ERR_SIZE_MISMATCH: map size, voxel size, score_init, box_lo and box_hi equal this handle's, and the origin
 *      rule below;
 *   3. chain, VOFOD_ERR_DELTA_BASE: a delta's base_gen is the generation this handle applied last;
 *   4. capacity, VOFOD_ERR_CAPACITY, all or nothing: the carried tiles this handle has not allocated fit its pool (which may have
 *      another max_tiles than the owner's).
 * The window need not sit where the owner's sat.  With d[a] = round((map_offset_handle[a] - map_offset_header[a]) / voxel_size) in
 * double, the residual must be below voxel_size / 4 (vofod_map_shift's rule), and the handle's origin becomes K = header.K + d, held
 * inside +-2^30.  A full snapshot empties the store (as vofod_reset does to it) and then sets K; a delta requires the computed K to
 * equal the handle's own.  The computed K does not change when the owner shifts, so a handle that never shifts follows an owner that
 * does.  Then existing tiles are overwritten, new ones take slots and both cumulative counters take the header's values: afterwards
 * vofod_world_status equals the owner's in every field but tiles_cap, and vofod_world_read outside the window equals the owner's.
 * VOFOD_ERR_BUSY while a submitted batch is pending, as vofod_map_apply.
 *
 * The applied chain holds only while vofod_world_apply is the only writer of this handle's store: vofod_map_shift,
 * vofod_load_apriori, vofod_reset and vofod_world_disable on the applying handle end it (the next delta is VOFOD_ERR_DELTA_BASE, a
 * full snapshot repairs it) - every such call that returns VOFOD_OK, a shift by zero voxels and a cloud of zero points included.  Why: the replica's own shift writes its window back into its store, and a window that is stale - it is
 * fed by vofod_map_apply at another rhythm - would overwrite tiles the owner's deltas no longer carry; the two stores would differ
 * with every check passing.  A live replica therefore shifts first, then takes a full world snapshot and a full window snapshot.
 *
 * There is no collective of its own: with VOFOD_MEM_DEVICE on both sides a caller moves the bytes with the broadcast it already has
 * (RCCL, MPI) between vofod_world_export and vofod_world_apply. */
int vofod_world_export(vofod_handle* h, int32_t kind, void* buf, size_t cap, int32_t memspace, size_t* n_bytes);
int vofod_world_apply(vofod_handle* h, const void* buf, size_t n_bytes, int32_t memspace);

#ifdef __cplusplus
}
#endif
#endif /* VOFOD_H */
