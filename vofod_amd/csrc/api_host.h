// The entry points of include/vofod.h that take no handle and make no HIP call: default parameters, the sensor-LUT builders, the
// mask layout, the sensor-parameter check, the column poses, the ROS 1 wire serialisers and the cloud loader.  Standard headers and
// include/vofod.h only: vofod_hip.hip includes it, and api_host_check.cpp compiles it alone with the host compiler and its
// sanitizers - these functions do raw pointer arithmetic on the caller's buffers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/vofod.h"

namespace
{
struct WireOut
{
  uint8_t* buf;
  size_t cap, n = 0;
  template <class T>
  void put(const T& v)
  {
    if (buf && n + sizeof(T) <= cap)
      std::memcpy(buf + n, &v, sizeof(T));
    n += sizeof(T);
  }
  void str(const char* s)
  {
    const uint32_t len = s ? static_cast<uint32_t>(std::strlen(s)) : 0u;
    put(len);
    if (len && buf && n + len <= cap)  // (a NULL string has no bytes to copy: memcpy must not see it)
      std::memcpy(buf + n, s, len);
    n += len;
  }
  void header(const vofod_msg_header* h)
  {
    put(h->seq);
    put(h->stamp_sec);
    put(h->stamp_nsec);
    str(h->frame_id);
  }
};
}  // namespace

// ---- vofod_column_poses: host only, double throughout
namespace colposes
{
struct Quat
{
  double x, y, z, w;
};
inline Quat mul(const Quat& a, const Quat& b)
{
  return Quat{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w,
              a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
inline Quat conj(const Quat& q) { return Quat{-q.x, -q.y, -q.z, q.w}; }
// The unit quaternion of the rotation part of a float[12].  A matrix that is orthonormal only to float precision is first replaced
// by the rotation nearest to it - the orthogonal factor of its polar decomposition, by Newton's iteration X <- (X + X^-T) / 2, which
// converges quadratically from 1e-7 away - then Markley 2008: the largest of the trace and the diagonal picks the well-conditioned
// formula.
inline Quat from_tf(const float tf[12])
{
  double m[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      m[i][j] = tf[4 * i + j];
  for (int it = 0; it < 6; it++)
  {
    double c[3][3];  // cofactors: X^-T = c / det
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
      {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        c[i][j] = m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
      }
    const double det = m[0][0] * c[0][0] + m[0][1] * c[0][1] + m[0][2] * c[0][2];
    if (!(std::abs(det) > 1e-300))
      break;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
        m[i][j] = 0.5 * (m[i][j] + c[i][j] / det);
  }
  const double tr = m[0][0] + m[1][1] + m[2][2];
  double q[4];
  int c = 3;
  double best = tr;
  for (int i = 0; i < 3; i++)
    if (m[i][i] > best)
      best = m[i][i], c = i;
  if (c != 3)
  {
    const int i = c, j = (i + 1) % 3, k = (j + 1) % 3;
    q[i] = 1.0 - tr + 2.0 * m[i][i];
    q[j] = m[j][i] + m[i][j];
    q[k] = m[k][i] + m[i][k];
    q[3] = m[k][j] - m[j][k];
  }
  else
  {
    q[0] = m[2][1] - m[1][2];
    q[1] = m[0][2] - m[2][0];
    q[2] = m[1][0] - m[0][1];
    q[3] = 1.0 + tr;
  }
  const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  return Quat{q[0] / nrm, q[1] / nrm, q[2] / nrm, q[3] / nrm};
}
inline void to_matrix(const Quat& q, double R[3][3])
{
  const double x2 = q.x * q.x, y2 = q.y * q.y, z2 = q.z * q.z, w2 = q.w * q.w;
  const double xy = q.x * q.y, zw = q.z * q.w, xz = q.x * q.z, yw = q.y * q.w, yz = q.y * q.z, xw = q.x * q.w;
  R[0][0] = x2 - y2 - z2 + w2, R[0][1] = 2 * (xy - zw), R[0][2] = 2 * (xz + yw);
  R[1][0] = 2 * (xy + zw), R[1][1] = -x2 + y2 - z2 + w2, R[1][2] = 2 * (yz - xw);
  R[2][0] = 2 * (xz - yw), R[2][1] = 2 * (yz + xw), R[2][2] = -x2 - y2 + z2 + w2;
}
// log on the shortest arc: the rotation vector of q, angle in [0, pi]
inline void rotvec(Quat q, double v[3])
{
  if (q.w < 0)
    q = Quat{-q.x, -q.y, -q.z, -q.w};
  const double s = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
  const double angle = 2.0 * std::atan2(s, q.w);
  // angle / sin(angle / 2); its series where the angle is small
  const double k = angle <= 1e-3 ? 2.0 + angle * angle / 12.0 + 7.0 * angle * angle * angle * angle / 2880.0 : angle / std::sin(angle / 2.0);
  v[0] = k * q.x, v[1] = k * q.y, v[2] = k * q.z;
}
inline Quat from_rotvec(const double v[3])
{
  const double angle = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double a2 = angle * angle;
  const double k = angle <= 1e-3 ? 0.5 - a2 / 48.0 + a2 * a2 / 3840.0 : std::sin(angle / 2.0) / angle;
  return Quat{k * v[0], k * v[1], k * v[2], std::cos(angle / 2.0)};
}
}  // namespace colposes

extern "C" {

void vofod_default_params(vofod_static_params* sp, vofod_dyn_params* dp)
{
  if (sp)
  {
    *sp = vofod_static_params{};
    sp->voxel_size = 0.5f;                           // detection_params.yaml:17
    sp->score_init = -740.0f;                        // :21
    sp->background_sufficient_points_ratio = 0.15f;  // :9
    const float oo[3] = {40.0f, 20.0f, -1.25f}, os[3] = {120.0f, 100.0f, 25.0f};  // sim.yaml:8-15
    const float eo[3] = {0.09f, 0.0f, -0.75f}, es[3] = {2.5f, 2.5f, 1.6f};         // detection_params.yaml:76-83
    for (int a = 0; a < 3; a++)
    {
      sp->oparea_offset[a] = oo[a];
      sp->oparea_size[a] = os[a];
      sp->exclude_offset[a] = eo[a];
      sp->exclude_size[a] = es[a];
    }
    sp->sensor_hrays = 1024;  // sensors/os1-128.yaml:3-5
    sp->sensor_vrays = 128;
    sp->sensor_vfov = static_cast<float>(45.0 / 180.0 * M_PI);
    sp->max_batch_frames = 1;
  }
  if (dp)
  {
    *dp = vofod_dyn_params{};
    dp->ground_points_max_distance = 1.5;
    dp->output__position_sigma = 0.1;
    dp->voxel_map__scores__point = 0.0;
    dp->voxel_map__scores__unknown = -740.0;
    dp->voxel_map__scores__ray = -1000.0;
    dp->voxel_map__thresholds__apriori_map = 0.0;
    dp->voxel_map__thresholds__new_obstacles = -300.0;
    dp->voxel_map__thresholds__sure_obstacles = -0.1;
    dp->voxel_map__thresholds__frontiers = -750.0;
    dp->classification__min_points = 2;
    dp->classification__max_size = 3.0;
    dp->classification__max_distance = 50.0;
    dp->classification__max_explore_distance = 3.0;
    dp->raycast__pause = 0;
    dp->raycast__new_update_rule = 1;
    dp->raycast__max_distance = 20.0;
    dp->raycast__min_intensity = 0.0;
    dp->raycast__weight_coefficient = 0.003;
    dp->sepclusters__pause = 0;
    dp->sepclusters__max_bg_distance = 0.8;
    dp->sepclusters__min_sure_points = 24;
  }
}

int vofod_sim_lut(int32_t w, int32_t hh, float vfov, float* directions)
{
  if (w < 2 || hh < 2 || !directions)
    return VOFOD_ERR_INVALID_ARG;
  // initialize_sensor_lut_simulation vofod_nodelet.cpp:374-420
  const double yaw_step = (2.0 * M_PI - 0.0) / (w - 1);
  const double pitch_min = -vfov / 2.0, pitch_max = vfov / 2.0;
  const double pitch_step = (pitch_max - pitch_min) / (hh - 1);
  for (int row = 0; row < hh; row++)
    for (int col = 0; col < w; col++)
    {
      const double y = col * yaw_step + 0.0, p = row * pitch_step + pitch_min;
      float* d = directions + 3 * (static_cast<size_t>(row) * w + col);
      d[0] = static_cast<float>(std::cos(p) * std::cos(y));
      d[1] = static_cast<float>(std::cos(p) * std::sin(y));
      d[2] = static_cast<float>(std::sin(p));
    }
  return VOFOD_OK;
}

// initialize_sensor_lut (vofod_nodelet.cpp:358-372): the beam model of [3P] ouster::make_xyz_lut (ouster_client
// lidar_scan.cpp; the reference pins no version) followed by the nodelet's float cast and per-column normalisation.
// A beam of ring u at encoder column v leaves the lidar frame's z axis at radius n (= lidar_origin_to_beam_origin_mm) in the
// encoder direction and points along (azimuth, altitude) of its ring:
//   theta_enc = 2 pi - v 2 pi / w,   theta = theta_enc - azimuth[u],   phi = altitude[u]
//   dir = (cos theta cos phi, sin theta cos phi, sin phi),   off = ((cos theta_enc, sin theta_enc, 0) - dir) n
// both taken to the sensor frame by lidar_to_sensor (off also translated) and scaled by range_unit.
// Product implementation: ring constants first, then a plain structure-of-rows sweep (the oracle restates the library loop).
namespace
{
struct BeamRing
{
  double azimuth, cos_alt, sin_alt;
};
inline void to_sensor(const double rot[3][3], const double* trans, const double in[3], double out[3])
{
  // Eigen row-vector product with the transposed rotation block: ((x r0 + y r1) + z r2), then the translation
  for (int j = 0; j < 3; j++)
  {
    out[j] = (in[0] * rot[j][0] + in[1] * rot[j][1]) + in[2] * rot[j][2];
    if (trans)
      out[j] += trans[j];
  }
}
}  // namespace

int vofod_ouster_lut(int32_t w, int32_t hh, double range_unit, double lidar_origin_to_beam_origin_mm, const double* tf16, const double* azimuth_deg, const double* altitude_deg,
                       float* directions, float* offsets)
{
  if (w < 1 || hh < 1 || !azimuth_deg || !altitude_deg || !directions || !offsets)
    return VOFOD_ERR_INVALID_ARG;
  double rot[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, trans[3] = {0, 0, 0};
  if (tf16)
    for (int r = 0; r < 3; r++)
    {
      std::copy(tf16 + 4 * r, tf16 + 4 * r + 3, rot[r]);
      trans[r] = tf16[4 * r + 3];
    }
  std::vector<BeamRing> rings(hh);
  for (int u = 0; u < hh; u++)
  {
    const double alt = altitude_deg[u] * M_PI / 180.0;
    rings[u] = BeamRing{-azimuth_deg[u] * M_PI / 180.0, std::cos(alt), std::sin(alt)};
  }
  const double step = M_PI * 2.0 / w;
  float* dir_out = directions;
  float* off_out = offsets;
  for (int u = 0; u < hh; u++)
  {
    const BeamRing& ring = rings[u];
    for (int v = 0; v < w; v++, dir_out += 3, off_out += 3)
    {
      const double theta_enc = 2.0 * M_PI - (v * step), theta = theta_enc + ring.azimuth;
      const double dir[3] = {std::cos(theta) * ring.cos_alt, std::sin(theta) * ring.cos_alt, ring.sin_alt};
      const double off[3] = {(std::cos(theta_enc) - dir[0]) * lidar_origin_to_beam_origin_mm, (std::sin(theta_enc) - dir[1]) * lidar_origin_to_beam_origin_mm,
                             (-dir[2]) * lidar_origin_to_beam_origin_mm};
      double dir_s[3], off_s[3];
      to_sensor(rot, nullptr, dir, dir_s);
      to_sensor(rot, trans, off, off_s);
      const float d32[3] = {static_cast<float>(dir_s[0] * range_unit), static_cast<float>(dir_s[1] * range_unit), static_cast<float>(dir_s[2] * range_unit)};
      const float len = std::sqrt((d32[0] * d32[0] + d32[1] * d32[1]) + d32[2] * d32[2]);  // colwise().normalize() :369
      for (int j = 0; j < 3; j++)
      {
        dir_out[j] = d32[j] / len;
        off_out[j] = static_cast<float>(off_s[j] * range_unit);
      }
    }
  }
  return VOFOD_OK;
}

// load_mask (vofod_nodelet.cpp:506-560) after cv::imread.  `image` is the decoded w x h picture (row-major) or NULL when the
// file is missing or has the wrong size (then every ray is valid, :558).  With `mangle` (:527-541) the picture is rearranged
// into the staggered column-major order of the raw Ouster packets: pixel (u, v) lands at ((v + pixel_shift_by_row[u]) % w) * h + u.
// Product implementation: destination-major gather through the inverse shift (the oracle scatters source-major).
int vofod_mask_layout(const uint8_t* image, int32_t w, int32_t hh, const int32_t* pixel_shift_by_row, int32_t mangle, uint8_t* mask)
{
  if (w < 1 || hh < 1 || !mask)
    return VOFOD_ERR_INVALID_ARG;
  const size_t n_px = static_cast<size_t>(w) * hh;
  if (!image)
    std::memset(mask, 1, n_px);
  else if (!mangle)
    std::memcpy(mask, image, n_px);
  else
  {
    // source column of destination column 0, per ring: v = (vv - shift) mod w.  A negative shift makes the reference index
    // its vector out of range for the first columns (std::out_of_range): refused here.
    std::vector<int32_t> back(hh);
    for (int u = 0; u < hh; u++)
    {
      const int32_t sft = pixel_shift_by_row ? pixel_shift_by_row[u] : 0;
      if (sft < 0)
        return VOFOD_ERR_INVALID_ARG;
      back[u] = (w - sft % w) % w;
    }
    uint8_t* dst = mask;
    for (int32_t vv = 0; vv < w; vv++)
      for (int u = 0; u < hh; u++, dst++)
      {
        int32_t v = vv + back[u];
        if (v >= w)
          v -= w;
        *dst = image[static_cast<size_t>(u) * w + v];
      }
  }
  return VOFOD_OK;
}

// check_sensor_params (vofod_nodelet.cpp:1869-1917): the first valid pixel of an organised cloud (mask set, range != 0)
// must agree with the sensor model: direction of (point - beam offset) equal to the LUT direction within 1e-3, its length
// equal to range * 0.001 m within 1e-3, LUT direction of unit length within 1e-3.  *checked tells whether a valid pixel was
// found (m_sensor_params_checked); the return value is VOFOD_OK when the parameters fit (or nothing could be checked) and
// VOFOD_ERR_SIZE_MISMATCH - the reference's "parameters do not match the data" - otherwise.  Host arrays, w * h elements.
int vofod_check_sensor_params(const vofod_scan* scan, const float* lut_directions, const float* lut_offsets, const uint8_t* mask, int32_t* checked)
{
  if (!scan || !scan->x || !scan->y || !scan->z || !scan->range || !lut_directions || scan->memspace != VOFOD_MEM_HOST)
    return VOFOD_ERR_INVALID_ARG;
  if (checked)
    *checked = 0;
  const size_t n_px = static_cast<size_t>(scan->width) * scan->height;
  auto f32 = [&](const void* base, size_t i) {
    float v;
    std::memcpy(&v, static_cast<const char*>(base) + i * scan->stride_bytes, 4);
    return v;
  };
  auto u32 = [&](const void* base, size_t i) {
    uint32_t v;
    std::memcpy(&v, static_cast<const char*>(base) + i * scan->stride_bytes, 4);
    return v;
  };
  for (size_t idx = 0; idx < n_px; idx++)  // row-major: idx = row * width + col, rows outer as in the reference
  {
    const uint32_t range = u32(scan->range, idx);
    if ((mask && !mask[idx]) || range == 0)
      continue;
    const float* ld = lut_directions + 3 * idx;
    const float lut_dist = 0.001f * static_cast<float>(range);
    float rel[3] = {f32(scan->x, idx), f32(scan->y, idx), f32(scan->z, idx)};
    if (lut_offsets)
      for (int a = 0; a < 3; a++)
        rel[a] -= lut_offsets[3 * idx + a];
    const float pt_dist = std::sqrt((rel[0] * rel[0] + rel[1] * rel[1]) + rel[2] * rel[2]);
    float diff2 = 0.0f;
    for (int a = 0; a < 3; a++)
    {
      const float d = rel[a] / pt_dist - ld[a];
      diff2 += d * d;
    }
    const float lut_norm = std::sqrt((ld[0] * ld[0] + ld[1] * ld[1]) + ld[2] * ld[2]);
    const bool ok = !(std::sqrt(diff2) > 1e-3f) && !(std::fabs(pt_dist - lut_dist) > 1e-3f) && !(1.0f - lut_norm > 1e-3f);
    if (checked)
      *checked = 1;
    return ok ? VOFOD_OK : VOFOD_ERR_SIZE_MISMATCH;
  }
  return VOFOD_OK;
}

int vofod_column_poses(const float tf_begin[12], const float tf_end[12], const float tf_ref[12], const double* frac, int32_t n, float* col_tfs)
{
  using namespace colposes;
  if (!tf_begin || !tf_end || !tf_ref || !col_tfs || n <= 0)
    return VOFOD_ERR_INVALID_ARG;
  const Quat q0 = from_tf(tf_begin), q1 = from_tf(tf_end), qr_inv = conj(from_tf(tf_ref));
  double w[3], Rr_inv[3][3];
  rotvec(mul(conj(q0), q1), w);
  to_matrix(qr_inv, Rr_inv);
  for (int32_t m = 0; m < n; m++)
  {
    const double f = frac ? frac[m] : (n > 1 ? static_cast<double>(m) / (n - 1) : 0.0);
    const double fw[3] = {f * w[0], f * w[1], f * w[2]};
    double R[3][3];
    to_matrix(mul(qr_inv, mul(q0, from_rotvec(fw))), R);
    double d[3];
    for (int a = 0; a < 3; a++)
      d[a] = (static_cast<double>(tf_begin[4 * a + 3]) + f * (static_cast<double>(tf_end[4 * a + 3]) - tf_begin[4 * a + 3])) - tf_ref[4 * a + 3];
    float* out = col_tfs + 12 * static_cast<size_t>(m);
    for (int i = 0; i < 3; i++)
    {
      for (int j = 0; j < 3; j++)
        out[4 * i + j] = static_cast<float>(R[i][j]);
      out[4 * i + 3] = static_cast<float>(Rr_inv[i][0] * d[0] + Rr_inv[i][1] * d[1] + Rr_inv[i][2] * d[2]);
    }
  }
  return VOFOD_OK;
}

// ---- vofod_pose_lattice: host only, double throughout, each entry rounded to float once
int vofod_pose_lattice(const float tf[12], const float step[3], const int32_t n[3], float yaw_step, int32_t n_yaw, float* tfs_out)
{
  if (!tf || !step || !n || !tfs_out || n_yaw < 1 || !std::isfinite(yaw_step))
    return VOFOD_ERR_INVALID_ARG;
  uint64_t total = static_cast<uint64_t>(n_yaw);
  for (int a = 0; a < 3; a++)
  {
    if (n[a] < 1 || !std::isfinite(step[a]))
      return VOFOD_ERR_INVALID_ARG;
    total *= static_cast<uint64_t>(n[a]);  // (four factors below 2^31, checked after each: no overflow of 64 bits)
    if (total > 65535)
      return VOFOD_ERR_INVALID_ARG;
  }
  if (total > 65535)
    return VOFOD_ERR_INVALID_ARG;
  float* out = tfs_out;
  for (int32_t iyaw = 0; iyaw < n_yaw; iyaw++)
  {
    const double psi = (iyaw - (n_yaw - 1) / 2.0) * static_cast<double>(yaw_step);
    const double c = std::cos(psi), s = std::sin(psi);
    for (int32_t iz = 0; iz < n[2]; iz++)
      for (int32_t iy = 0; iy < n[1]; iy++)
        for (int32_t ix = 0; ix < n[0]; ix++, out += 12)
        {
          const int32_t i[3] = {ix, iy, iz};
          for (int j = 0; j < 3; j++)
          {
            out[j] = static_cast<float>(c * static_cast<double>(tf[j]) - s * static_cast<double>(tf[4 + j]));
            out[4 + j] = static_cast<float>(s * static_cast<double>(tf[j]) + c * static_cast<double>(tf[4 + j]));
            out[8 + j] = tf[8 + j];
          }
          for (int a = 0; a < 3; a++)
            out[4 * a + 3] = static_cast<float>(static_cast<double>(tf[4 * a + 3]) + (i[a] - (n[a] - 1) / 2.0) * static_cast<double>(step[a]));
        }
  }
  return VOFOD_OK;
}

// ---- row N3: the nodelet's outgoing messages in the ROS 1 wire format (little endian, strings and arrays prefixed with a
// uint32 length; std_msgs/Header = seq, stamp.sec, stamp.nsec, frame_id).  A ROS-free host (examples/vofod_replay.cpp)
// writes exactly the bytes a subscriber of the reference's topics receives.

// vofod/Detections (msgs/Detections.msg, msgs/Detection.msg:1-12; filled at vofod_nodelet.cpp:968-988)
int vofod_serialize_detections(const vofod_msg_header* header, const vofod_detection* dets, size_t n, uint8_t* buf, size_t cap, size_t* n_bytes)
{
  if (!header || (n && !dets) || !n_bytes)
    return VOFOD_ERR_INVALID_ARG;
  WireOut w{buf, cap};
  w.header(header);
  w.put(static_cast<uint32_t>(n));
  for (size_t i = 0; i < n; i++)
  {
    const vofod_detection& d = dets[i];
    w.put(d.id);
    w.put(d.confidence);
    w.put(d.n_points);
    for (int a = 0; a < 3; a++)
      w.put(d.position[a]);  // geometry_msgs/Point
    for (int a = 0; a < 9; a++)
      w.put(d.covariance[a]);
    w.put(d.detection_probability);
  }
  *n_bytes = w.n;
  return w.n > cap ? VOFOD_ERR_CAPACITY : VOFOD_OK;
}

// vofod/Status (msgs/Status.msg; vofod_nodelet.cpp:1379-1385)
int vofod_serialize_status(const vofod_msg_header* header, int detection_enabled, int detection_active, uint8_t* buf, size_t cap, size_t* n_bytes)
{
  if (!header || !n_bytes)
    return VOFOD_ERR_INVALID_ARG;
  WireOut w{buf, cap};
  w.header(header);
  w.put(static_cast<uint8_t>(detection_enabled ? 1 : 0));
  w.put(static_cast<uint8_t>(detection_active ? 1 : 0));
  *n_bytes = w.n;
  return w.n > cap ? VOFOD_ERR_CAPACITY : VOFOD_OK;
}

// vofod/ProfilingInfo (msgs/ProfilingInfo.msg; vofod_nodelet.cpp:2178-2201)
int vofod_serialize_profiling_info(uint32_t stamp_sec, uint32_t stamp_nsec, uint32_t routine_id, uint64_t event_sequence, uint8_t event_type, uint8_t* buf, size_t cap, size_t* n_bytes)
{
  if (!n_bytes)
    return VOFOD_ERR_INVALID_ARG;
  WireOut w{buf, cap};
  w.put(stamp_sec);
  w.put(stamp_nsec);
  w.put(routine_id);
  w.put(event_sequence);
  w.put(event_type);
  *n_bytes = w.n;
  return w.n > cap ? VOFOD_ERR_CAPACITY : VOFOD_OK;
}

// load_cloud pc_loader.cpp:17-90 (host I/O helper, no device work)
int vofod_load_cloud(const char* filename, float* xyz, size_t cap, size_t* n_out)
{
  if (!filename || !n_out)
    return VOFOD_ERR_INVALID_ARG;
  std::ifstream fs(filename, std::ios::binary);
  if (!fs.is_open() || fs.fail())
    return VOFOD_ERR_INVALID_ARG;
  const std::string name(filename);
  const bool pts_file = name.size() >= 4 && name.compare(name.size() - 4, 4, ".pts") == 0;
  std::string line;
  if (pts_file)
    std::getline(fs, line);  // first line of a .pts file is the point count (:36-41)
  size_t n = 0;
  while (std::getline(fs, line))
  {
    // tokens are maximal runs of characters other than tab, CR, space (:61-63); blank lines are skipped (:56)
    const char* s = line.c_str();
    const char* tok[3];
    int nt = 0;
    size_t i = 0;
    const size_t L = line.size();
    auto is_ws = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\v' || c == '\f'; };
    while (i < L && nt < 3)
    {
      while (i < L && is_ws(s[i]))
        i++;
      if (i >= L)
        break;
      tok[nt++] = s + i;
      while (i < L && !(s[i] == ' ' || s[i] == '\t' || s[i] == '\r'))
        i++;
    }
    if (nt < 3)
      continue;  // :65-69
    if (xyz && n < cap)
      for (int c = 0; c < 3; c++)
        xyz[3 * n + c] = static_cast<float>(std::atof(tok[c]));
    n++;
  }
  *n_out = n;
  return n > cap ? VOFOD_ERR_CAPACITY : VOFOD_OK;
}

}  // extern "C"
