// The handle-free entry points (api_host.h) on the CPU: every function of the header on small inputs and at its edges, every
// caller buffer allocated to the byte, so that the host compiler's sanitizers see any access beside one.
//   api_host_check      exit status 0 and "api_host_check: ok", or the first failed line and exit status 1
// Includes api_host.h and nothing else of the library (tests/test_api_host_cpu.py builds it with the host compiler and
// -fsanitize=address,undefined, and runs it).
#include <unistd.h>

#include <cstdio>
#include <memory>

#include "api_host.h"

#define CHECK(cond)                                                        \
  do                                                                       \
  {                                                                        \
    if (!(cond))                                                           \
    {                                                                      \
      std::fprintf(stderr, "api_host_check:%d: %s\n", __LINE__, #cond);   \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// a buffer of exactly n elements on the heap: the sanitizer's red zones start at its ends
template <class T>
static std::unique_ptr<T[]> exact(size_t n)
{
  return std::unique_ptr<T[]>(new T[n]());
}

static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

static void check_default_params()
{
  vofod_static_params sp;
  vofod_dyn_params dp;
  vofod_default_params(&sp, &dp);
  CHECK(sp.voxel_size == 0.5f && sp.sensor_hrays == 1024 && sp.sensor_vrays == 128 && sp.max_batch_frames == 1);
  CHECK(dp.sepclusters__min_sure_points == 24 && dp.raycast__weight_coefficient == 0.003);
  vofod_default_params(&sp, nullptr);
  vofod_default_params(nullptr, &dp);
  vofod_default_params(nullptr, nullptr);
}

static void check_luts()
{
  const int w = 5, h = 3;
  auto dirs = exact<float>(3 * w * h), offs = exact<float>(3 * w * h);
  CHECK(vofod_sim_lut(w, h, 0.5f, dirs.get()) == VOFOD_OK);
  for (int i = 0; i < w * h; i++)
    CHECK(near(std::hypot(std::hypot(dirs[3 * i], dirs[3 * i + 1]), dirs[3 * i + 2]), 1.0, 1e-6));
  CHECK(near(dirs[0], std::cos(-0.25), 1e-7) && near(dirs[2], std::sin(-0.25), 1e-7));  // row 0, column 0: yaw 0, pitch -vfov / 2
  CHECK(vofod_sim_lut(1, h, 0.5f, dirs.get()) == VOFOD_ERR_INVALID_ARG && vofod_sim_lut(w, h, 0.5f, nullptr) == VOFOD_ERR_INVALID_ARG);
  auto two = exact<float>(3 * 2 * 2);
  CHECK(vofod_sim_lut(2, 2, 0.5f, two.get()) == VOFOD_OK);

  const double az[h] = {-1.5, 0.0, 1.5}, alt[h] = {10.0, 0.0, -10.0};
  const double tf[16] = {-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 36.18, 0, 0, 0, 1};
  CHECK(vofod_ouster_lut(w, h, 0.001, 15.806, tf, az, alt, dirs.get(), offs.get()) == VOFOD_OK);
  for (int i = 0; i < w * h; i++)
  {
    CHECK(near(std::hypot(std::hypot(dirs[3 * i], dirs[3 * i + 1]), dirs[3 * i + 2]), 1.0, 1e-6));
    CHECK(std::fabs(offs[3 * i + 2]) > 0.03);  // (the translation, in metres)
  }
  // ring 1 (no azimuth offset, no altitude) at column 0: the encoder looks along +x of the lidar, -x of the sensor, and the beam
  // starts on its axis
  CHECK(near(dirs[3 * w], -1.0, 1e-6) && near(offs[3 * w], 0.0, 1e-9) && near(offs[3 * w + 2], 0.03618, 1e-7));
  CHECK(vofod_ouster_lut(w, h, 0.001, 0.0, nullptr, az, alt, dirs.get(), offs.get()) == VOFOD_OK);
  CHECK(near(dirs[3 * w], 1.0, 1e-6) && offs[3 * w + 2] == 0.0f);
  auto one_d = exact<float>(3), one_o = exact<float>(3);
  CHECK(vofod_ouster_lut(1, 1, 0.001, 15.806, tf, az, alt, one_d.get(), one_o.get()) == VOFOD_OK);
  CHECK(vofod_ouster_lut(0, 1, 0.001, 0.0, tf, az, alt, one_d.get(), one_o.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_ouster_lut(w, h, 0.001, 0.0, tf, nullptr, alt, dirs.get(), offs.get()) == VOFOD_ERR_INVALID_ARG);
}

static void check_mask_layout()
{
  const int w = 6, h = 4;
  auto img = exact<uint8_t>(w * h), mask = exact<uint8_t>(w * h);
  for (int i = 0; i < w * h; i++)
    img[i] = static_cast<uint8_t>(i + 1);
  // shifts below, at and beyond the width
  const int32_t shift[h] = {0, 5, 6, 2 * w + 3};
  CHECK(vofod_mask_layout(img.get(), w, h, shift, 1, mask.get()) == VOFOD_OK);
  for (int u = 0; u < h; u++)
    for (int v = 0; v < w; v++)
      CHECK(mask[((v + shift[u]) % w) * h + u] == img[u * w + v]);
  CHECK(vofod_mask_layout(img.get(), w, h, nullptr, 1, mask.get()) == VOFOD_OK);  // no shifts: the plain transpose
  for (int u = 0; u < h; u++)
    for (int v = 0; v < w; v++)
      CHECK(mask[v * h + u] == img[u * w + v]);
  const int32_t negative[h] = {0, 1, -1, 0};
  CHECK(vofod_mask_layout(img.get(), w, h, negative, 1, mask.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_mask_layout(img.get(), w, h, negative, 0, mask.get()) == VOFOD_OK);  // (not mangled: the shifts are not read)
  CHECK(std::memcmp(mask.get(), img.get(), w * h) == 0);
  CHECK(vofod_mask_layout(nullptr, w, h, shift, 1, mask.get()) == VOFOD_OK);
  for (int i = 0; i < w * h; i++)
    CHECK(mask[i] == 1);
  auto one = exact<uint8_t>(1);
  CHECK(vofod_mask_layout(img.get(), 1, 1, shift + 3, 1, one.get()) == VOFOD_OK && one[0] == img[0]);
  CHECK(vofod_mask_layout(img.get(), 0, h, shift, 1, mask.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_mask_layout(img.get(), w, h, shift, 1, nullptr) == VOFOD_ERR_INVALID_ARG);
}

static void check_sensor_params()
{
  // points of 48 bytes (x, y, z, an unused word, the range, padding), the only valid pixel the last one
  const int w = 4, h = 3, n = w * h;
  const size_t stride = 48;
  auto cloud = exact<char>(n * stride);
  auto dirs = exact<float>(3 * n), offs = exact<float>(3 * n);
  auto mask = exact<uint8_t>(n);
  CHECK(vofod_sim_lut(w, h, 0.6f, dirs.get()) == VOFOD_OK);
  for (int i = 0; i < 3 * n; i++)
    offs[i] = 0.01f * static_cast<float>(i % 3);
  std::memset(mask.get(), 1, n);
  const int last = n - 1;
  const uint32_t range = 2500;
  float p[3];
  for (int a = 0; a < 3; a++)
    p[a] = dirs[3 * last + a] * 2.5f + offs[3 * last + a];
  std::memcpy(cloud.get() + last * stride, p, 12);
  std::memcpy(cloud.get() + last * stride + 16, &range, 4);
  vofod_scan scan{};
  scan.x = reinterpret_cast<const float*>(cloud.get());
  scan.y = reinterpret_cast<const float*>(cloud.get() + 4);
  scan.z = reinterpret_cast<const float*>(cloud.get() + 8);
  scan.range = reinterpret_cast<const uint32_t*>(cloud.get() + 16);
  scan.stride_bytes = stride;
  scan.width = w;
  scan.height = h;
  scan.memspace = VOFOD_MEM_HOST;
  int32_t checked = -1;
  CHECK(vofod_check_sensor_params(&scan, dirs.get(), offs.get(), mask.get(), &checked) == VOFOD_OK && checked == 1);
  CHECK(vofod_check_sensor_params(&scan, dirs.get(), offs.get(), nullptr, nullptr) == VOFOD_OK);
  CHECK(vofod_check_sensor_params(&scan, dirs.get(), nullptr, mask.get(), &checked) == VOFOD_ERR_SIZE_MISMATCH && checked == 1);  // (the offsets are missing: 1.7 cm off)
  mask[last] = 0;
  CHECK(vofod_check_sensor_params(&scan, dirs.get(), offs.get(), mask.get(), &checked) == VOFOD_OK && checked == 0);
  mask[last] = 1;
  p[0] += 0.01f;
  std::memcpy(cloud.get() + last * stride, p, 12);
  CHECK(vofod_check_sensor_params(&scan, dirs.get(), offs.get(), mask.get(), &checked) == VOFOD_ERR_SIZE_MISMATCH && checked == 1);
  scan.memspace = VOFOD_MEM_DEVICE;
  CHECK(vofod_check_sensor_params(&scan, dirs.get(), offs.get(), mask.get(), &checked) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_check_sensor_params(nullptr, dirs.get(), offs.get(), mask.get(), &checked) == VOFOD_ERR_INVALID_ARG);
}

// the pose with rotation `angle` about z and the translation t
static void pose_z(double angle, float tx, float ty, float tz, float tf[12])
{
  const float c = static_cast<float>(std::cos(angle)), s = static_cast<float>(std::sin(angle));
  const float m[12] = {c, -s, 0, tx, s, c, 0, ty, 0, 0, 1, tz};
  std::memcpy(tf, m, sizeof(m));
}

static void check_column_poses()
{
  float ident[12], begin[12], end[12];
  pose_z(0.0, 0, 0, 0, ident);
  pose_z(0.3, 1, 2, 3, begin);
  pose_z(0.5, 2, 2, 3, end);
  // one column: the begin pose seen from the reference, here the begin pose itself - the identity
  auto one = exact<float>(12);
  CHECK(vofod_column_poses(begin, end, begin, nullptr, 1, one.get()) == VOFOD_OK);
  for (int k = 0; k < 12; k++)
    CHECK(near(one[k], ident[k], 1e-6));
  // a half turn about z over three columns: the ends are the given poses, the middle a quarter turn (either way round)
  const int n = 3;
  auto cols = exact<float>(12 * n);
  pose_z(M_PI, 4, 0, 0, end);
  CHECK(vofod_column_poses(ident, end, ident, nullptr, n, cols.get()) == VOFOD_OK);
  for (int k = 0; k < 12; k++)
    CHECK(near(cols[k], ident[k], 1e-6) && near(cols[24 + k], end[k], 1e-6));
  const float* mid = cols.get() + 12;
  CHECK(near(mid[0], 0.0, 1e-6) && near(std::fabs(mid[1]), 1.0, 1e-6) && near(mid[1], -mid[4], 1e-6) && near(mid[5], 0.0, 1e-6) && near(mid[10], 1.0, 1e-6));
  CHECK(near(mid[3], 2.0, 1e-6) && mid[7] == 0.0f && mid[11] == 0.0f);
  // fractions of the caller's, beyond [0, 1] too
  const double frac[2] = {-0.5, 1.5};
  auto two = exact<float>(24);
  pose_z(0.2, 1, 0, 0, end);
  CHECK(vofod_column_poses(ident, end, ident, frac, 2, two.get()) == VOFOD_OK);
  CHECK(near(two[0], std::cos(-0.1), 1e-6) && near(two[3], -0.5, 1e-6) && near(two[12], std::cos(0.3), 1e-6) && near(two[15], 1.5, 1e-6));
  CHECK(vofod_column_poses(ident, end, ident, nullptr, 0, two.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_column_poses(ident, end, nullptr, nullptr, 2, two.get()) == VOFOD_ERR_INVALID_ARG);
}

static void check_pose_lattice()
{
  float tf[12];
  pose_z(0.3, 1, 2, 3, tf);
  const float step[3] = {0.25f, 0.5f, 1.0f};
  // an exact allocation of 3 * 3 * 1 * 3 poses: x fastest, the yaw slowest, the centre candidate is tf itself
  const int32_t n[3] = {3, 3, 1};
  auto out = exact<float>(27 * 12);
  CHECK(vofod_pose_lattice(tf, step, n, 0.1f, 3, out.get()) == VOFOD_OK);
  for (int k = 0; k < 12; k++)
    CHECK(out[13 * 12 + k] == tf[k]);
  CHECK(near(out[3], 0.75, 1e-6) && near(out[12 + 3], 1.0, 1e-6) && near(out[7], 1.5, 1e-6) && near(out[3 * 12 + 7], 2.0, 1e-6) && out[11] == 3.0f);
  CHECK(near(out[0], std::cos(0.3 - 0.1), 1e-6) && near(out[4], std::sin(0.3 - 0.1), 1e-6) && near(out[26 * 12], std::cos(0.3 + 0.1), 1e-6));
  CHECK(out[9 * 12 + 3] == out[3] && out[18 * 12 + 7] == out[7]);  // (the yaw turns about the sensor's own origin: t stays)
  // refusals: a count below 1, a product above 65 535 (also one that would overflow 32 bits), a step that is not finite, a NULL
  const int32_t zero[3] = {3, 0, 1}, many[3] = {256, 256, 1}, huge[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
  const float bad[3] = {0.25f, NAN, 1.0f};
  auto none = exact<float>(1);
  CHECK(vofod_pose_lattice(tf, step, zero, 0.0f, 1, none.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_pose_lattice(tf, step, many, 0.0f, 1, none.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_pose_lattice(tf, step, huge, 0.0f, INT32_MAX, none.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_pose_lattice(tf, step, n, 0.0f, 0, none.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_pose_lattice(tf, bad, n, 0.0f, 1, none.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_pose_lattice(tf, step, n, INFINITY, 1, none.get()) == VOFOD_ERR_INVALID_ARG);
  CHECK(vofod_pose_lattice(tf, step, n, 0.0f, 1, nullptr) == VOFOD_ERR_INVALID_ARG);
}

// a serialiser at every capacity that matters: size query (no buffer), one byte short, exact
template <class F>
static std::unique_ptr<uint8_t[]> serialised(size_t want, F&& call)
{
  size_t n = 0;
  CHECK(call(nullptr, 0, &n) == VOFOD_ERR_CAPACITY && n == want);
  CHECK(call(nullptr, want, &n) == VOFOD_OK && n == want);  // (nothing to write to: only the size)
  auto small = exact<uint8_t>(want - 1);
  n = 0;
  CHECK(call(small.get(), want - 1, &n) == VOFOD_ERR_CAPACITY && n == want);
  auto buf = exact<uint8_t>(want);
  n = 0;
  CHECK(call(buf.get(), want, &n) == VOFOD_OK && n == want);
  CHECK(std::memcmp(small.get(), buf.get(), 4) == 0);  // (what fits is written)
  CHECK(call(buf.get(), want, nullptr) == VOFOD_ERR_INVALID_ARG);
  return buf;
}

template <class T>
static T at(const uint8_t* p, size_t off)
{
  T v;
  std::memcpy(&v, p + off, sizeof(T));
  return v;
}

static void check_serialisers()
{
  const vofod_msg_header hd{7, 100, 200, "map"}, anonymous{8, 1, 2, nullptr};
  const size_t H = 4 + 4 + 4 + 4 + 3, D = 4 + 8 + 8 + 3 * 8 + 9 * 8 + 8;
  vofod_detection dets[2] = {};
  dets[0].id = 11;
  dets[0].confidence = 0.5;
  dets[0].n_points = 1ull << 40;
  dets[1].id = 12;
  dets[1].position[2] = -3.0;
  dets[1].covariance[8] = 9.0;
  dets[1].detection_probability = 0.25;
  auto b = serialised(H + 4 + 2 * D, [&](uint8_t* buf, size_t cap, size_t* n) { return vofod_serialize_detections(&hd, dets, 2, buf, cap, n); });
  CHECK(at<uint32_t>(b.get(), 0) == 7 && at<uint32_t>(b.get(), 4) == 100 && at<uint32_t>(b.get(), 8) == 200 && at<uint32_t>(b.get(), 12) == 3 && std::memcmp(b.get() + 16, "map", 3) == 0);
  CHECK(at<uint32_t>(b.get(), H) == 2 && at<uint32_t>(b.get(), H + 4) == 11 && at<double>(b.get(), H + 8) == 0.5 && at<uint64_t>(b.get(), H + 16) == 1ull << 40);
  const size_t d1 = H + 4 + D;
  CHECK(at<uint32_t>(b.get(), d1) == 12 && at<double>(b.get(), d1 + 20 + 16) == -3.0 && at<double>(b.get(), d1 + 44 + 64) == 9.0 && at<double>(b.get(), d1 + 116) == 0.25);
  serialised(H - 3 + 4, [&](uint8_t* buf, size_t cap, size_t* n) { return vofod_serialize_detections(&anonymous, nullptr, 0, buf, cap, n); });
  size_t n = 0;
  CHECK(vofod_serialize_detections(&hd, nullptr, 1, nullptr, 0, &n) == VOFOD_ERR_INVALID_ARG && vofod_serialize_detections(nullptr, dets, 1, nullptr, 0, &n) == VOFOD_ERR_INVALID_ARG);
  b = serialised(H + 2, [&](uint8_t* buf, size_t cap, size_t* n) { return vofod_serialize_status(&hd, 5, 0, buf, cap, n); });
  CHECK(b[H] == 1 && b[H + 1] == 0);
  CHECK(vofod_serialize_status(nullptr, 1, 1, nullptr, 0, &n) == VOFOD_ERR_INVALID_ARG);
  b = serialised(21, [&](uint8_t* buf, size_t cap, size_t* n) { return vofod_serialize_profiling_info(1, 2, 3, 1ull << 33, 4, buf, cap, n); });
  CHECK(at<uint32_t>(b.get(), 8) == 3 && at<uint64_t>(b.get(), 12) == 1ull << 33 && b[20] == 4);
}

static void check_load_cloud()
{
  char path[] = "/tmp/api_host_check_XXXXXX.pts";
  const int fd = mkstemps(path, 4);
  CHECK(fd >= 0);
  // the count line, a point, a blank line, a short line, CR line ends, tabs, a line of blanks, a fourth column, no newline at the end
  const char text[] = "5\n1 2 3\n\n4 5\n6.5\t7.5  8.5\r\n\r\n   \t \n-1e2 0.25 9 77\r\n10 11 12";
  CHECK(write(fd, text, sizeof(text) - 1) == static_cast<ssize_t>(sizeof(text) - 1));
  close(fd);
  const float want[12] = {1, 2, 3, 6.5f, 7.5f, 8.5f, -100, 0.25f, 9, 10, 11, 12};
  size_t n = 0;
  CHECK(vofod_load_cloud(path, nullptr, 0, &n) == VOFOD_ERR_CAPACITY && n == 4);
  auto all = exact<float>(12);
  CHECK(vofod_load_cloud(path, all.get(), 4, &n) == VOFOD_OK && n == 4 && std::memcmp(all.get(), want, sizeof(want)) == 0);
  auto some = exact<float>(6);  // a capacity below the count: the first two points, the count of all
  CHECK(vofod_load_cloud(path, some.get(), 2, &n) == VOFOD_ERR_CAPACITY && n == 4 && std::memcmp(some.get(), want, 24) == 0);
  CHECK(vofod_load_cloud(path, all.get(), 4, nullptr) == VOFOD_ERR_INVALID_ARG && vofod_load_cloud(nullptr, all.get(), 4, &n) == VOFOD_ERR_INVALID_ARG);
  unlink(path);
  CHECK(vofod_load_cloud(path, all.get(), 4, &n) == VOFOD_ERR_INVALID_ARG);  // (no such file)
  // another suffix: no count line
  char xyz[] = "/tmp/api_host_check_XXXXXX.xyz";
  const int fd2 = mkstemps(xyz, 4);
  CHECK(fd2 >= 0);
  CHECK(write(fd2, text, sizeof(text) - 1) == static_cast<ssize_t>(sizeof(text) - 1));
  close(fd2);
  CHECK(vofod_load_cloud(xyz, nullptr, 0, &n) == VOFOD_ERR_CAPACITY && n == 4);  // ("5" is a short line)
  unlink(xyz);
}

int main()
{
  check_default_params();
  check_luts();
  check_mask_layout();
  check_sensor_params();
  check_column_poses();
  check_pose_lattice();
  check_serialisers();
  check_load_cloud();
  std::puts("api_host_check: ok");
  return 0;
}
