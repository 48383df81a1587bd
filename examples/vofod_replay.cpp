// vofod_replay — ROS-free host driver with the nodelet's three thread roles.
//
// What vofod_nodelet.cpp does around the hot path, with nothing but the C-ABI of include/vofod.h:
//   main loop      = cloud_callback / processMsg (:878-986): one vofod_process_scan per organised cloud, detections out;
//   raycast thread = raycast_cloud (:1392-1605), spawned per scan unless one is still running (:951-957): begin,
//                    wait for a detection iteration (condition variable, 800 ms timeout :1530-1537), finish;
//   sepclusters    = the timer callback updateSeparatedBGClusters (:1124-1276), every `sepclusters_period`.
// The clouds come from a small synthetic world (ground plane, two static boxes, one flying box on a circle) ray-cast
// through the simulated sensor LUT (initialize_sensor_lut_simulation :374-420 via vofod_sim_lut), exactly the shape
// the nodelet receives from the Ouster driver: organised h x w xyz + range in mm, zeros for no return.
//
//   vofod_replay [--scans N] [--rows H] [--cols W] [--voxel S] [--apriori file.xyz] [--period-ms P]
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../include/vofod.h"

namespace
{

struct Box
{
  float lo[3], hi[3];
};

// nearest positive hit of a ray with the ground plane z = 0 (inside +-60 m) and a list of boxes; inf when none
float cast(const float o[3], const float d[3], const std::vector<Box>& boxes)
{
  float best = INFINITY;
  if (d[2] < 0)
  {
    const float t = -o[2] / d[2];
    const float gx = o[0] + t * d[0], gy = o[1] + t * d[1];
    if (t > 0 && std::fabs(gx) < 60 && std::fabs(gy) < 60)
      best = t;
  }
  for (const Box& b : boxes)
  {
    float tmin = -INFINITY, tmax = INFINITY;
    for (int a = 0; a < 3; a++)
    {
      const float inv = 1.0f / d[a];
      float t1 = (b.lo[a] - o[a]) * inv, t2 = (b.hi[a] - o[a]) * inv;
      if (t1 > t2)
        std::swap(t1, t2);
      tmin = std::max(tmin, t1);
      tmax = std::min(tmax, t2);
    }
    if (tmax >= std::max(tmin, 0.0f) && tmin > 0 && tmin < best)
      best = tmin;
  }
  return best;
}

struct Cloud
{
  std::vector<float> x, y, z, intensity;
  std::vector<uint32_t> range;
  float tf[12];
};

}  // namespace

int main(int argc, char** argv)
{
  int n_scans = 40, rows = 32, cols = 1024, period_ms = 0, extents = 0, pixels = 0, render = 0, agree = 0, match = 0, field = 0;
  float voxel = 0.5f;
  std::string apriori;
  for (int i = 1; i + 1 < argc; i += 2)
  {
    const std::string k = argv[i];
    if (k == "--scans")
      n_scans = std::atoi(argv[i + 1]);
    else if (k == "--rows")
      rows = std::atoi(argv[i + 1]);
    else if (k == "--cols")
      cols = std::atoi(argv[i + 1]);
    else if (k == "--voxel")
      voxel = static_cast<float>(std::atof(argv[i + 1]));
    else if (k == "--apriori")
      apriori = argv[i + 1];
    else if (k == "--period-ms")
      period_ms = std::atoi(argv[i + 1]);
    else if (k == "--extents")  // 1: after each scan, the member count and the AABB of every detection (vofod_detection_points)
      extents = std::atoi(argv[i + 1]);
    else if (k == "--pixels")  // 1: after each scan, the number of raw returns of every detection and their (row, col) rectangle (vofod_detection_pixels)
      pixels = std::atoi(argv[i + 1]);
    else if (k == "--render")  // 1: after the run, the map as the sensor sees it from the last pose (vofod_map_render): the counts of the four kinds of pixel
      render = std::atoi(argv[i + 1]);
    else if (k == "--agree")  // 1: before each scan's update, the scan against the map as it stands (vofod_map_render_scans): the counts of the seven verdicts
      agree = std::atoi(argv[i + 1]);
    else if (k == "--match")  // 1: before each scan's update, a 5 x 5 x 1 lattice of poses one voxel apart with 3 yaws around the scan's pose, scored against the map (vofod_map_match)
      match = std::atoi(argv[i + 1]);
    else if (k == "--field")  // 1: every 10th scan the distance field of the map (vofod_map_distance, radius 8); before each scan's update --match's lattice scored by it (vofod_map_match_field) beside vofod_map_match
      field = std::atoi(argv[i + 1]);
  }
  const float vfov = 45.0f * 3.14159265f / 180.0f;
  vofod_static_params sp;
  vofod_dyn_params dp;
  vofod_default_params(&sp, &dp);  // detection_params.yaml + sim.yaml defaults
  sp.voxel_size = voxel;
  sp.sensor_hrays = cols;
  sp.sensor_vrays = rows;
  sp.sensor_vfov = vfov;
  vofod_handle* h = nullptr;
  if (vofod_create(&sp, &dp, &h) != VOFOD_OK)
  {
    std::fprintf(stderr, "vofod_create failed\n");
    return 2;
  }
  std::vector<float> lut(3 * static_cast<size_t>(rows) * cols);
  vofod_sim_lut(cols, rows, vfov, lut.data());

  // static world: also the apriori background (initialize_apriori_map) unless a cloud file is given
  const std::vector<Box> statics = {{{8, -6, 0}, {12, -2, 5}}, {{-14, 5, 0}, {-9, 11, 3}}};
  if (!apriori.empty())
  {
    const float t[3] = {0, 0, 0}, c[3] = {0, 0, 0};
    size_t nl = 0, nv = 0;
    const int r = vofod_ingest_apriori(h, apriori.c_str(), t, 0.0, c, &nl, &nv);
    std::printf("apriori map: %zu points -> %zu voxels (status %d)\n", nl, nv, r);
  }
  else
  {
    std::vector<float> xyz;
    const float s = voxel;
    for (float gx = -40; gx < 40; gx += s)
      for (float gy = -40; gy < 40; gy += s)
        xyz.insert(xyz.end(), {gx + s / 2, gy + s / 2, s / 4});
    for (const Box& b : statics)
      for (float bx = b.lo[0] + s / 2; bx < b.hi[0]; bx += s)
        for (float by = b.lo[1] + s / 2; by < b.hi[1]; by += s)
          for (float bz = b.lo[2] + s / 2; bz < b.hi[2]; bz += s)
            if (bx - b.lo[0] < s || b.hi[0] - bx < s || by - b.lo[1] < s || b.hi[1] - by < s || b.hi[2] - bz < s)
              xyz.insert(xyz.end(), {bx, by, bz});
    vofod_load_apriori(h, xyz.data(), xyz.size() / 3);
    std::printf("apriori map: %zu synthetic background points\n", xyz.size() / 3);
  }

  // ---- the two background roles
  std::mutex mtx;
  std::condition_variable detection_cv;  // m_detection_cv (:951)
  std::atomic<bool> raycast_running{false}, stop{false};
  std::atomic<int> n_raycasts{0}, n_raycast_timeouts{0}, n_sep{0};
  std::vector<std::thread> raycast_threads;
  auto raycast_role = [&](std::shared_ptr<Cloud> c) {
    vofod_scan scan{c->x.data(), c->y.data(), c->z.data(), c->intensity.data(), c->range.data(), 4, cols, rows, VOFOD_MEM_HOST, 0.0};
    if (vofod_raycast_begin(h, &scan, c->tf) == VOFOD_OK)
    {
      {
        std::unique_lock<std::mutex> lck(mtx);
        detection_cv.wait_for(lck, std::chrono::milliseconds(800));  // :1530-1537
      }
      const int r = vofod_raycast_finish(h);
      n_raycasts++;
      if (r == VOFOD_ERR_RAYCAST_NO_DETECTION)
        n_raycast_timeouts++;
    }
    raycast_running = false;
  };
  std::thread sep_thread([&] {
    const auto period = std::chrono::milliseconds(100);  // sepclusters__period (detection_params.yaml:3)
    while (!stop)
    {
      std::this_thread::sleep_for(period_ms > 0 ? period : std::chrono::milliseconds(5));
      int sure = 0;
      if (vofod_sepclusters_begin(h, &sure) == VOFOD_OK && sure)
        vofod_sepclusters_finish(h);
      n_sep++;
    }
  });

  // ---- main role: one cloud per iteration
  size_t total_det = 0, det_on_target = 0, det_off_target = 0, msg_bytes = 0;
  float last_tf[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4};
  std::vector<uint8_t> msg_buf;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint16_t> d2;  // --field: the distance field of the map as it stood at the last scan that is a multiple of ten
  for (int k = 0; k < n_scans; k++)
  {
    auto c = std::make_shared<Cloud>();
    const size_t n = static_cast<size_t>(rows) * cols;
    c->x.assign(n, 0), c->y.assign(n, 0), c->z.assign(n, 0), c->intensity.assign(n, 100.0f), c->range.assign(n, 0);
    const float yaw = 0.02f * k;
    const float o[3] = {0.5f * std::cos(0.1f * k), 0.5f * std::sin(0.1f * k), 4.0f};  // sensor 4 m above ground
    const float R[9] = {std::cos(yaw), -std::sin(yaw), 0, std::sin(yaw), std::cos(yaw), 0, 0, 0, 1};
    for (int r = 0; r < 3; r++)
    {
      for (int cc = 0; cc < 3; cc++)
        c->tf[4 * r + cc] = R[3 * r + cc];
      c->tf[4 * r + 3] = o[r];
    }
    std::vector<Box> boxes = statics;
    const float a = 0.15f * k;  // the flying target: 0.5 m cube on a circle of 6 m radius, 3 m above ground
    boxes.push_back({{6 * std::cos(a) - 0.25f, 6 * std::sin(a) - 0.25f, 2.75f}, {6 * std::cos(a) + 0.25f, 6 * std::sin(a) + 0.25f, 3.25f}});
    for (size_t i = 0; i < n; i++)
    {
      const float* ds = &lut[3 * i];
      const float d[3] = {R[0] * ds[0] + R[1] * ds[1] + R[2] * ds[2], R[3] * ds[0] + R[4] * ds[1] + R[5] * ds[2], R[6] * ds[0] + R[7] * ds[1] + R[8] * ds[2]};
      const float t = cast(o, d, boxes);
      if (!(t > 0.3f && t < 100.0f))
        continue;
      c->range[i] = static_cast<uint32_t>(std::lround(t * 1000.0f));
      const float rm = static_cast<float>(c->range[i]) * 0.001f;
      c->x[i] = ds[0] * rm, c->y[i] = ds[1] * rm, c->z[i] = ds[2] * rm;
    }
    std::copy(c->tf, c->tf + 12, last_tf);
    vofod_scan scan{c->x.data(), c->y.data(), c->z.data(), c->intensity.data(), c->range.data(), 4, cols, rows, VOFOD_MEM_HOST, 0.1 * k};
    if (agree)
    {
      // which share of this scan agrees with the map under this pose, and how many returns lie in space the map holds free -
      // asked BEFORE the scan updates the map; a voxel of tolerance, the counts alone (no image is read back)
      uint32_t counts[8];
      if (vofod_map_render_scans(h, &scan, c->tf, 1, static_cast<float>(dp.voxel_map__thresholds__new_obstacles), static_cast<float>(dp.raycast__max_distance), voxel, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, counts, VOFOD_MEM_HOST) == VOFOD_OK)
        std::printf("scan %3d against the map: %u none, %u agree, %u empty, %u nearer, %u through, %u missing, %u beyond\n", k, counts[VOFOD_VERDICT_NONE], counts[VOFOD_VERDICT_AGREES],
                    counts[VOFOD_VERDICT_EMPTY], counts[VOFOD_VERDICT_NEARER], counts[VOFOD_VERDICT_THROUGH], counts[VOFOD_VERDICT_MISSING], counts[VOFOD_VERDICT_BEYOND]);
      else
        std::fprintf(stderr, "map_render_scans: %s\n", vofod_last_error_string(h));
    }
    if (match)
    {
      // where do this scan's returns land under 75 poses around the one it came with - asked BEFORE the scan updates the map.  The
      // centre of the lattice (candidate 37) is the scan's own pose: best == 37 says that no neighbour explains the scan better.
      const float step[3] = {voxel, voxel, voxel};
      const int32_t cnt[3] = {5, 5, 1};
      float tfs[75 * 12];
      uint32_t counts[75 * 4];
      int32_t best = -1;
      if (vofod_pose_lattice(c->tf, step, cnt, 0.01f, 3, tfs) == VOFOD_OK &&
          vofod_map_match(h, &scan, tfs, 75, static_cast<float>(dp.voxel_map__thresholds__new_obstacles), counts, &best) == VOFOD_OK)
        std::printf("scan %3d matched under 75 poses: best %d (%u occupied, %u free, %u outside), the scan's own pose %u occupied; %u pixels skipped\n", k, best,
                    counts[4 * best + VOFOD_MATCH_OCCUPIED], counts[4 * best + VOFOD_MATCH_FREE], counts[4 * best + VOFOD_MATCH_OUTSIDE], counts[4 * 37 + VOFOD_MATCH_OCCUPIED],
                    counts[VOFOD_MATCH_SKIPPED]);
      else
        std::fprintf(stderr, "map_match: %s\n", vofod_last_error_string(h));
    }
    if (field)
    {
      // the same 75 poses scored by the distance to the map's surfaces: a cost with a slope where vofod_map_match's count is a step.
      // The field is rebuilt every 10th scan - a field a few scans old is what a matcher uses - and kept by the caller.  THIS EXAMPLE HAS NO
      // HIP OF ITS OWN, so it keeps the field in host memory, and every vofod_map_match_field below copies all of it to the device
      // again (2 bytes per voxel per scan).  A caller that can hold device memory passes a device buffer with VOFOD_MEM_DEVICE to
      // both calls: it is then written and read in place, and nothing is copied.
      const float step[3] = {voxel, voxel, voxel};
      const int32_t cnt[3] = {5, 5, 1};
      const float thr = static_cast<float>(dp.voxel_map__thresholds__new_obstacles);
      float tfs[75 * 12];
      uint32_t counts[75 * 4], occupied[75 * 4];
      uint64_t cost[75];
      int32_t best = -1, best_count = -1;
      if (d2.empty())
      {
        vofod_status_info si;
        vofod_get_status(h, &si);
        d2.resize(static_cast<size_t>(si.map_size[0]) * si.map_size[1] * si.map_size[2]);
      }
      int st_f = VOFOD_OK;
      if (k % 10 == 0)
        st_f = vofod_map_distance(h, thr, 8, d2.data(), d2.size(), VOFOD_MEM_HOST);
      if (st_f == VOFOD_OK && vofod_pose_lattice(c->tf, step, cnt, 0.01f, 3, tfs) == VOFOD_OK &&
          vofod_map_match_field(h, &scan, tfs, 75, d2.data(), d2.size(), VOFOD_MEM_HOST, 0, 64, counts, cost, &best) == VOFOD_OK &&
          vofod_map_match(h, &scan, tfs, 75, thr, occupied, &best_count) == VOFOD_OK)
        std::printf("scan %3d scored by the field of scan %d under 75 poses: best %d (cost %llu, %u near, %u far, %u outside), the scan's own pose costs %llu; vofod_map_match's best %d\n", k,
                    k - k % 10, best, static_cast<unsigned long long>(cost[best]), counts[4 * best + VOFOD_FIELD_NEAR], counts[4 * best + VOFOD_FIELD_FAR], counts[4 * best + VOFOD_FIELD_OUTSIDE],
                    static_cast<unsigned long long>(cost[37]), best_count);
      else
        std::fprintf(stderr, "map_distance / map_match_field: %s\n", vofod_last_error_string(h));
    }
    vofod_detection dets[64];
    size_t n_det = 0;
    const int st = vofod_process_scan(h, &scan, c->tf, VOFOD_SCAN_DEFAULT, dets, 64, &n_det, nullptr);
    if (st != VOFOD_OK && st != VOFOD_ERR_CAPACITY)
    {
      std::fprintf(stderr, "process_scan: status %d (%s)\n", st, vofod_last_error_string(h));
      stop = true;
      break;
    }
    if (extents && n_det)
    {
      // what detection_t::aabb and cluster_t::pc hold in the nodelet (:110-130): asked for before anything else takes the workspace
      size_t n_ext = 0, n_pts = 0;
      if (vofod_detection_points(h, VOFOD_POINTS_SYNC, nullptr, 0, &n_ext, nullptr, nullptr, 0, &n_pts, VOFOD_MEM_HOST) == VOFOD_OK)
      {
        std::vector<vofod_detection_extent> ext(n_ext);
        std::vector<vofod_point_xyzr> pts(n_pts);
        if (vofod_detection_points(h, VOFOD_POINTS_SYNC, ext.data(), n_ext, &n_ext, pts.data(), nullptr, n_pts, &n_pts, VOFOD_MEM_HOST) == VOFOD_OK)
          for (const vofod_detection_extent& e : ext)
          {
            uint64_t hits = 0;
            for (uint32_t i = e.first; i < e.first + e.count; i++)
              hits += pts[i].range;
            std::printf("scan %3d detection id %u extent: %u voxels (%llu returns), aabb (%.2f, %.2f, %.2f) - (%.2f, %.2f, %.2f)\n", k, e.id, e.count, static_cast<unsigned long long>(hits),
                        e.aabb_min[0], e.aabb_min[1], e.aabb_min[2], e.aabb_max[0], e.aabb_max[1], e.aabb_max[2]);
          }
      }
    }
    if (pixels && n_det)
    {
      // the sensor returns behind every detection: their pixels in the organised scan, for a camera cue or a tracker's re-fit
      size_t n_span = 0, n_px = 0;
      if (vofod_detection_pixels(h, VOFOD_POINTS_SYNC, nullptr, 0, &n_span, nullptr, nullptr, nullptr, 0, &n_px, VOFOD_MEM_HOST) == VOFOD_OK)
      {
        std::vector<vofod_detection_span> span(n_span);
        std::vector<uint32_t> px(n_px);
        if (vofod_detection_pixels(h, VOFOD_POINTS_SYNC, span.data(), n_span, &n_span, px.data(), nullptr, nullptr, n_px, &n_px, VOFOD_MEM_HOST) == VOFOD_OK)
          for (const vofod_detection_span& sdet : span)
          {
            // (the rectangle does not know that column 0 follows column cols - 1: a target across the seam spans the whole width)
            uint32_t r0 = rows, r1 = 0, c0 = cols, c1 = 0;
            for (uint32_t i = sdet.first; i < sdet.first + sdet.count; i++)
            {
              const uint32_t r = px[i] / static_cast<uint32_t>(cols), cc = px[i] % static_cast<uint32_t>(cols);
              r0 = std::min(r0, r), r1 = std::max(r1, r), c0 = std::min(c0, cc), c1 = std::max(c1, cc);
            }
            std::printf("scan %3d detection id %u pixels: %u returns, rows %u-%u, cols %u-%u\n", k, sdet.id, sdet.count, r0, r1, c0, c1);
          }
      }
      else
        std::fprintf(stderr, "detection_pixels: %s\n", vofod_last_error_string(h));
    }
    detection_cv.notify_one();  // :951
    if (!raycast_running.exchange(true))  // :953-957
      raycast_threads.emplace_back(raycast_role, c);
    for (size_t i = 0; i < std::min<size_t>(n_det, 64); i++)
    {
      std::printf("scan %3d detection id %u conf %.3f at (%.2f, %.2f, %.2f), %llu points\n", k, dets[i].id, dets[i].confidence, dets[i].position[0], dets[i].position[1],
                  dets[i].position[2], static_cast<unsigned long long>(dets[i].n_points));
      // result check: the only thing flying in this world is the 0.5 m cube (OBB centre of its visible faces: within 0.6 m)
      const double e[3] = {dets[i].position[0] - 6 * std::cos(a), dets[i].position[1] - 6 * std::sin(a), dets[i].position[2] - 3.0};
      (std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) <= 0.6 ? det_on_target : det_off_target)++;
    }
    total_det += n_det;
    {
      // what m_pub_detections / m_pub_status would carry (:968-989, :1379-1385), byte for byte in the ROS 1 wire format
      const vofod_msg_header mh{static_cast<uint32_t>(k), static_cast<uint32_t>(k / 10), static_cast<uint32_t>((k % 10) * 100000000), "world_origin"};
      size_t nb = 0;
      msg_buf.resize(4096);
      if (vofod_serialize_detections(&mh, dets, std::min<size_t>(n_det, 64), msg_buf.data(), msg_buf.size(), &nb) == VOFOD_OK)
        msg_bytes += nb;
      vofod_status_info st_now;
      vofod_get_status(h, &st_now);
      if (vofod_serialize_status(&mh, 1, st_now.background_pts_sufficient && st_now.sure_background_sufficient, msg_buf.data(), msg_buf.size(), &nb) == VOFOD_OK)
        msg_bytes += nb;
    }
    if (period_ms > 0)
      std::this_thread::sleep_for(std::chrono::milliseconds(period_ms));
  }
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  stop = true;
  sep_thread.join();
  for (auto& t : raycast_threads)
    t.join();
  vofod_status_info si;
  vofod_get_status(h, &si);
  std::printf("done: %d scans in %.3f s (%.1f scans/s incl. synthesis), detections %zu, detection_its %d, raycasts %d (timeouts %d), sepclusters passes %d\n", n_scans, secs, n_scans / secs,
              total_det, si.detection_its, n_raycasts.load(), n_raycast_timeouts.load(), n_sep.load());
  std::printf("check: %zu detections on the flying target, %zu elsewhere; %zu message bytes serialised\n", det_on_target, det_off_target, msg_bytes);
  if (render)
  {
    // the expected range image of the last pose: what the map, as the run left it, says the sensor should see (background above
    // thresholds/new_obstacles); `range` is a range image for vofod_process_scan / vofod_raycast_begin as it stands
    const size_t n = static_cast<size_t>(rows) * cols;
    std::vector<uint32_t> range(n);
    std::vector<uint8_t> what(n);
    if (vofod_map_render(h, last_tf, 1, static_cast<float>(dp.voxel_map__thresholds__new_obstacles), static_cast<float>(dp.raycast__max_distance), range.data(), nullptr, what.data(), nullptr,
                         VOFOD_MEM_HOST) == VOFOD_OK)
    {
      size_t count[4] = {0, 0, 0, 0};
      for (size_t i = 0; i < n; i++)
        count[what[i] & 3]++;
      std::printf("render of the last pose: %zu hits, %zu rays ended inside the map, %zu left it, %zu not cast\n", count[VOFOD_RENDER_HIT], count[VOFOD_RENDER_END], count[VOFOD_RENDER_LEFT],
                  count[VOFOD_RENDER_NOT_CAST]);
    }
    else
      std::fprintf(stderr, "map_render: %s\n", vofod_last_error_string(h));
  }
  vofod_destroy(h);
  return det_off_target > det_on_target ? 3 : 0;  // (the target is found in most scans once the map has settled; strays are rare)
}
