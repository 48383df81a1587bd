// vofod_map_distance and vofod_map_match_field (included by vofod_hip.hip after api_match.h): the squared distance, in voxels, from
// every voxel of the map to the nearest occupied one, and candidate poses scored by such a field.  Contract: include/vofod.h, MAP
// DISTANCE; kernels and the account of their launches: map_distance.h.  The scan's refusals, its live list, the occupancy image and the
// scoring launch with its read-back are api_match.h's (match_refusal, match_live_list, match_bits, match_score).
#pragma once

#include "api_match.h"

namespace
{

// a list of `count` rows, tiles or planes as gridDim.y x gridDim.z: the kernels fold it back and leave beyond `count`
inline void fold_grid(uint32_t count, uint32_t& gy, uint32_t& gz)
{
  gy = std::min(count, vmd::MD_MAX_GRID);
  gz = (count + gy - 1) / gy;
}

}  // namespace

extern "C" {

int vofod_map_distance(vofod_handle* h, float threshold, int32_t radius, uint16_t* d2, size_t n, int32_t memspace)
{
  if (!h || !d2 || std::isnan(threshold) || radius < 1 || radius > static_cast<int32_t>(vmd::MD_MAX_RADIUS) || (memspace != VOFOD_MEM_HOST && memspace != VOFOD_MEM_DEVICE))
    return VOFOD_ERR_INVALID_ARG;
  const bool on_device = memspace == VOFOD_MEM_DEVICE;
  if (on_device && (reinterpret_cast<uintptr_t>(d2) & 1))
    return VOFOD_ERR_INVALID_ARG;
  if (n != h->mg.n)
    return VOFOD_ERR_SIZE_MISMATCH;
  ApiLock lock(h);
  // as vofod_map_render: reads the voxel map only, in a workspace of its own: admitted with tickets in flight and with a raycast or
  // sepclusters pass pending
  VCHK(admit(h, NEEDS_NOTHING));
  vmd::Workspace& w = h->dist;
  HIPCHK(w.d_a.reserve(n));
  HIPCHK(w.d_b.reserve(n));
  const uint32_t sx = static_cast<uint32_t>(h->mg.sx), sy = static_cast<uint32_t>(h->mg.sy), sz = static_cast<uint32_t>(h->mg.sz), R = static_cast<uint32_t>(radius);
  uint32_t gy = 0, gz = 0;
  // ---- the occupancy image of this threshold
  VCHK(match_bits(h, threshold));
  // ---- along x: bits -> A
  fold_grid(sy * sz, gy, gz);
  KLAUNCH_AS(h, "k_dist_x", vmd::k_dist_x, dim3((sx + 255) / 256, gy, gz), dim3(256), static_cast<const unsigned long long*>(h->match.d_bits.p), sx, sy * sz, R, w.d_a.p);
  HIPCHK(hipGetLastError());
  // ---- along y: A -> B, by the instantiation whose LDS tile has rows for R either side
  const uint32_t y_tiles = (sy + vmd::MD_TY - 1) / vmd::MD_TY;
  fold_grid(y_tiles * sz, gy, gz);
  auto along_y = R <= 16 ? vmd::k_dist_y<16> : R <= 64 ? vmd::k_dist_y<64> : vmd::k_dist_y<vmd::MD_MAX_RADIUS>;
  KLAUNCH_AS(h, "k_dist_y", along_y, dim3((sx + vmd::MD_TX - 1) / vmd::MD_TX, gy, gz), dim3(256), static_cast<const uint16_t*>(w.d_a.p), sx, sy, y_tiles, y_tiles * sz, R, w.d_b.p);
  HIPCHK(hipGetLastError());
  // ---- along z: B -> the caller's device buffer, or A again, which is copied out
  const uint64_t plane = static_cast<uint64_t>(sx) * sy;
  fold_grid(sz, gy, gz);
  KLAUNCH_AS(h, "k_dist_z", vmd::k_dist_z, dim3(static_cast<uint32_t>((plane + 255) / 256), gy, gz), dim3(256), static_cast<const uint16_t*>(w.d_b.p), plane, sz, R, on_device ? d2 : w.d_a.p);
  HIPCHK(hipGetLastError());
  if (!on_device)
    HIPCHK(hipMemcpyAsync(d2, w.d_a, n * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // (the call's only one: a host field arrives with it)
  return VOFOD_OK;
}

int vofod_map_match_field(vofod_handle* h, const vofod_scan* scan, const float* tfs, size_t n_poses, const uint16_t* d2, size_t n, int32_t field_memspace, uint32_t near2,
                          uint32_t outside_cost, uint32_t* counts, uint64_t* cost, int32_t* best)
{
  if (!d2 || !cost || (field_memspace != VOFOD_MEM_HOST && field_memspace != VOFOD_MEM_DEVICE) || outside_cost > 65535u)
    return VOFOD_ERR_INVALID_ARG;
  const bool field_on_device = field_memspace == VOFOD_MEM_DEVICE;
  if (field_on_device && (reinterpret_cast<uintptr_t>(d2) & 1))
    return VOFOD_ERR_INVALID_ARG;
  VCHK(match_refusal(h, scan, tfs, n_poses, counts));
  if (n != h->mg.n)
    return VOFOD_ERR_SIZE_MISMATCH;
  ApiLock lock(h);
  // as vofod_map_match - and the voxel map is not even read: the field and the scan are
  VCHK(admit(h, NEEDS_NOTHING));
  const uint32_t n_px = static_cast<uint32_t>(h->sp.sensor_hrays) * static_cast<uint32_t>(h->sp.sensor_vrays);
  const uint32_t np = static_cast<uint32_t>(n_poses);
  vmm::Workspace& w = h->match;  // (the scan's staging, the live list, the candidates and the counts: one call at a time holds the lock)
  vmd::Workspace& d = h->dist;
  HIPCHK(d.d_cost.reserve(n_poses));
  const uint16_t* field = d2;
  if (!field_on_device)
  {
    HIPCHK(d.d_field.reserve(n));
    HIPCHK(hipMemcpyAsync(d.d_field, d2, n * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    field = d.d_field.p;
  }
  HIPCHK(hipMemsetAsync(d.d_cost, 0, n_poses * sizeof(unsigned long long), h->stream));
  // ---- the live list
  VCHK(match_live_list(h, w, *scan, tfs, n_poses));
  // ---- counts and sums
  VCHK(match_score(h, "k_match_field", vmm::LookField{field, near2, d.d_cost.p}, n_poses));
  const uint32_t n_live = w.h_out[0];
  int32_t best_k = 0;
  for (uint32_t k = 0; k < np; k++)
  {
    const uint32_t* c = w.h_out.data() + vmm::MM_HEAD + 4 * static_cast<size_t>(k);
    uint32_t* o = counts + 4 * static_cast<size_t>(k);
    o[VOFOD_FIELD_SKIPPED] = n_px - n_live;  // the same for every candidate
    o[VOFOD_FIELD_OUTSIDE] = c[1];
    o[VOFOD_FIELD_NEAR] = c[3];
    o[VOFOD_FIELD_FAR] = n_live - c[1] - c[3];
    cost[k] = d.h_cost[k] + static_cast<uint64_t>(outside_cost) * c[1];
    if (cost[k] < cost[best_k])
      best_k = static_cast<int32_t>(k);
  }
  if (best)
    *best = best_k;
  return VOFOD_OK;
}

}  // extern "C"
