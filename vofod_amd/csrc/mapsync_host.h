// Host side of the map snapshots (kernels and wire header: mapsync.h; contract: include/vofod.h): vofod_map_export,
// vofod_map_apply and the RCCL broadcast vofod_broadcast_map.  Included by vofod_hip.hip after api_gate.h, driver_aux.h, api_maps.h
// (pick_map) and collective.h.
#pragma once
#include <atomic>
#include <random>

namespace
{

constexpr int MS_MAPS_ALL = (1 << VOFOD_MAP_VOXELS) | (1 << VOFOD_MAP_FLAGS) | (1 << VOFOD_MAP_RAYCAST);

inline uint32_t ms_init_bits(const vofod_handle* h, int m)
{
  const float v = m == VOFOD_MAP_VOXELS ? h->sp.score_init : 0.0f;
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}

// a fresh 64-bit generation: random per process, never 0 (0 = "no chain" / the base of a full snapshot)
uint64_t ms_fresh_gen()
{
  static std::atomic<uint64_t> ctr{0};
  static const uint64_t seed = [] {
    std::random_device rd;
    return (static_cast<uint64_t>(rd()) << 32) ^ rd() ^ static_cast<uint64_t>(std::chrono::steady_clock::now().time_since_epoch().count());
  }();
  uint64_t z = seed + (ctr.fetch_add(1) + 1) * 0x9E3779B97F4A7C15ull;  // splitmix64
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z ? z : 1;
}

int ms_ensure(vofod_handle* h)
{
  MapSyncState& s = h->msync;
  if (s.h_small)  // (allocated last: it stands for all five)
    return VOFOD_OK;
  const uint64_t nt = (h->mg.n + vms::MS_TILE - 1) / vms::MS_TILE;
  s.ntiles = static_cast<uint32_t>(nt);
  HIPCHK(s.d_tiles.alloc(3 * (nt + 1)));
  HIPCHK(s.d_prefix.alloc(3 * (nt + 1)));
  HIPCHK(s.d_bsum.alloc(nt / vr::GS_EPB + 2));
  HIPCHK(s.d_small.alloc(16));
  HIPCHK(s.h_small.alloc(16));
  return VOFOD_OK;
}

int ms_ensure_wire(vofod_handle* h, size_t bytes)
{
  MapSyncState& s = h->msync;
  if (bytes > s.d_wire.n)
    HIPCHK(s.d_wire.alloc(std::max(bytes + bytes / 4 + 4096, 2 * s.d_wire.n)));  // (geometric: a stream of growing deltas reallocates rarely)
  return VOFOD_OK;
}

// count pass + scan of map m: tile counts, their prefix and the total (d_small[slot]) on the stream
int ms_count_map(vofod_handle* h, int m, bool full, const uint32_t* d_map, int slot)
{
  MapSyncState& s = h->msync;
  const uint32_t nt = s.ntiles;
  uint32_t* tiles = s.d_tiles + static_cast<size_t>(m) * (nt + 1);
  uint32_t* prefix = s.d_prefix + static_cast<size_t>(m) * (nt + 1);
  const dim3 grid(std::min<uint32_t>(nt, vms::MS_GRID));
  if (full)
    KLAUNCH_AS(h, "k_ms_count", vms::k_ms_count<true>, grid, dim3(vms::MS_THREADS), d_map, nullptr, h->mg.n, ms_init_bits(h, m), nt, tiles);
  else
    KLAUNCH_AS(h, "k_ms_count", vms::k_ms_count<false>, grid, dim3(vms::MS_THREADS), d_map, s.d_shadow[m], h->mg.n, 0u, nt, tiles);
  return gscan(h, tiles, nt, prefix, s.d_bsum, s.d_small + slot);
}

// records per selected map of an export of kind `full` (0 for maps not selected)
int ms_count(vofod_handle* h, int maps, bool full, uint64_t nrec[3])
{
  int r;
  for (int m = 0; m < 3; m++)
  {
    nrec[m] = 0;
    if ((maps >> m & 1) && (r = ms_count_map(h, m, full, reinterpret_cast<const uint32_t*>(pick_map(h, m)), m)) != VOFOD_OK)
      return r;
  }
  HIPCHK(hipMemcpyAsync(h->msync.h_small, h->msync.d_small, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int m = 0; m < 3; m++)
    if (maps >> m & 1)
      nrec[m] = h->msync.h_small[m];
  return VOFOD_OK;
}

// the export behind vofod_map_export / vofod_broadcast_map: counts, and - unless size_only - the records and header written to
// the device buffer d_dst (cap bytes; nullptr: the handle's staging buffer d_wire, grown to fit).  *n_bytes = size of the
// snapshot in every case.  Nothing but the counts is touched before the capacity check.
int ms_export_locked(vofod_handle* h, int maps, int kind, uint8_t* d_dst, size_t cap, bool size_only, size_t* n_bytes)
{
  MapSyncState& s = h->msync;
  const bool full = kind == VOFOD_SNAPSHOT_FULL;
  if (!full && (s.chain_gen == 0 || s.chain_mask != maps))
  {
    h->err = "map export: no full snapshot of this maps mask was exported before (a delta needs a chain)";
    return VOFOD_ERR_DELTA_BASE;
  }
  if (h->mg.n > 0xffffffffull)
  {
    h->err = "map export: the map has more voxels than 32-bit record indices reach";
    return VOFOD_ERR_INDEX_OVERFLOW;
  }
  VCHK(ms_ensure(h));
  uint64_t nrec[3];
  VCHK(ms_count(h, maps, full, nrec));
  const size_t bytes = sizeof(vms::WireHeader) + 8 * (nrec[0] + nrec[1] + nrec[2]);
  *n_bytes = bytes;
  if (size_only)
    return VOFOD_OK;
  if (cap < bytes)
  {
    h->err = "map export: buffer too small (n_bytes holds the size)";
    return VOFOD_ERR_CAPACITY;
  }
  if (!d_dst)
  {
    VCHK(ms_ensure_wire(h, bytes));
    d_dst = s.d_wire;
  }
  if (full)  // the shadows are allocated on the first export of their map (4 * M bytes each)
    for (int m = 0; m < 3; m++)
      if ((maps >> m & 1) && !s.d_shadow[m])
        HIPCHK(s.d_shadow[m].alloc(h->mg.n));
  vms::WireHeader hd{};
  hd.magic = vms::MS_MAGIC;
  hd.version = vms::MS_VERSION;
  hd.maps = static_cast<uint32_t>(maps);
  hd.kind = static_cast<uint32_t>(kind);
  hd.map_size[0] = h->mg.sx;
  hd.map_size[1] = h->mg.sy;
  hd.map_size[2] = h->mg.sz;
  for (int a = 0; a < 3; a++)
    hd.map_offset[a] = h->mg.off[a];
  hd.voxel_size = h->sp.voxel_size;
  hd.score_init = h->sp.score_init;
  hd.base_gen = full ? 0 : s.chain_gen;
  hd.new_gen = ms_fresh_gen();
  hd.detection_its = h->detection_its;
  hd.last_detection_id = h->last_detection_id;
  hd.background_pts_sufficient = h->background_pts_sufficient;
  hd.sure_background_sufficient = h->sure_background_sufficient;
  hd.raycast_pending = h->raycast_pending;
  hd.raycast_start_its = h->raycast_start_its;
  // a pending exact pass whose units travel: byte 0 of the reserved block holds S + 1 (include/vofod.h, EXACT RAYCAST ACCUMULATION)
  if (h->raycast_pending && h->ray_pass_exact && (maps >> VOFOD_MAP_RAYCAST & 1))
    hd.zero[0] = static_cast<uint8_t>(h->ray_log2_units + 1);
  size_t off = sizeof(vms::WireHeader);
  const uint32_t nt = s.ntiles;
  const dim3 grid(std::min<uint32_t>(nt, vms::MS_GRID));
  for (int m = 0; m < 3; m++)
  {
    if (!(maps >> m & 1))
      continue;
    hd.n_records[m] = nrec[m];
    uint32_t* idx = reinterpret_cast<uint32_t*>(d_dst + off);
    uint32_t* bits = idx + nrec[m];
    const uint32_t* map = reinterpret_cast<const uint32_t*>(pick_map(h, m));
    const uint32_t* tiles = s.d_tiles + static_cast<size_t>(m) * (nt + 1);
    const uint32_t* prefix = s.d_prefix + static_cast<size_t>(m) * (nt + 1);
    if (full)
      KLAUNCH_AS(h, "k_ms_emit", vms::k_ms_emit<true>, grid, dim3(vms::MS_THREADS), map, s.d_shadow[m], h->mg.n, ms_init_bits(h, m), nt, tiles, prefix, idx, bits);
    else if (nrec[m])
      KLAUNCH_AS(h, "k_ms_emit", vms::k_ms_emit<false>, grid, dim3(vms::MS_THREADS), map, s.d_shadow[m], h->mg.n, 0u, nt, tiles, prefix, idx, bits);
    off += 8 * nrec[m];
  }
  HIPCHK(hipMemcpyAsync(d_dst, &hd, sizeof(hd), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // (hd is on this frame)
  s.chain_gen = hd.new_gen;
  s.chain_mask = maps;
  return VOFOD_OK;
}

// the apply behind vofod_map_apply / vofod_broadcast_map: hd = the header (host copy), d_buf = the whole snapshot on the device
int ms_apply_locked(vofod_handle* h, const vms::WireHeader& hd, const uint8_t* d_buf, size_t n_bytes)
{
  MapSyncState& s = h->msync;
  const int maps = static_cast<int>(hd.maps);
  const bool full = hd.kind == VOFOD_SNAPSHOT_FULL;
  int r;
  VCHK(ms_ensure(h));
  // records: strictly ascending and inside the map, checked on the device before anything is written
  HIPCHK(hipMemsetAsync(s.d_small + 3, 0, sizeof(uint32_t), h->stream));
  size_t off = sizeof(vms::WireHeader);
  const uint32_t* rec[3][2] = {};
  for (int m = 0; m < 3; m++)
  {
    const uint32_t cnt = static_cast<uint32_t>(hd.n_records[m]);
    rec[m][0] = reinterpret_cast<const uint32_t*>(d_buf + off);
    rec[m][1] = rec[m][0] + cnt;
    off += 8 * static_cast<size_t>(cnt);
    if (cnt)
      KLAUNCH(h, vms::k_ms_check, dim3(std::min<uint32_t>((cnt + 255) / 256, vms::MS_GRID)), dim3(256), rec[m][0], cnt, h->mg.n, s.d_small + 3);
  }
  HIPCHK(hipMemcpyAsync(s.h_small + 3, s.d_small + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (s.h_small[3])
  {
    h->err = "map apply: record indices not strictly ascending or outside the map";
    return VOFOD_ERR_INVALID_ARG;
  }
  (void)n_bytes;
  for (int m = 0; m < 3; m++)
  {
    if (!(maps >> m & 1))
      continue;
    float* map = pick_map(h, m);
    if (full && (r = fill_map(h, map, m == VOFOD_MAP_VOXELS ? h->sp.score_init : 0.0f)) != VOFOD_OK)
      return r;
    const uint32_t cnt = static_cast<uint32_t>(hd.n_records[m]);
    if (cnt)
      KLAUNCH(h, vms::k_ms_scatter, dim3(std::min<uint32_t>((cnt + 255) / 256, vms::MS_GRID)), dim3(256), rec[m][0], rec[m][1], cnt, reinterpret_cast<uint32_t*>(map));
  }
  // handle state carried by the header
  h->detection_its = hd.detection_its;
  h->last_detection_id = hd.last_detection_id;
  h->background_pts_sufficient = hd.background_pts_sufficient != 0;
  h->sure_background_sufficient = hd.sure_background_sufficient != 0;
  const int ray_maps = (1 << VOFOD_MAP_FLAGS) | (1 << VOFOD_MAP_RAYCAST);
  if ((maps & ray_maps) == ray_maps)
  {
    h->raycast_pending = hd.raycast_pending != 0;
    h->raycast_start_its = hd.raycast_start_its;
    if (h->raycast_pending)
    {
      // raycast_finish asks whether any ray added a length (k_raycast's hit word): the raycast map is non-zero somewhere
      HIPCHK(hipMemsetAsync(h->d_counter + 1, 0, sizeof(unsigned long long), h->stream));
      if (full)
      {
        if (hd.n_records[VOFOD_MAP_RAYCAST])
          HIPCHK(hipMemsetAsync(h->d_counter + 1, 1, 1, h->stream));
      }
      else
      {
        VCHK(ms_count_map(h, VOFOD_MAP_RAYCAST, true, reinterpret_cast<const uint32_t*>(h->d_ray.p), 4));
        HIPCHK(hipMemcpyAsync(h->d_counter + 1, s.d_small + 4, sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
      }
    }
  }
  if (maps & (1 << VOFOD_MAP_RAYCAST))
  {
    h->ray_pass_exact = h->raycast_pending && hd.zero[0] != 0;  // (the representation travels with the bits; S was checked)
    h->ray_dirty = true;  // (the next raycast_begin clears the accumulator unless a finish sweeps it)
  }
  h->sep_pending = false;  // a sepclusters pass of this handle belongs to the map it replaced
  forget_detections(h);  // ... and so do the detections vofod_detection_points would answer for
  h->mapbits_valid = false;  // occupancy image, dilated image and nVoxelsOver are rebuilt on next use (as after write_map)
  HIPCHK(hipStreamSynchronize(h->stream));
  s.applied_gen = hd.new_gen;
  s.applied_mask = maps;
  return VOFOD_OK;
}

// header checks of vofod_map_apply, in order: format (INVALID_ARG), geometry (SIZE_MISMATCH), chain (DELTA_BASE)
int ms_check_header(vofod_handle* h, const vms::WireHeader& hd, size_t n_bytes)
{
  if (hd.magic != vms::MS_MAGIC || hd.version != vms::MS_VERSION || hd.kind > 1 || hd.maps == 0 || (hd.maps & ~static_cast<uint32_t>(MS_MAPS_ALL)))
  {
    h->err = "map apply: not a map snapshot (magic, version, kind or maps mask)";
    return VOFOD_ERR_INVALID_ARG;
  }
  uint64_t total = 0;
  for (int m = 0; m < 3; m++)
  {
    if ((!(hd.maps >> m & 1) && hd.n_records[m]) || hd.n_records[m] > 0xffffffffull)
    {
      h->err = "map apply: record counts do not match the maps mask";
      return VOFOD_ERR_INVALID_ARG;
    }
    total += hd.n_records[m];
  }
  // byte 0 of the reserved block: S + 1 of a pending exact raycast pass that travels with its units, else 0; the other 15 are zero
  bool reserved_ok = hd.zero[0] == 0 || (hd.raycast_pending != 0 && (hd.maps >> VOFOD_MAP_RAYCAST & 1) && hd.zero[0] <= vr::RX_MAX_LOG2 + 1);
  for (size_t k = 1; k < sizeof(hd.zero); k++)
    reserved_ok &= hd.zero[k] == 0;
  if (!reserved_ok)
  {
    h->err = "map apply: reserved header bytes are not zero (byte 0 may hold S + 1 of a pending exact raycast pass)";
    return VOFOD_ERR_INVALID_ARG;
  }
  if (n_bytes != sizeof(vms::WireHeader) + 8 * total)
  {
    h->err = "map apply: length does not match the header's record counts";
    return VOFOD_ERR_INVALID_ARG;
  }
  bool same = hd.map_size[0] == h->mg.sx && hd.map_size[1] == h->mg.sy && hd.map_size[2] == h->mg.sz;
  for (int a = 0; a < 3; a++)
    same &= std::memcmp(&hd.map_offset[a], &h->mg.off[a], 4) == 0;
  same &= std::memcmp(&hd.voxel_size, &h->sp.voxel_size, 4) == 0 && std::memcmp(&hd.score_init, &h->sp.score_init, 4) == 0;
  if (!same)
  {
    h->err = "map apply: map geometry (size, offset, voxel size, score_init) differs from this handle's";
    return VOFOD_ERR_SIZE_MISMATCH;
  }
  if (hd.zero[0] != 0 && static_cast<int>(hd.zero[0]) - 1 != h->ray_log2_units)
  {
    h->err = "map apply: the pending exact raycast pass counts 2^" + std::to_string(static_cast<int>(hd.zero[0]) - 1) + " units per metre, this handle 2^" + std::to_string(h->ray_log2_units);
    return VOFOD_ERR_SIZE_MISMATCH;
  }
  if (hd.kind == VOFOD_SNAPSHOT_DELTA && (hd.base_gen == 0 || hd.base_gen != h->msync.applied_gen || static_cast<int>(hd.maps) != h->msync.applied_mask))
  {
    h->err = "map apply: the delta does not follow the snapshot this handle applied last";
    return VOFOD_ERR_DELTA_BASE;
  }
  return VOFOD_OK;
}

}  // namespace

extern "C" {

int vofod_map_export(vofod_handle* h, int32_t maps, int32_t kind, void* buf, size_t cap, int32_t memspace, size_t* n_bytes)
{
  if (!h || !n_bytes || maps <= 0 || (maps & ~MS_MAPS_ALL) || (kind != VOFOD_SNAPSHOT_DELTA && kind != VOFOD_SNAPSHOT_FULL) ||
      (memspace != VOFOD_MEM_HOST && memspace != VOFOD_MEM_DEVICE) || (!buf && cap))
    return VOFOD_ERR_INVALID_ARG;
  const bool size_only = !buf;
  if (memspace == VOFOD_MEM_DEVICE && (reinterpret_cast<uintptr_t>(buf) & 3))
    return VOFOD_ERR_INVALID_ARG;  // records are 32-bit words
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));  // (a pending exact raycast pass travels as its units: ms_export_locked marks the header)
  if (size_only || memspace == VOFOD_MEM_DEVICE)
    return ms_export_locked(h, maps, kind, static_cast<uint8_t*>(buf), cap, size_only, n_bytes);
  // host buffer: emitted into the staging buffer, then copied out
  VCHK(ms_export_locked(h, maps, kind, nullptr, cap, false, n_bytes));
  HIPCHK(hipMemcpy(buf, h->msync.d_wire, *n_bytes, hipMemcpyDeviceToHost));
  return VOFOD_OK;
}

int vofod_map_apply(vofod_handle* h, const void* buf, size_t n_bytes, int32_t memspace)
{
  if (!h || !buf || (memspace != VOFOD_MEM_HOST && memspace != VOFOD_MEM_DEVICE))
    return VOFOD_ERR_INVALID_ARG;
  if (n_bytes < sizeof(vms::WireHeader) || (memspace == VOFOD_MEM_DEVICE && (reinterpret_cast<uintptr_t>(buf) & 3)))
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, MAP_UNREAD));
  vms::WireHeader hd;
  if (memspace == VOFOD_MEM_HOST)
    std::memcpy(&hd, buf, sizeof(hd));
  else
  {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(&hd, buf, sizeof(hd), hipMemcpyDeviceToHost));
  }
  VCHK(ms_check_header(h, hd, n_bytes));
  const uint8_t* d_buf = static_cast<const uint8_t*>(buf);
  if (memspace == VOFOD_MEM_HOST)
  {
    VCHK(ms_ensure_wire(h, n_bytes));
    HIPCHK(hipMemcpyAsync(h->msync.d_wire, buf, n_bytes, hipMemcpyHostToDevice, h->stream));
    d_buf = h->msync.d_wire;
  }
  return ms_apply_locked(h, hd, d_buf, n_bytes);
}

// Collective over the communicator's ranks, device-resident.  Every rank makes the same four RCCL calls whatever happens on it,
// and every rank returns the same status:
//   1. ncclBroadcast of the control word (status, bytes): the root exports into the handle's staging buffer first; a failing
//      export ends the call on every rank with the root's status;
//   2. ncclAllReduce (max) of the receiving ranks' readiness: their small state, a staging buffer of `bytes`, no submitted
//      batch pending;
//   3. ncclBroadcast of the payload;
//   4. ncclAllReduce (max) of the apply statuses: a replica that cannot take the snapshot (VOFOD_ERR_DELTA_BASE after a missed
//      delta, a bad record) makes every rank return that status, so a caller's recovery (a full snapshot) runs on all ranks.
// Only a failing HIP runtime or RCCL call ends the call on one rank alone.
int vofod_broadcast_map(vofod_comm* c, vofod_handle* h, int32_t root, int32_t maps, int32_t kind, size_t* n_bytes)
{
  if (!c || !h || !n_bytes || root < 0 || root >= c->n_ranks || c->device != h->device)
    return VOFOD_ERR_INVALID_ARG;  // (the arguments agree on every rank: checked before any communication)
  std::scoped_lock lck(c->mtx, h->mtx);
  (void)hipSetDevice(h->device);
  *n_bytes = 0;
  const bool is_root = c->rank == root;
  auto rccl_error = [&](const char* what, int e) {
    c->err = std::string(what) + ": " + (vcoll::api().GetErrorString ? vcoll::api().GetErrorString(e) : "error");
    h->err = "broadcast_map: " + c->err;
    return VOFOD_ERR_DEVICE;
  };
  // the maximum of every rank's `local` status (0 = ok), returned on every rank
  auto agree = [&](int local, int* out) -> int {
    c->h_ctl[2] = static_cast<uint64_t>(static_cast<uint32_t>(local));
    HIPCHK(hipMemcpyAsync(c->d_ctl + 2, c->h_ctl + 2, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    if (const int e = vcoll::api().AllReduce(c->d_ctl + 2, c->d_ctl + 3, 1, 5 /* ncclUint64 */, 2 /* ncclMax */, c->comm, c->stream); e != 0)
      return rccl_error("ncclAllReduce", e);
    HIPCHK(hipMemcpyAsync(c->h_ctl + 3, c->d_ctl + 3, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = static_cast<int>(static_cast<uint32_t>(c->h_ctl[3]));
    if (*out != VOFOD_OK && local == VOFOD_OK)
      h->err = "broadcast_map: another rank failed with status " + std::to_string(*out);
    return VOFOD_OK;
  };
  int local = ms_ensure(h);  // (reported through the exchanges below, not by returning alone)
  MapSyncState& s = h->msync;
  // 1. the root's export and the control word
  if (is_root)
  {
    if (local == VOFOD_OK && (maps <= 0 || (maps & ~MS_MAPS_ALL) || (kind != VOFOD_SNAPSHOT_DELTA && kind != VOFOD_SNAPSHOT_FULL)))
    {
      h->err = "broadcast_map: bad maps mask or kind";
      local = VOFOD_ERR_INVALID_ARG;
    }
    size_t bytes = 0;
    if (local == VOFOD_OK)
      local = ms_export_locked(h, maps, kind, nullptr, SIZE_MAX, false, &bytes);
    c->h_ctl[0] = static_cast<uint64_t>(static_cast<uint32_t>(local));
    c->h_ctl[1] = local == VOFOD_OK ? bytes : 0;
    HIPCHK(hipMemcpyAsync(c->d_ctl, c->h_ctl, 2 * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  }
  if (const int e = vcoll::api().Broadcast(c->d_ctl, c->d_ctl, 2 * sizeof(uint64_t), 0 /* ncclChar */, root, c->comm, c->stream); e != 0)
    return rccl_error("ncclBroadcast", e);
  HIPCHK(hipMemcpyAsync(c->h_ctl, c->d_ctl, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int root_st = static_cast<int>(static_cast<uint32_t>(c->h_ctl[0]));
  const size_t bytes = static_cast<size_t>(c->h_ctl[1]);
  if (root_st != VOFOD_OK)
  {
    if (!is_root)
      h->err = "broadcast_map: the root's export failed with status " + std::to_string(root_st);
    return root_st;
  }
  *n_bytes = bytes;
  // 2. readiness of the receiving ranks
  if (!is_root && local == VOFOD_OK)
    local = ms_ensure_wire(h, bytes);
  if (!is_root && local == VOFOD_OK)
    local = admit(h, MAP_UNREAD);  // (a local refusal is every rank's: agreed on below)
  int st = VOFOD_OK;
  VCHK(agree(local, &st));
  if (st != VOFOD_OK)
    return st;
  // 3. the payload
  if (const int e = vcoll::api().Broadcast(s.d_wire, s.d_wire, bytes, 0 /* ncclChar */, root, c->comm, c->stream); e != 0)
    return rccl_error("ncclBroadcast", e);
  HIPCHK(hipStreamSynchronize(c->stream));
  // 4. apply on the receiving ranks; the outcome is every rank's
  if (!is_root)
  {
    vms::WireHeader hd;
    HIPCHK(hipMemcpy(&hd, s.d_wire, sizeof(hd), hipMemcpyDeviceToHost));
    local = ms_check_header(h, hd, bytes);
    if (local == VOFOD_OK)
      local = ms_apply_locked(h, hd, s.d_wire, bytes);
  }
  VCHK(agree(local, &st));
  return st;
}

}  // extern "C"
