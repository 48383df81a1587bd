// Host side of the world snapshots (kernels and wire header: world_sync.h; contract: include/vofod.h, WORLD SNAPSHOTS):
// vofod_world_export and vofod_world_apply.  Included by vofod_hip.hip after api_maps.h (world_view, world_clear,
// world_fetch_counters) and mapsync_host.h (ms_fresh_gen).
#pragma once

namespace
{

int wy_ensure(vofod_handle* h)
{
  vwy::State& s = h->wsync;
  if (s.h_small)  // (allocated last: it stands for all six)
    return VOFOD_OK;
  const uint32_t nc = static_cast<uint32_t>((h->world.n_dir + vwy::WY_CHUNK - 1) / vwy::WY_CHUNK);  // (n_dir <= 2^31)
  s.n_chunks = nc;
  HIPCHK(s.d_sel.alloc(nc));
  HIPCHK(s.d_cnt.alloc(nc));
  HIPCHK(s.d_prefix.alloc(static_cast<size_t>(nc) + 1));
  HIPCHK(s.d_bsum.alloc(nc / vr::GS_EPB + 2));
  HIPCHK(s.d_small.alloc(4));
  HIPCHK(s.h_small.alloc(4));
  return VOFOD_OK;
}

int wy_ensure_wire(vofod_handle* h, size_t bytes)
{
  vwy::State& s = h->wsync;
  if (bytes > s.d_wire.n && s.d_wire.alloc(std::max(bytes + bytes / 4 + 4096, 2 * s.d_wire.n)) != hipSuccess)  // (geometric, as the map snapshots' staging)
  {
    (void)hipGetLastError();  // (the allocation's error is answered here: it must not show up at the next launch)
    h->err = "world snapshot: the staging buffer of " + std::to_string(bytes) + " bytes could not be allocated";
    return VOFOD_ERR_DEVICE;
  }
  return VOFOD_OK;
}

dim3 wy_grid(uint64_t waves) { return dim3(static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>((waves + vwy::WY_WAVES - 1) / vwy::WY_WAVES, 1), vwy::WY_GRID))); }

// select + scan, and - unless size_only - index list, tiles and header written to the device buffer d_dst (cap bytes; nullptr: the
// handle's staging buffer, grown to fit).  *n_bytes = the snapshot's size in every case.  Nothing but the selection scratch is
// touched before the capacity check: a refused export leaves generation and shadow as they were.
int wy_export_locked(vofod_handle* h, int kind, uint8_t* d_dst, size_t cap, bool size_only, size_t* n_bytes)
{
  vwy::State& s = h->wsync;
  const vws::Store& w = h->world;
  const bool full = kind == VOFOD_SNAPSHOT_FULL;
  if (!full && s.chain_gen == 0)
  {
    h->err = "world export: no full world snapshot was exported before (a delta needs a chain; reset, disable and apply end it)";
    return VOFOD_ERR_DELTA_BASE;
  }
  VCHK(wy_ensure(h));
  const uint32_t nc = s.n_chunks, n_dir = static_cast<uint32_t>(w.n_dir);
  const dim3 grid = wy_grid(nc), block(vwy::WY_THREADS);
  if (full)
    KLAUNCH_AS(h, "k_world_select", vwy::k_world_select<true>, grid, block, static_cast<const uint32_t*>(w.d_dir.p), n_dir, nc, static_cast<const uint32_t*>(w.d_pool.p), static_cast<const uint32_t*>(nullptr), 0u,
               w.cap, s.d_sel.p, s.d_cnt.p);
  else
    KLAUNCH_AS(h, "k_world_select", vwy::k_world_select<false>, grid, block, static_cast<const uint32_t*>(w.d_dir.p), n_dir, nc, static_cast<const uint32_t*>(w.d_pool.p),
               static_cast<const uint32_t*>(s.d_shadow.p), static_cast<uint32_t>(s.known_used), w.cap, s.d_sel.p, s.d_cnt.p);
  HIPCHK(hipGetLastError());
  VCHK(gscan(h, s.d_cnt, nc, s.d_prefix, s.d_bsum, s.d_small));
  HIPCHK(hipMemcpyAsync(s.h_small, s.d_small, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const uint32_t n = s.h_small[0];
  const size_t bytes = vwy::wire_bytes(n);
  *n_bytes = bytes;
  if (size_only)
    return VOFOD_OK;
  if (cap < bytes)
  {
    h->err = "world export: buffer too small (n_bytes holds the size)";
    return VOFOD_ERR_CAPACITY;
  }
  if (!d_dst)
  {
    VCHK(wy_ensure_wire(h, bytes));
    d_dst = s.d_wire;
  }
  if (!s.d_shadow && s.d_shadow.alloc(w.cap * vws::WS_TILE_WORDS) != hipSuccess)  // (a full export: a delta has a chain, and a chain has a shadow)
  {
    (void)hipGetLastError();  // (as vofod_world_enable: the allocation's error is answered here)
    h->err = "world export: the shadow pool (" + std::to_string(w.cap * vws::WS_TILE_WORDS * sizeof(uint32_t)) + " bytes, as large as the pool) could not be allocated; nothing changed";
    return VOFOD_ERR_DEVICE;
  }
  vwy::WireHeader hd{};
  hd.magic = vwy::WY_MAGIC;
  hd.version = vwy::WY_VERSION;
  hd.kind = static_cast<uint32_t>(kind);
  hd.tile_edge = vws::WS_EDGE;
  hd.map_size[0] = h->mg.sx;
  hd.map_size[1] = h->mg.sy;
  hd.map_size[2] = h->mg.sz;
  for (int a = 0; a < 3; a++)
    hd.map_offset[a] = h->mg.off[a], hd.K[a] = w.K[a], hd.box_lo[a] = w.lo[a], hd.box_hi[a] = w.hi[a];
  hd.voxel_size = h->sp.voxel_size;
  hd.score_init = h->sp.score_init;
  hd.base_gen = full ? 0 : s.chain_gen;
  hd.new_gen = ms_fresh_gen();
  hd.n_tiles = n;
  hd.shifts_short_of_tiles = w.h_ctr[vws::WC_SHORT];
  hd.voxels_forgotten = w.h_ctr[vws::WC_FORGOTTEN];
  uint32_t* idx = reinterpret_cast<uint32_t*>(d_dst + sizeof(vwy::WireHeader));
  const uint64_t n4 = vwy::pad4(n);
  if (n)
  {
    HIPCHK(hipMemsetAsync(idx, 0xFF, 4 * n4, h->stream));  // (the padding entries; k_world_emit writes the other n)
    KLAUNCH_AS(h, "k_world_emit", vwy::k_world_emit, grid, block, static_cast<const uint32_t*>(w.d_dir.p), n_dir, nc, static_cast<const uint32_t*>(w.d_pool.p), s.d_shadow.p, w.cap,
               static_cast<const unsigned long long*>(s.d_sel.p), static_cast<const uint32_t*>(s.d_prefix.p), n, idx, idx + n4);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(d_dst, &hd, sizeof(hd), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // (hd is on this frame)
  s.chain_gen = hd.new_gen;
  s.known_used = w.h_ctr[vws::WC_USED];
  return VOFOD_OK;
}

// format checks of vofod_world_apply that need the header alone
int wy_check_format(vofod_handle* h, const vwy::WireHeader& hd, size_t n_bytes)
{
  if (hd.magic != vwy::WY_MAGIC || hd.version != vwy::WY_VERSION || hd.kind > 1 || hd.tile_edge != static_cast<uint32_t>(vws::WS_EDGE) || hd.zero != 0)
  {
    h->err = "world apply: not a world snapshot (magic, version, kind, tile edge or the reserved word)";
    return VOFOD_ERR_INVALID_ARG;
  }
  if (hd.n_tiles > vws::WS_MAX_TILES || n_bytes != vwy::wire_bytes(hd.n_tiles))
  {
    h->err = "world apply: length does not match the header's tile count";
    return VOFOD_ERR_INVALID_ARG;
  }
  return VOFOD_OK;
}

// geometry checks; K1 = the origin this handle holds after the apply
int wy_check_geometry(vofod_handle* h, const vwy::WireHeader& hd, int32_t K1[3])
{
  const vws::Store& w = h->world;
  bool same = hd.map_size[0] == h->mg.sx && hd.map_size[1] == h->mg.sy && hd.map_size[2] == h->mg.sz;
  same &= std::memcmp(&hd.voxel_size, &h->sp.voxel_size, 4) == 0 && std::memcmp(&hd.score_init, &h->sp.score_init, 4) == 0;
  for (int a = 0; a < 3; a++)
    same &= hd.box_lo[a] == w.lo[a] && hd.box_hi[a] == w.hi[a];
  if (!same)
  {
    h->err = "world apply: map size, voxel size, score_init or the world box differ from this handle's";
    return VOFOD_ERR_SIZE_MISMATCH;
  }
  const double vs = static_cast<double>(h->sp.voxel_size);
  for (int a = 0; a < 3; a++)
  {
    // the window need not sit where the owner's sat: a whole number of voxels apart (vofod_map_shift's rule)
    const double gap = static_cast<double>(h->mg.off[a]) - static_cast<double>(hd.map_offset[a]);
    const double d = std::nearbyint(gap / vs);
    const double k1 = static_cast<double>(hd.K[a]) + d;
    if (!(std::fabs(gap - d * vs) < vs / 4.0) || !(std::fabs(k1) <= static_cast<double>(vws::WS_K_LIMIT)))
    {
      h->err = "world apply: this handle's map offset is not a whole number of voxels from the snapshot's, or the origin would leave +-2^30, on axis " + std::to_string(a);
      return VOFOD_ERR_SIZE_MISMATCH;
    }
    K1[a] = static_cast<int32_t>(k1);
    if (hd.kind == VOFOD_SNAPSHOT_DELTA && K1[a] != w.K[a])
    {
      h->err = "world apply: the delta's origin is not this handle's on axis " + std::to_string(a);
      return VOFOD_ERR_SIZE_MISMATCH;
    }
  }
  return VOFOD_OK;
}

// hd = the header (host copy, format checked), d_buf = the whole snapshot on the device
int wy_apply_locked(vofod_handle* h, const vwy::WireHeader& hd, const uint8_t* d_buf)
{
  vwy::State& s = h->wsync;
  vws::Store& w = h->world;
  const bool full = hd.kind == VOFOD_SNAPSHOT_FULL;
  const uint32_t n = static_cast<uint32_t>(hd.n_tiles), n4 = static_cast<uint32_t>(vwy::pad4(n)), n_dir = static_cast<uint32_t>(w.n_dir);
  const uint32_t* idx = reinterpret_cast<const uint32_t*>(d_buf + sizeof(vwy::WireHeader));
  const uint32_t* tiles = idx + n4;
  VCHK(wy_ensure(h));
  // 1. format, the part on the device: the index list - and, in the same pass, the tiles this directory does not hold
  s.h_small[1] = s.h_small[2] = 0;
  if (n4)
  {
    HIPCHK(hipMemsetAsync(s.d_small + 1, 0, 2 * sizeof(uint32_t), h->stream));
    KLAUNCH_AS(h, "k_world_check", vwy::k_world_check, dim3(std::min<uint32_t>((n4 + vwy::WY_THREADS - 1) / vwy::WY_THREADS, vwy::WY_GRID)), dim3(vwy::WY_THREADS), idx, n, n4,
               static_cast<const uint32_t*>(w.d_dir.p), n_dir, s.d_small + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.h_small + 1, s.d_small + 1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  if (s.h_small[1])
  {
    h->err = "world apply: tile indices not strictly ascending, beyond the directory, or the list's padding is not 0xFFFFFFFF";
    return VOFOD_ERR_INVALID_ARG;
  }
  // 2. geometry, 3. chain
  int32_t K1[3];
  VCHK(wy_check_geometry(h, hd, K1));
  if (!full && (hd.base_gen == 0 || hd.base_gen != s.applied_gen))
  {
    h->err = "world apply: the delta does not follow the world snapshot this handle applied last (or the store was written since)";
    return VOFOD_ERR_DELTA_BASE;
  }
  // 4. capacity, all or nothing (a full snapshot empties the store first: every carried tile is new)
  const uint64_t used = full ? 0 : w.h_ctr[vws::WC_USED], fresh = full ? n : s.h_small[2];
  if (used + fresh > w.cap)
  {
    h->err = "world apply: the snapshot needs " + std::to_string(fresh) + " new tiles, " + std::to_string(w.cap - used) + " are free";
    return VOFOD_ERR_CAPACITY;
  }
  if (full)
    VCHK(world_clear(h));
  KLAUNCH_AS(h, "k_world_scatter", vwy::k_world_scatter, wy_grid(n), dim3(vwy::WY_THREADS), idx, tiles, n, w.d_dir.p, n_dir, w.d_pool.p, w.cap, w.d_ctr.p,
             static_cast<unsigned long long>(hd.shifts_short_of_tiles), static_cast<unsigned long long>(hd.voxels_forgotten));
  HIPCHK(hipGetLastError());
  VCHK(world_fetch_counters(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int a = 0; a < 3; a++)
    w.K[a] = K1[a];
  s.applied_gen = hd.new_gen;
  s.chain_gen = 0;  // this handle's own exports described a store that is gone
  return VOFOD_OK;
}

}  // namespace

extern "C" {

int vofod_world_export(vofod_handle* h, int32_t kind, void* buf, size_t cap, int32_t memspace, size_t* n_bytes)
{
  if (!h || !n_bytes || (kind != VOFOD_SNAPSHOT_DELTA && kind != VOFOD_SNAPSHOT_FULL) || (memspace != VOFOD_MEM_HOST && memspace != VOFOD_MEM_DEVICE) || (!buf && cap))
    return VOFOD_ERR_INVALID_ARG;
  const bool size_only = !buf;
  if (memspace == VOFOD_MEM_DEVICE && (reinterpret_cast<uintptr_t>(buf) & 15))
    return VOFOD_ERR_INVALID_ARG;  // tiles travel as 16-byte words
  ApiLock lock(h);
  if (!h->world.enabled)
    return VOFOD_ERR_NOT_PENDING;
  VCHK(admit(h, NEEDS_NOTHING));  // (no frame kernel touches the store: export may run beside batches in flight)
  if (size_only || memspace == VOFOD_MEM_DEVICE)
    return wy_export_locked(h, kind, static_cast<uint8_t*>(buf), cap, size_only, n_bytes);
  VCHK(wy_export_locked(h, kind, nullptr, cap, false, n_bytes));
  HIPCHK(hipMemcpy(buf, h->wsync.d_wire, *n_bytes, hipMemcpyDeviceToHost));
  return VOFOD_OK;
}

int vofod_world_apply(vofod_handle* h, const void* buf, size_t n_bytes, int32_t memspace)
{
  if (!h || !buf || (memspace != VOFOD_MEM_HOST && memspace != VOFOD_MEM_DEVICE))
    return VOFOD_ERR_INVALID_ARG;
  if (n_bytes < sizeof(vwy::WireHeader) || (memspace == VOFOD_MEM_DEVICE && (reinterpret_cast<uintptr_t>(buf) & 15)))
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  if (!h->world.enabled)
    return VOFOD_ERR_NOT_PENDING;
  VCHK(admit(h, MAP_UNREAD));
  vwy::WireHeader hd;
  if (memspace == VOFOD_MEM_HOST)
    std::memcpy(&hd, buf, sizeof(hd));
  else
  {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(&hd, buf, sizeof(hd), hipMemcpyDeviceToHost));
  }
  VCHK(wy_check_format(h, hd, n_bytes));
  const uint8_t* d_buf = static_cast<const uint8_t*>(buf);
  if (memspace == VOFOD_MEM_HOST)
  {
    VCHK(wy_ensure_wire(h, n_bytes));
    HIPCHK(hipMemcpyAsync(h->wsync.d_wire, buf, n_bytes, hipMemcpyHostToDevice, h->stream));
    d_buf = h->wsync.d_wire;
  }
  return wy_apply_locked(h, hd, d_buf);
}

}  // extern "C"
