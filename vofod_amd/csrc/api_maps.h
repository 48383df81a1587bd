// The map entry points of include/vofod.h (included by vofod_hip.hip after driver_aux.h): reading and writing the three maps, the
// a-priori cloud, the rolling operation area (vofod_map_shift) and the world store (vofod_world_*) with its host helpers.
#pragma once

extern "C" {

// ---- world store (contract: include/vofod.h, WORLD STORE; kernels and the order between them: world_store.h)
static vws::View world_view(vofod_handle* h)
{
  const vws::Store& w = h->world;
  vws::View v{};
  v.dir = w.d_dir;
  v.pool = w.d_pool;
  v.ctr = w.d_ctr;
  for (int a = 0; a < 3; a++)
    v.lo[a] = w.lo[a], v.hi[a] = w.hi[a], v.T[a] = w.T[a];
  std::memcpy(&v.init, &h->sp.score_init, 4);
  v.cap = w.cap;
  return v;
}

// n items, `per_lane` of them per lane and step of the grid-stride loop
static dim3 world_grid(uint64_t n, uint64_t per_lane = 1)
{
  const uint64_t per_block = vws::WS_THREADS * per_lane;
  return dim3(static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>((n + per_block - 1) / per_block, 1), vws::WS_GRID)));
}

// the counters travel to the host behind the kernels queued so far; they are valid after the caller's hipStreamSynchronize
static int world_fetch_counters(vofod_handle* h)
{
  HIPCHK(hipMemcpyAsync(h->world.h_ctr, h->world.d_ctr, sizeof(unsigned long long) * vws::WC_N, hipMemcpyDeviceToHost, h->stream));
  return VOFOD_OK;
}

// slabs of the window that the shift s pushes out (leaving) or, with -s, that the new window gains
static vws::Rim world_rim(vofod_handle* h, const int32_t s[3], int sign)
{
  const int32_t S[3] = {h->mg.sx, h->mg.sy, h->mg.sz};
  int32_t a0[3], a1[3];
  for (int a = 0; a < 3; a++)
    vws::rim_interval(static_cast<int64_t>(sign) * s[a], S[a], a0[a], a1[a]);
  return vws::make_rim(S, a0, a1);
}

// step 1 of a shift with the store: mark, claim, put - on the voxel map as it stands, in front of the k_map_shift passes
static int world_write_back(vofod_handle* h, const int32_t s[3])
{
  vws::Store& w = h->world;
  const vws::View v = world_view(h);
  const vws::Rim rim = world_rim(h, s, +1);
  const uint32_t* map = reinterpret_cast<const uint32_t*>(h->d_map.p);
  const dim3 grid = world_grid(rim.first[3], vws::WS_UNROLL), block(vws::WS_THREADS);
  KLAUNCH_AS(h, "k_world_mark", vws::k_world_mark, grid, block, v, rim, map, h->mg.sx, h->mg.sy, static_cast<int64_t>(w.K[0]), static_cast<int64_t>(w.K[1]), static_cast<int64_t>(w.K[2]), w.d_list.p, w.list_cap);
  KLAUNCH_AS(h, "k_world_claim", vws::k_world_claim, dim3(std::min<uint32_t>((w.list_cap + 1) / 2, 2048u)), block, v, static_cast<const uint32_t*>(w.d_list.p), w.list_cap);
  KLAUNCH_AS(h, "k_world_put", vws::k_world_put, grid, block, v, rim, map, h->mg.sx, h->mg.sy, static_cast<int64_t>(w.K[0]), static_cast<int64_t>(w.K[1]), static_cast<int64_t>(w.K[2]));
  HIPCHK(hipGetLastError());
  return VOFOD_OK;
}

// step 3: behind the k_map_shift of the voxel map (h->d_map is the shifted map), K1 = K + s
static int world_read_in(vofod_handle* h, const int32_t s[3], const int64_t K1[3])
{
  const vws::Rim rim = world_rim(h, s, -1);
  KLAUNCH_AS(h, "k_world_get", vws::k_world_get, world_grid(rim.first[3], vws::WS_UNROLL), dim3(vws::WS_THREADS), world_view(h), rim, reinterpret_cast<uint32_t*>(h->d_map.p), h->mg.sx, h->mg.sy, K1[0], K1[1], K1[2]);
  HIPCHK(hipGetLastError());
  return world_fetch_counters(h);
}

// the world store as vofod_world_enable leaves it: an empty directory (every byte of WS_EMPTY is 0xFF), a free pool, zero counters.
// The pool keeps its bytes: k_world_claim fills a tile when it hands it out.  Queued on the stream; the caller synchronises.
static int world_clear(vofod_handle* h)
{
  vws::Store& w = h->world;
  HIPCHK(hipMemsetAsync(w.d_dir, 0xFF, w.n_dir * sizeof(uint32_t), h->stream));
  HIPCHK(hipMemsetAsync(w.d_ctr, 0, sizeof(unsigned long long) * vws::WC_N, h->stream));
  std::memset(w.h_ctr, 0, sizeof(unsigned long long) * vws::WC_N);
  return VOFOD_OK;
}

int vofod_load_apriori(vofod_handle* h, const float* xyz, size_t n)
{
  if (!h || (!xyz && n))
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, WS0_FREE | MAP_UNREAD));
  if (n)
  {
    DevBuf<float> d;
    HIPCHK(d.alloc(n * 3));
    HIPCHK(hipMemcpy(d, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    // World store: the points beyond the window.  Their tiles are counted first (mark, claim), and the host looks at the sum before
    // anything else changes - init-time work, so this one call pays a round trip that a shift does not.
    vws::Store& w = h->world;
    const int64_t K[3] = {w.K[0], w.K[1], w.K[2]};
    const dim3 pgrid(static_cast<uint32_t>((n + vws::WS_THREADS - 1) / vws::WS_THREADS)), pblock(vws::WS_THREADS);
    if (w.enabled)
    {
      DevBuf<uint32_t> list;  // the wanted tiles of this cloud: at most one per point, at most the directory
      const uint32_t list_cap = static_cast<uint32_t>(std::min<uint64_t>(n, w.n_dir));
      HIPCHK(list.alloc(list_cap));
      const vws::View v = world_view(h);
      KLAUNCH_AS(h, "k_world_mark_points", vws::k_world_mark_points, pgrid, pblock, v, h->mg, static_cast<const float*>(d.p), static_cast<uint32_t>(n), K[0], K[1], K[2], list.p, list_cap);
      KLAUNCH_AS(h, "k_world_claim", vws::k_world_claim, dim3(std::min<uint32_t>((list_cap + 1) / 2, 2048u)), pblock, v, static_cast<const uint32_t*>(list.p), list_cap);
      HIPCHK(hipGetLastError());
      VCHK(world_fetch_counters(h));
      HIPCHK(hipStreamSynchronize(h->stream));
      if (w.h_ctr[vws::WC_USED] + w.h_ctr[vws::WC_WANTED] > w.cap)
      {
        // (k_world_claim has put the directory words back: only the list's length is left to clear)
        h->err = "load apriori: the cloud needs " + std::to_string(w.h_ctr[vws::WC_WANTED]) + " new tiles of the world store, " + std::to_string(w.cap - w.h_ctr[vws::WC_USED]) + " are free";
        HIPCHK(hipMemsetAsync(w.d_ctr + vws::WC_WANTED, 0, sizeof(unsigned long long), h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        w.h_ctr[vws::WC_WANTED] = 0;
        return VOFOD_ERR_CAPACITY;
      }
    }
    KLAUNCH(h, k_apriori, dim3((n + 255) / 256), dim3(256), h->d_map, h->mg, d, static_cast<uint32_t>(n));
    if (w.enabled)
    {
      KLAUNCH_AS(h, "k_world_put_points", vws::k_world_put_points, pgrid, pblock, world_view(h), h->mg, static_cast<const float*>(d.p), static_cast<uint32_t>(n), K[0], K[1], K[2]);
      HIPCHK(hipGetLastError());
      VCHK(world_fetch_counters(h));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  h->wsync.applied_gen = 0;  // (world snapshots: a call other than vofod_world_apply that may write the store ends the applied chain - a cloud of zero points too, so that the rule has no exception; the owner's chain records it)
  h->sure_background_sufficient = true;  // vofod_nodelet.cpp:343-344
  h->background_pts_sufficient = true;
  h->mapbits_valid = false;
  return VOFOD_OK;
}

static float* pick_map(vofod_handle* h, int which)
{
  switch (which)
  {
    case VOFOD_MAP_VOXELS: return h->d_map;
    case VOFOD_MAP_FLAGS: return h->d_flags;
    case VOFOD_MAP_RAYCAST: return h->d_ray;
  }
  return nullptr;
}

int vofod_read_map(vofod_handle* h, int which, float* dst, size_t n)
{
  if (!h || !dst)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));  // (the raycast map of a pending exact pass is read as its float view, below)
  float* m = pick_map(h, which);
  if (!m || n != h->mg.n)
    return VOFOD_ERR_SIZE_MISMATCH;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(dst, m, n * sizeof(float), hipMemcpyDeviceToHost));
  if (which == VOFOD_MAP_RAYCAST && h->raycast_pending && h->ray_pass_exact)
  {
    // the float view of a pending exact pass, formed in the caller's copy (the device keeps the units)
    const float inv = std::ldexp(1.0f, -h->ray_log2_units);
    for (size_t i = 0; i < n; i++)
    {
      uint32_t u;
      std::memcpy(&u, &dst[i], 4);
      dst[i] = static_cast<float>(u) * inv;
    }
  }
  return VOFOD_OK;
}

int vofod_voxels_as_pc(vofod_handle* h, int which, float threshold, int greater_than, vofod_point_xyzi* out, size_t cap, size_t* n_out)
{
  if (!h || !n_out || (cap && !out))
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  const float* m = pick_map(h, which);
  if (!m)
    return VOFOD_ERR_INVALID_ARG;
  VCHK(admit(h, floats_in(which), nullptr, " (vofod_read_map returns its float view)"));
  *n_out = 0;
  vr::SepState& s = h->sep;
  const uint32_t ncol = static_cast<uint32_t>(h->mg.sx) * h->mg.sy;
  VCHK(sep_ensure_words(h, ncol + 2));
  VCHK(sep_ensure_pts(h, std::max<size_t>(1 << 16, ncol)));
  KLAUNCH(h, vr::k_col_count_thr, dim3((ncol + 255) / 256), dim3(256), h->mg, m, threshold, greater_than, s.d_tpop);
  VCHK(gscan(h, s.d_tpop, ncol, s.d_tprefix, s.d_bsum, s.d_small));
  HIPCHK(hipMemcpyAsync(s.h_small, s.d_small, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const uint32_t P = s.h_small[0];
  *n_out = P;
  if (P > cap)
    return VOFOD_ERR_CAPACITY;  // n_out holds the required size
  if (P == 0)
    return VOFOD_OK;
  VCHK(ensure_boxstage(h, static_cast<size_t>(P) * 4));
  KLAUNCH(h, vr::k_col_emit_xyzi, dim3((ncol + 255) / 256), dim3(256), h->mg, m, threshold, greater_than, s.d_tprefix, P, reinterpret_cast<float4*>(h->d_boxstage.p));
  HIPCHK(hipMemcpyAsync(out, h->d_boxstage, sizeof(vofod_point_xyzi) * P, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VOFOD_OK;
}

int vofod_update_ground(vofod_handle* h, float range, float min_range, float max_range, const float tf[12])
{
  if (!h || !tf)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, MAP_UNREAD));
  if (range <= min_range && range >= max_range)  // vofod_nodelet.cpp:585, as written
    return VOFOD_OK;
  // one voxel at the range-finder's rate: read, blend on the host in the reference's double expression, write back
  const float p[3] = {tf[0] * range + tf[3], tf[4] * range + tf[7], tf[8] * range + tf[11]};  // :597
  int idx[3];
  h->hg.coordToIdx(p, idx);
  if (!h->hg.inLimits(idx))  // :601-605
    return VOFOD_ERR_MAP_RANGE;
  float* cell = h->d_map + h->hg.lin(idx);
  float m = 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(&m, cell, sizeof(float), hipMemcpyDeviceToHost));
  m = static_cast<float>((static_cast<double>(m) + h->dp.voxel_map__scores__point) / 2.0);  // :609
  HIPCHK(hipMemcpy(cell, &m, sizeof(float), hipMemcpyHostToDevice));
  h->mapbits_valid = false;
  return VOFOD_OK;
}

int vofod_write_map(vofod_handle* h, int which, const float* src, size_t n)
{
  if (!h || !src)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, MAP_UNREAD));
  float* m = pick_map(h, which);
  if (!m || n != h->mg.n)
    return VOFOD_ERR_SIZE_MISMATCH;
  VCHK(admit(h, floats_in(which)));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(m, src, n * sizeof(float), hipMemcpyHostToDevice));
  h->mapbits_valid = false;
  return VOFOD_OK;
}

// Rolling operation area (contract: include/vofod.h; kernel, geometry function and the account of the scratch buffers: map_shift.h).
// Everything is checked before anything changes; the maps move out of place into the spare buffer, whose owner is then swapped with
// the map's - nothing holds a map pointer between calls (map_shift.h), so there is nothing to refresh behind the swap.
int vofod_map_shift(vofod_handle* h, const int32_t shift_voxels[3], const float new_oparea_offset[3])
{
  if (!h || !shift_voxels || !new_oparea_offset)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, MAP_UNREAD | NO_RAYCAST_PASS | NO_SEP_PASS, "map shift"));
  vws::Store& w = h->world;
  if (w.enabled)
    for (int a = 0; a < 3; a++)
      if (std::llabs(static_cast<long long>(w.K[a]) + shift_voxels[a]) > vws::WS_K_LIMIT)
      {
        h->err = "map shift: the world store's origin would leave +-2^30 on axis " + std::to_string(a);
        return VOFOD_ERR_INVALID_ARG;
      }
  // the geometry a handle created at the new offset would hold
  vofod_static_params nsp = h->sp;
  vsh::AreaGeometry ng;
  bool same_offset = true;
  for (int a = 0; a < 3; a++)
  {
    if (!std::isfinite(new_oparea_offset[a]))
      return VOFOD_ERR_INVALID_ARG;
    nsp.oparea_offset[a] = new_oparea_offset[a];
    same_offset &= std::memcmp(&nsp.oparea_offset[a], &h->sp.oparea_offset[a], 4) == 0;
  }
  vsh::area_geometry(nsp, ng);
  const int S[3] = {h->mg.sx, h->mg.sy, h->mg.sz};
  for (int a = 0; a < 3; a++)
  {
    const double want = static_cast<double>(h->mg.off[a]) + static_cast<double>(shift_voxels[a]) * static_cast<double>(h->mg.vs);
    if (!(std::fabs(static_cast<double>(ng.map_off[a]) - want) < static_cast<double>(h->mg.vs) / 4.0))
    {
      h->err = "map shift: new_oparea_offset does not move the map origin by shift_voxels * voxel_size on axis " + std::to_string(a);
      return VOFOD_ERR_INVALID_ARG;
    }
  }
  if (same_offset && shift_voxels[0] == 0 && shift_voxels[1] == 0 && shift_voxels[2] == 0)
  {
    h->wsync.applied_gen = 0;  // (world snapshots: every successful shift ends the applied chain, the one that moves nothing too - the rule has no exception)
    return VOFOD_OK;
  }
  const size_t M = h->mg.n;
  HIPCHK(h->d_shift_spare.reserve(std::max<size_t>(M, 4)));  // (it becomes a map: sized as vofod_create sizes them)
  vsh::ShiftParams p{};
  p.n = M;
  p.sx = S[0];
  p.sy = S[1];
  p.sz = S[2];
  int32_t s[3];
  for (int a = 0; a < 3; a++)
    s[a] = std::min(std::max(shift_voxels[a], -S[a]), S[a]);  // (a shift of a whole map size or more: nothing is valid either way)
  p.s0 = s[0];
  p.s1 = s[1];
  p.s2 = s[2];
  p.delta = static_cast<int64_t>(s[0]) + static_cast<int64_t>(s[1]) * S[0] + static_cast<int64_t>(s[2]) * S[0] * S[1];
  p.ntiles = static_cast<uint32_t>((M + vsh::SH_TILE - 1) / vsh::SH_TILE);
  const dim3 grid(std::min<uint32_t>(p.ntiles, vsh::SH_GRID));
  DevBuf<float>* maps[3] = {&h->d_map, &h->d_flags, &h->d_ray};
  if (w.enabled)
    VCHK(world_write_back(h, shift_voxels));  // (the shift as given, not the one clamped for k_map_shift: K moves by it)
  for (int m = 0; m < 3; m++)
  {
    const float init = m == VOFOD_MAP_VOXELS ? h->sp.score_init : 0.0f;
    std::memcpy(&p.init, &init, 4);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(maps[m]->p);
    uint32_t* dst = reinterpret_cast<uint32_t*>(h->d_shift_spare.p);
    KLAUNCH_AS(h, "k_map_shift", vsh::k_map_shift, grid, dim3(vsh::SH_THREADS), src, dst, p);
    HIPCHK(hipGetLastError());
    std::swap(*maps[m], h->d_shift_spare);  // (stream order: the next launch writes the buffer this one has read)
  }
  int64_t K1[3] = {0, 0, 0};
  if (w.enabled)
  {
    for (int a = 0; a < 3; a++)
      K1[a] = static_cast<int64_t>(w.K[a]) + shift_voxels[a];
    VCHK(world_read_in(h, shift_voxels, K1));
  }
  HIPCHK(hipStreamSynchronize(h->stream));  // (the call's only one: the store's counters arrive with it)
  if (w.enabled)
  {
    for (int a = 0; a < 3; a++)
      w.K[a] = static_cast<int32_t>(K1[a]);
    h->wsync.applied_gen = 0;  // (world snapshots: this handle's own write-back ends the applied chain; the owner's chain records it)
  }
  h->sp = nsp;
  set_area_geometry(h);
  h->mapbits_valid = false;  // occupancy image, dilated image and nVoxelsOver are rebuilt on next use (as after write_map)
  forget_detections(h);  // (they belong to the old area)
  // the snapshot chain ends on both sides (the shadows hold the unshifted maps; a full export rewrites them)
  h->msync.chain_gen = 0;
  h->msync.chain_mask = 0;
  h->msync.applied_gen = 0;
  h->msync.applied_mask = 0;
  return VOFOD_OK;
}

int vofod_world_enable(vofod_handle* h, const int32_t margin_lo[3], const int32_t margin_hi[3], uint64_t max_tiles)
{
  if (!h || !margin_lo || !margin_hi)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, MAP_UNREAD | NO_RAYCAST_PASS | NO_SEP_PASS, "world enable"));
  vws::Store& w = h->world;
  if (w.enabled || max_tiles == 0 || max_tiles > vws::WS_MAX_TILES)
  {
    h->err = w.enabled ? "world enable: the store is enabled already" : "world enable: max_tiles outside 1 .. 2^32 - 16";
    return VOFOD_ERR_INVALID_ARG;
  }
  const int32_t S[3] = {h->mg.sx, h->mg.sy, h->mg.sz};
  int32_t lo[3], hi[3], T[3];
  uint64_t n_dir = 1, window_tiles = 1;
  for (int a = 0; a < 3; a++)
  {
    const int64_t hi64 = static_cast<int64_t>(S[a]) + margin_hi[a];
    if (margin_lo[a] < 0 || margin_hi[a] < 0 || hi64 > INT32_MAX)
    {
      h->err = "world enable: a negative margin, or a box beyond 2^31 on axis " + std::to_string(a);
      return VOFOD_ERR_INVALID_ARG;
    }
    lo[a] = -margin_lo[a];
    hi[a] = static_cast<int32_t>(hi64);
    const int64_t tiles = (hi64 - lo[a] + vws::WS_EDGE - 1) / vws::WS_EDGE;  // (< 2^29)
    T[a] = static_cast<int32_t>(tiles);
    n_dir *= static_cast<uint64_t>(tiles);  // (at most 2^31 * 2^29: tested after every axis)
    if (n_dir > (1ull << 31))
    {
      h->err = "world enable: the directory would hold more than 2^31 words";
      return VOFOD_ERR_INVALID_ARG;
    }
    window_tiles *= static_cast<uint64_t>((S[a] + vws::WS_EDGE - 1) / vws::WS_EDGE + 1);  // (the grid is anchored at lo, not at the window)
  }
  w.cap = std::min<uint64_t>(max_tiles, n_dir);
  w.n_dir = n_dir;
  w.list_cap = static_cast<uint32_t>(std::min<uint64_t>(window_tiles, n_dir));
  const bool ok = w.d_dir.alloc(n_dir) == hipSuccess && w.d_pool.alloc(w.cap * vws::WS_TILE_WORDS) == hipSuccess && w.d_list.alloc(w.list_cap) == hipSuccess &&
                  w.d_ctr.alloc(vws::WC_N) == hipSuccess && w.h_ctr.alloc(vws::WC_N) == hipSuccess;
  if (!ok)
  {
    (void)hipGetLastError();  // (the allocation's error is answered here: it must not show up at the next launch)
    w.drop();
    h->err = "world enable: directory or pool could not be allocated";
    return VOFOD_ERR_DEVICE;
  }
  for (int a = 0; a < 3; a++)
    w.K[a] = 0, w.lo[a] = lo[a], w.hi[a] = hi[a], w.T[a] = T[a];
  if (const int r = world_clear(h); r != VOFOD_OK || hipStreamSynchronize(h->stream) != hipSuccess)
  {
    w.drop();
    return VOFOD_ERR_DEVICE;
  }
  w.enabled = true;
  return VOFOD_OK;
}

int vofod_world_disable(vofod_handle* h)
{
  if (!h)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  if (!h->world.enabled)
    return VOFOD_ERR_NOT_PENDING;  // (a disabled store answers so even while a batch is in flight)
  VCHK(admit(h, MAP_UNREAD));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->world.drop();
  h->wsync.drop();  // (the shadow pool, the scratch and both chains of the world snapshots)
  return VOFOD_OK;
}

int vofod_world_status(vofod_handle* h, vofod_world_info* out)
{
  if (!h || !out)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h, ApiLock::LOCK_ONLY);
  VCHK(admit(h, NEEDS_NOTHING));
  *out = vofod_world_info{};
  const vws::Store& w = h->world;
  if (!w.enabled)
    return VOFOD_OK;
  out->enabled = 1;
  out->tile_edge = vws::WS_EDGE;
  for (int a = 0; a < 3; a++)
    out->origin[a] = w.K[a], out->box_lo[a] = w.lo[a], out->box_hi[a] = w.hi[a];
  out->tiles_used = w.h_ctr[vws::WC_USED];
  out->tiles_cap = w.cap;
  out->shifts_short_of_tiles = w.h_ctr[vws::WC_SHORT];
  out->voxels_forgotten = w.h_ctr[vws::WC_FORGOTTEN];
  return VOFOD_OK;
}

int vofod_world_read(vofod_handle* h, const int32_t lo[3], const int32_t size[3], float* dst, size_t n)
{
  if (!h || !lo || !size || !dst)
    return VOFOD_ERR_INVALID_ARG;
  ApiLock lock(h);
  VCHK(admit(h, NEEDS_NOTHING));
  const vws::Store& w = h->world;
  if (!w.enabled)
    return VOFOD_ERR_NOT_PENDING;
  uint64_t want = 1;
  for (int a = 0; a < 3; a++)
  {
    if (size[a] < 1 || static_cast<int64_t>(lo[a]) + size[a] > INT32_MAX)
      return VOFOD_ERR_INVALID_ARG;
    want *= static_cast<uint64_t>(size[a]);
    if (want > (1ull << 40))
      return VOFOD_ERR_INVALID_ARG;
  }
  if (want != n)
    return VOFOD_ERR_SIZE_MISMATCH;
  DevBuf<uint32_t> tmp;
  HIPCHK(tmp.alloc(n));
  KLAUNCH_AS(h, "k_world_gather", vws::k_world_gather, world_grid(n), dim3(vws::WS_THREADS), world_view(h), reinterpret_cast<const uint32_t*>(h->d_map.p), h->mg.sx, h->mg.sy, h->mg.sz,
             static_cast<int64_t>(w.K[0]), static_cast<int64_t>(w.K[1]), static_cast<int64_t>(w.K[2]), static_cast<int64_t>(lo[0]), static_cast<int64_t>(lo[1]), static_cast<int64_t>(lo[2]),
             static_cast<uint32_t>(size[0]), static_cast<uint32_t>(size[1]), static_cast<uint64_t>(n), tmp.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(dst, tmp, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VOFOD_OK;
}

int vofod_ingest_apriori(vofod_handle* h, const char* filename, const float tf_xyz[3], double yaw_deg, const float sim_correction[3], size_t* n_loaded, size_t* n_voxels)
{
  if (!h || !filename || !tf_xyz || !sim_correction)
    return VOFOD_ERR_INVALID_ARG;
  size_t n = 0;
  int r = vofod_load_cloud(filename, nullptr, 0, &n);
  if (r != VOFOD_OK && r != VOFOD_ERR_CAPACITY)
    return r;
  std::vector<float> xyz(3 * n), cent;
  if (n && (r = vofod_load_cloud(filename, xyz.data(), n, &n)) != VOFOD_OK)
    return r;
  vt::ingest_apriori_points(xyz, tf_xyz, yaw_deg, sim_correction, h->sp.voxel_size, cent);  // init-time host work, as in the reference
  if (n_loaded)
    *n_loaded = n;
  if (n_voxels)
    *n_voxels = cent.size() / 3;
  return vofod_load_apriori(h, cent.data(), cent.size() / 3);
}

}  // extern "C"
