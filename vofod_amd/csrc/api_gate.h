// The admission rule of the C API (included by vofod_hip.hip in front of the entry points): which call is admitted in which
// handle state, written once.  Every entry point that takes a handle opens with an ApiLock and states what it needs of the
// handle's state in one admit(...) line, placed where that test stands among the entry's own argument and state tests - the
// first refusal in the body's order is the one the caller gets.  `grep "admit("` lists the contract include/vofod.h promises.
#pragma once

namespace
{

// The handle's mutex for the length of the call and, unless told otherwise, the handle's device made current.  The setters and
// status calls that touch no device state (set_dynamic_params, get_status, set_point_motion, set_raycast_motion,
// set_raycast_exact, world_status) take the lock alone.
struct ApiLock
{
  enum Device
  {
    SELECT_DEVICE,
    LOCK_ONLY
  };
  explicit ApiLock(vofod_handle* h, Device d = SELECT_DEVICE) : lck(h->mtx)
  {
    if (d == SELECT_DEVICE)
      (void)hipSetDevice(h->device);
  }
  std::scoped_lock<std::mutex> lck;
};

// What a call needs of the handle's state.  A submitted batch reads the voxel map, its images and (ticket 0) the synchronous
// workspace until it is collected; a raycast or sepclusters pass between begin and finish owns the raycast map or the cluster
// list.  Calls that would overwrite that state are refused with VOFOD_ERR_BUSY instead of racing it (the reference serialises
// them on m_voxels_mtx; a batch in flight is "inside the lock" until vofod_batch_collect).
enum Need : unsigned
{
  NEEDS_NOTHING = 0,
  WS0_FREE = 1u << 0,        // the synchronous workspace is free: ticket 0 is not in flight
  MAP_UNREAD = 1u << 1,      // no submitted batch reads the voxel map
  NO_RAYCAST_PASS = 1u << 2, // no raycast pass is pending
  NO_SEP_PASS = 1u << 3,     // no sepclusters pass is pending
  RAY_FLOATS = 1u << 4,      // the raycast map holds floats: no EXACT raycast pass is pending (a pending one holds its units there)
};

// the need of a call that names one of the maps: floats in the raycast map for VOFOD_MAP_RAYCAST, nothing for the others
inline unsigned floats_in(int which) { return which == VOFOD_MAP_RAYCAST ? RAY_FLOATS : NEEDS_NOTHING; }

inline bool any_batch_in_flight(vofod_handle* h)
{
  for (int t = 0; t < vofod_handle::MAX_INFLIGHT; t++)
    if (h->slot(t)->pending)
      return true;
  return false;
}

// VOFOD_OK, or VOFOD_ERR_BUSY with the handle's error text set; the needs are tested in the order of their bits.  `entry` ("map
// shift") is put in front of the text of a pending pass by the entries that name themselves there; `note` follows the text of the
// exact pass.
inline int admit(vofod_handle* h, unsigned needs, const char* entry = nullptr, const char* note = nullptr)
{
  const std::string prefix = entry ? std::string(entry) + ": " : std::string();
  if ((needs & WS0_FREE) && h->ws.pending)
    h->err = "ticket 0 is in flight on the synchronous workspace: collect it first";
  else if ((needs & MAP_UNREAD) && any_batch_in_flight(h))
    h->err = "a submitted batch still reads the voxel map: collect it first";
  else if ((needs & NO_RAYCAST_PASS) && h->raycast_pending)
    h->err = prefix + "a raycast pass is pending: finish it first";
  else if ((needs & NO_SEP_PASS) && h->sep_pending)
    h->err = prefix + "a sepclusters pass is pending: finish it first";
  else if ((needs & RAY_FLOATS) && h->raycast_pending && h->ray_pass_exact)
    h->err = std::string("the raycast map holds the units of a pending exact pass: finish it first") + (note ? note : "");
  else
    return VOFOD_OK;
  return VOFOD_ERR_BUSY;
}

// the detections vofod_detection_points would answer for are gone (the ids start again, or they belong to a map that was replaced)
inline void forget_detections(vofod_handle* h)
{
  for (int t = 0; t < vofod_handle::MAX_INFLIGHT; t++)
    h->slot(t)->det_valid = false;
}

}  // namespace
