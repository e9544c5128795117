// The suppression stage of csrc/nms.hip, shared with the uncapped inference tail (drn_detect_all in detect.hip): greedy NMS of
// candidates that are already in descending score order, over many workgroups.  Not part of the C ABI (exports.map keeps it local).
#pragma once
#include "drn_common.h"

namespace drn_supp {

constexpr int PANEL = 512;         // sorted rows resolved per (mask, scan) launch pair
constexpr long MAX_N = 524288;     // include/drn_wsod.h DRN_NMS_MAX_N

struct SuppressIn {
  const float* boxes;           // [cap][4] in candidate order (never written)
  const int* cls;               // [cap] class of a candidate, or NULL: one class, no offsets
  const int* order;             // [cap] candidate ids by descending score (stable)
  const int* count;             // [1] live candidates n <= cap, on the device
  const float* maxcoord_f;      // [1] largest coordinate as a float, or NULL
  const unsigned* maxcoord_key; // [1] largest coordinate as an ascending-order key (nms.hip's reduction), or NULL
  int per_class_from;           // n >= this: classes suppress only themselves on the raw boxes; below: boxes offset by class
  float thr;
  int limit;                    // keep at most this many (the first ones)
};

// bytes launch_suppress needs for up to cap candidates: 88 * cap + 49152
long suppress_ws_bytes(long cap);

// Leaves the kept candidate ids, in descending score order, in keep32 or keep64 (whichever is not NULL) and their number in n_keep[0].
// 1 + 2 * ceil(cap / PANEL) launches on st, whatever the device-side count is.  ws: 16-byte aligned.
void launch_suppress(const SuppressIn& in, int cap, void* ws, int* keep32, long long* keep64, int* n_keep, hipStream_t st);

}  // namespace drn_supp
