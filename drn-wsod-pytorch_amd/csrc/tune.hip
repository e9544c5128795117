// The library-wide tuning state (tune.h): g_tune, the rule of every drn_tune knob, and the GEMM tile pin.  Host code only.
#include "tune.h"
#include "../../include/drn_wsod.h"

#include <limits.h>

DrnTune g_tune;  // (tune.h)

// drn_tune's knobs: {id, field of g_tune, accept}.  accept(v, cur) gives what the field holds after drn_tune(id, v) - `cur` where
// the knob ignores v; drn_tune returns the field's previous value.  Rows without a field do all of it themselves: accept(v, 0)
// is drn_tune's result.  The rules differ knob by knob on purpose (tests and tools rely on them): tests/test_tune_cpu.py.
namespace {
struct TuneRow { int id; int DrnTune::*field; int (*accept)(int v, int cur); };
int tune_truthy(int v, int) { return v != 0; }
template <int LO, int HI> int tune_range(int v, int cur) { return v >= LO && v <= HI ? v : cur; }
template <int... S> int tune_one_of(int v, int cur) { return ((v == S) || ...) ? v : cur; }
const TuneRow kTuneRows[] = {
    {1, &DrnTune::gemm_persistent, tune_truthy},
    {2, &DrnTune::sgd_grid, tune_range<8, 65535>},
    {3, &DrnTune::gemm_group_rows, tune_range<0, 64>},
    {4, &DrnTune::roi_map64, [](int v, int cur) { return v == 1 ? 512 : tune_one_of<0, 256, 512, 1024>(v, cur); }},
    {5, &DrnTune::conv_ksplit, tune_truthy},
    {6, &DrnTune::gemm_tail_split, tune_truthy},
    {7, &DrnTune::conv_ks_tiles, tune_range<0, INT_MAX>},
    {8, &DrnTune::conv_k2_tiles, [](int v, int) { return v; }},
    {9, nullptr, [](int v, int) {  // returns the pixel threshold while the kernel is on, 0 while it is off
       const int old = g_tune.conv_patch ? g_tune.conv_patch_min : 0;
       g_tune.conv_patch = v != 0;
       if (v > 1) g_tune.conv_patch_min = v;
       return old;
     }},
    {10, &DrnTune::roi_cpb, [](int v, int cur) { return v >= 1 && v <= 64 && (v & (v - 1)) == 0 ? v : cur; }},
    {11, &DrnTune::roi_prefetch, tune_truthy},
    {12, &DrnTune::gemm_pingpong, [](int v, int) { return v < 0 ? 0 : v; }},
    {13, &DrnTune::fp8_k64, tune_truthy},
    {14, &DrnTune::roi_map64_a, tune_truthy},
    {15, &DrnTune::roi_lds_kb, tune_range<60, 154>},
    {18, &DrnTune::gemm_nwg, [](int v, int cur) { return v >= 0 && v % 8 == 0 && v <= 4096 ? v : cur; }},
    {19, nullptr, [](int v, int) {  // 3 = setting 1 with ONE sub-group of ROIs per walking-kernel block (tests)
       const int old = g_tune.roi_lane;
       g_tune.roi_walk_nsg = v == 3 ? 1 : 2;
       g_tune.roi_lane = v < 0 ? 0 : v == 3 ? 1 : v > 2 ? 2 : v;
       return old;
     }},
    {20, &DrnTune::sgdp_ep4, tune_truthy},
    {22, &DrnTune::roi_lane_reps, tune_range<0, 64>},
    {23, &DrnTune::conv_ring, tune_one_of<0, 1, 64, 128>},
    {24, &DrnTune::conv_pp, tune_range<0, INT_MAX>},
    {25, &DrnTune::pp8, tune_range<0, 2>},
    {26, &DrnTune::pp8_stages, tune_one_of<3, 4, 5>},
    {27, &DrnTune::pp8_var, [](int v, int cur) { return v >= 0 && v <= 10 && (v & 3) != 3 ? v : cur; }},
    {28, nullptr, [](int, int) { return drn_tune_pp8_profile_dump(); }},
    {29, &DrnTune::pp8_wide, tune_range<0, 2>},
    {30, &DrnTune::pp8_wvar, tune_one_of<0, 1, 4, 5, 8, 9, 13>},
    {31, nullptr, [](int v, int) {  // 0..2 = the setting; 10 / 11 = profile builds on / off; 12 = print and clear their counters
       const int old = g_tune.roi_st;
       g_tune.roi_st = tune_range<0, 2>(v, old);
       if (v == 10 || v == 11) g_tune.roi_st_prof = v == 10;
       if (v == 12 && drn_tune_roi_st_profile_dump() != 0) return -1;
       return old;
     }},
    {32, &DrnTune::msm_wave, tune_truthy},
};
}  // namespace

extern "C" {

// tuning/test hook: pin the GEMM tile (0 restores the heuristic). Returns the previous value.
int drn_gemm_set_tile(int tile) {
  const int old = g_tune.force_tile;
  if (tile == 0 || tile == 64 || tile == 128 || tile == 255 || tile == 256) g_tune.force_tile = tile;
  return old;
}

// tuning knobs (A/B measurements and tests; defaults are the measured best).  Returns the previous value or -1.
int drn_tune(int knob, int value) {
  for (const TuneRow& row : kTuneRows) {
    if (row.id != knob) continue;
    if (!row.field) return row.accept(value, 0);
    const int old = g_tune.*row.field;
    g_tune.*row.field = row.accept(value, old);
    return old;
  }
  return -1;
}

}  // extern "C"
