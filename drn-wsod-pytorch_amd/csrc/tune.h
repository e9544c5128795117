// The tuning state of the library: every knob of drn_tune (include/drn_wsod.h documents them, by id) and the tile pin of
// drn_gemm_set_tile, each with its default.  ONE instance, g_tune, defined in tune.hip - the knobs' one home - next to
// drn_tune's table of {id, field, accept rule}; the other translation units only read it.  Defaults are the measured best.
#pragma once

struct DrnTune {
  int gemm_persistent = 1;   //  1 DRN_TUNE_GEMM_PERSISTENT: 256x256 GEMMs with more work items than CUs loop
  int sgd_grid = 512;        //  2 DRN_TUNE_SGD_GRID: workgroups (x) of the optimizer kernels; measured (tools/overlap_bench.py): 512 -> 6.5 TB/s, 1024 -> 5.8, 256 -> 5.3 on the fc6 slabs
  int gemm_group_rows = 0;   //  3 DRN_TUNE_GEMM_GROUP_ROWS: 0 = default (4)
  int roi_map64 = 512;       //  4 DRN_TUNE_ROI_MAP64: 0 = off, else threads per block (256 / 512 / 1024)
  int conv_ksplit = 1;       //  5 DRN_TUNE_CONV_KSPLIT: 0 = never use the 32x32 wave-K-split kernel
  int gemm_tail_split = 1;   //  6 DRN_TUNE_GEMM_TAIL_SPLIT: peel a nearly empty last round off persistent launches
  int conv_ks_tiles = 0;     //  7 DRN_TUNE_CONV_KS_TILES: largest 64x64-tile count of ONE image that still takes it (0 = CUs / 4)
  int conv_k2_tiles = -1;    //  8 DRN_TUNE_CONV_K2_TILES: largest 64x64-tile count of ONE image for the two-K-group kernel (-1 = 2 x CUs, 0 = off)
  int conv_patch = 1;        //  9 DRN_TUNE_CONV_PATCH: 0 = never use conv3x3_c64_kernel ...
  int conv_patch_min = 32768;  //   ... and its minimum pixels per image (a knob value > 1 sets it; drn_tune returns it while the kernel is on)
  int roi_cpb = 1;           // 10 DRN_TUNE_ROI_CPB: most 8-channel chunks per block of the 64-ROI kernel (power of two)
  int roi_prefetch = 1;      // 11 DRN_TUNE_ROI_PREFETCH: 0/1 - second map buffer, next chunk's slice fetched under the scan
  int gemm_pingpong = 1;     // 12 DRN_TUNE_GEMM_PINGPONG: bf16 256x256 GEMMs run the ping-pong mainloop
  int fp8_k64 = 1;           // 13 DRN_TUNE_FP8_K64: 0 = the K = 16 non-scaled fp8 MFMA (A/B; bf16 rate)
  int roi_map64_a = 0;       // 14 DRN_TUNE_ROI_MAP64_A: 1 = the 64-ROI kernel also for A alone (no A^T)
  int roi_lds_kb = 154;      // 15 DRN_TUNE_ROI_LDS_KB: LDS a 64-ROI pooling block may take
  int gemm_nwg = 0;          // 18 DRN_TUNE_GEMM_NWG: resident workgroups of persistent launches (0 = one per CU); for launches on a CU-masked stream
  int roi_lane = 1;          // 19 DRN_TUNE_ROI_LANE: 0 = the 64-ROI kernel writes A as before, 2 = never the walking kernel ...
  int roi_walk_nsg = 2;      //   ... and the walking kernel's sub-groups of 64 ROIs per block on one-block-per-CU maps (tests: knob value 3 -> 1)
  int sgdp_ep4 = 1;          // 20 DRN_TUNE_SGDP_EPILOGUE: the fused dW + SGD launch's tile epilogue reads LDS four pieces at a time
  int roi_lane_reps = 0;     // 22 DRN_TUNE_ROI_LANE_REPS: groups per block on one-block-per-CU maps (0 = default: 4, fewer while < 2 rounds of blocks)
  int conv_ring = 1;         // 23 DRN_TUNE_CONV_RING: 0 = off, 1 = tile by cost model, 64 / 128 pin 64x64 / 128x128
  int conv_pp = 1;           // 24 DRN_TUNE_CONV_PP: 0 = never run a 1x1 conv on the 256x256 ping-pong GEMM mainloop
  int pp8 = 1;               // 25 DRN_TUNE_PP8: 0 = off, 1 = default class, 2 = every layer in the kernel's class
  int pp8_stages = 5;        // 26 DRN_TUNE_PP8_STAGES: LDS ring stages of the 128x128 form (3 / 4 / 5 = 1 / 2 / 3 slabs in flight)
  int pp8_var = 1;           // 27 DRN_TUNE_PP8_VARIANT: schedule variant (pp8_kernel VAR), A/B knob
                             // 28 DRN_TUNE_PP8_PROFILE: no state (pp8.hip prints and clears its device counters)
  int pp8_wide = 1;          // 29 DRN_TUNE_PP8_WIDE: the 256x128 form: 0 = never, 1 = where it fills the chip, 2 = always
  int pp8_wvar = 4;          // 30 DRN_TUNE_PP8_WIDE_VARIANT: VAR of the 256x128 form (1 = all DMA pieces in phase L1, 4 = no s_setprio, 8 = profile)
  int roi_st = 1;            // 31 DRN_TUNE_ROI_ST: 0 = off, 1 = where it is faster (large maps with enough ROIs), 2 = every map whose slice fits ...
  int roi_st_prof = 0;       //   ... and its profile builds (knob values 10 / 11: on / off; 12: roi.hip prints and clears the counters)
  int msm_wave = 1;          // 32 DRN_TUNE_MSM_WAVE: 0 = the thread-per-row kernel also for C <= 64 (tests, A/B)
  int force_tile = 0;        // drn_gemm_set_tile: 0 = heuristic; 64 / 128 / 256 pin the GEMM tile (tuning + tests)
};

extern __attribute__((visibility("hidden"))) DrnTune g_tune;

// The two knobs that act on device symbols of their own translation unit (called from drn_tune's table):
__attribute__((visibility("hidden"))) int drn_tune_pp8_profile_dump();  // pp8.hip, knob 28: 0, or -1 when the device calls fail
__attribute__((visibility("hidden"))) int drn_tune_roi_st_profile_dump();  // roi.hip, knob 31 value 12: likewise
