// MFMA GEMM (NT / TN) for gfx950: the 64x64 / 128x128 register-staged and the 256x256 LDS-DMA / ping-pong kernels on the
// mainloops of mfma_mainloop.h, the fused dW + SGD forms, and their entry points.
//
// Replaces on the reference path: F.linear of fc6/fc7 and the predictor Linears
// (projects/WSL/wsl/modeling/roi_heads/box_head.py:82-91, fast_rcnn.py:493-527, :1363-1387).
#include "mfma_mainloop.h"
#include "tune.h"
#include "../../include/drn_wsod.h"

namespace {

struct GemmParams {
  const char* A;
  const char* B;
  float* C;
  int M, N, K;
  long lda, ldb, ldc;  // elements
  int k_slabs_per_split;
  long c_split_stride;  // elements
  int accumulate;
  // fused optimizer step (drn_gemm_tn_sgd, SgdPipe): the previous tile's update rides in the next tile's mainloop
  float* sgd_w;
  float* sgd_mom;
  bf16_t* sgd_shadow;  // bf16 compute copy of W (same layout) or null
  const SgdSeg* sgd_seg;  // lr / wd of this tensor, read on the device (a replayed hipGraph follows the schedule)
  float sgd_momentum, sgd_grad_scale;
  int sgd_first_step;
  long sgd_ld;  // SGDP (drn_gemm_tn_sgd): row pitch of sgd_w / sgd_mom / sgd_shadow in elements (C = the bf16 gradient bucket, ldc)
  int c_bf16;  // C holds bf16 (gradient buckets that cross xGMI in bf16); splits == 1, no accumulate
  int nsplit;  // number of K-splits (the persistent kernel's grid is 1-D: it cannot read it from gridDim.y)
  int gm;      // tile rows per group of the XCD patch mapping (tile_coords)
  // TN operand (drn_gemm_tn): B is given as Bt [kb_rows][ldb] row-major - the contraction index is the ROW index - and the
  // 256x256 ping-pong kernels read it through transposing LDS reads (ds_read_b64_tr_b16); rows >= kb_rows read as zeros
  int kb_rows;
  // ACC (drn_gemm_tn_acc_sgd): fp32 [M][sgd_acc_ld] gradient accumulator of the window's earlier micro-steps, added to the
  // fp32 accumulators in front of the bf16 rounding; read only
  const float* sgd_acc;
  long sgd_acc_ld;
  // GUARD (drn_gemm_tn_sgd_guard / drn_gemm_tn_acc_sgd_guard): state[0] of drn_loss_guard, one uniform load per workgroup
  const int* sgd_guard;
};

template <int DT, int BM, int BN>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = DT == DRN_BF16 ? 2 : 4;
  constexpr int MI = BM / 64, NJ = BN / 64;
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  // (tile, split) are linearised together before the XCD remap: one XCD then owns a contiguous
  // run of tiles of ONE K-split (a 4 x tiles_n patch), so its L2 fetches each operand panel once.
  const int tiles = tiles_m * tiles_n;
  const int logical = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, tiles * gridDim.y);
  const int split = logical / tiles;
  int tm, tn;
  tile_coords(logical - split * tiles, tiles_m, tiles_n, tm, tn, p.gm);
  const int bm = tm * BM, bn = tn * BN;
  const int nslab = p.K * ES / 128;
  const int s0 = split * p.k_slabs_per_split;
  const int s1 = s0 + p.k_slabs_per_split < nslab ? s0 + p.k_slabs_per_split : nslab;
  const RowLoader la = make_row_loader(p.A, bm, p.M, BM, p.lda * ES);
  const RowLoader lb = make_row_loader(p.B, bn, p.N, BN, p.ldb * ES);
  f32x16_t acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  mainloop<DT, BM, BN>(acc, smem, la, lb, s0, s1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  float* C = p.C + (long)split * p.c_split_stride;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = bn + wn * (BN / 2) + j * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = bm + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < p.M && n < p.N) {
          if (p.c_bf16) {
            ((bf16_t*)p.C)[(long)m * p.ldc + n] = f32_to_bf16(acc[i][j][r]);
          } else {
            float* dst = C + (long)m * p.ldc + n;
            *dst = p.accumulate ? *dst + acc[i][j][r] : acc[i][j][r];
          }
        }
      }
    }
}

// ------------------------------------------------------------------------------------------------
// 256x256 tile, 8 waves (2 x 4, 128x64 per wave = 4x2 MFMA 32x32 tiles), LDS-DMA staging.
//   * global -> LDS by `buffer_load_dwordx4 ... lds` (no staging VGPRs, hardware bounds check keeps the free zero
//     fill of ragged edges).  An LDS-DMA wave-instruction writes base + lane*16, i.e. 8 rows x 128 B, so the LDS
//     image is row-major and the XOR swizzle is applied to the per-lane SOURCE k-slot (same involution on the
//     ds_read side): the 8 lanes of a row still read one whole 128-B line.
//   * 2 LDS stages of 64 KB; the next slab's 8 loads per thread are issued before the current slab is consumed and
//     stay in flight across the barrier: counted `s_waitcnt vmcnt(8)` + raw s_barrier (a __syncthreads() would
//     drain them).
//   * operands are swapped in the MFMA (D^T = B.A^T) so a lane holds 4 consecutive output columns per register
//     quad: the epilogue issues 16-B stores (4x fewer store instructions; the fc6 dW output is 411 MB).
// Buffer descriptor of the TN operand's tile: Bt [kb_rows][ldb] from column bn on; rows beyond kb_rows (the K padding) and
// everything behind the matrix read as zeros.  (Columns beyond N inside a row run into the next row: finite values that
// only reach output columns >= N, which are never stored.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_tn_rsrc(const char* B, int bn, int kb_rows, long ldb_bytes, int es) {
  long bytes = (long)kb_rows * ldb_bytes - (long)bn * es;
  if (bytes < 0) bytes = 0;
  return __builtin_amdgcn_make_buffer_rsrc((void*)(B + (long)bn * es), 0, (unsigned)bytes, 0x00020000);
}

template <int DT, bool PIPE, int PP = 0, bool TN = false>
__global__ __launch_bounds__(512) void gemm_nt256_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = DT == DRN_BF16 ? 2 : 4;
  constexpr int BM = 256, BN = 256, MI = 4, NJ = 2;
  constexpr int A_BYTES = BM * 128, STAGE = (BM + BN) * 128;
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  // (tile, split) are linearised together before the XCD remap: one XCD then owns a contiguous
  // run of tiles of ONE K-split (a 4 x tiles_n patch), so its L2 fetches each operand panel once.
  const int tiles = tiles_m * tiles_n;
  const int logical = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, tiles * gridDim.y);
  const int split = logical / tiles;
  int tm, tn;
  tile_coords(logical - split * tiles, tiles_m, tiles_n, tm, tn, p.gm);
  const int bm = tm * BM, bn = tn * BN;
  const int nslab = p.K * ES / 128;
  const int s0 = split * p.k_slabs_per_split;
  const int s1 = s0 + p.k_slabs_per_split < nslab ? s0 + p.k_slabs_per_split : nslab;
  const RowLoader la = make_row_loader(p.A, bm, p.M, BM, p.lda * ES);
  const RowLoader lb = make_row_loader(p.B, bn, p.N, BN, p.ldb * ES);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  // per-thread source offsets of its 4 A-chunks and 4 B-chunks (row = i*64 + tid/8, k-slot pre-swizzled)
  unsigned voa[4], vob[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned row = i * 64 + (tid >> 3), ks = (tid & 7) ^ ((row >> 1) & 7);
    voa[i] = row * la.ld_bytes + ks * 16;
    vob[i] = row * lb.ld_bytes + ks * 16;
  }
  auto issue = [&](char* stage, int slab) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      char* dst = stage + (i * 64 + wave * 8) * 128;  // wave-uniform LDS base of this 1-KB piece
      __builtin_amdgcn_raw_ptr_buffer_load_lds(la.rsrc, (__attribute__((address_space(3))) void*)dst, 16, voa[i], slab * 128, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(lb.rsrc, (__attribute__((address_space(3))) void*)(dst + A_BYTES), 16, vob[i], slab * 128, 0, 0);
    }
  };
  f32x16_t acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  auto load_frags = [&](const char* buf, int ks, i32x4_t (&fa)[MI], i32x4_t (&fb)[NJ]) {
    const int slot = ks * 2 + (lane >> 5);
#pragma unroll
    for (int i = 0; i < MI; ++i) fa[i] = *(const i32x4_t*)(buf + swz(wm * 128 + i * 32 + (lane & 31), slot));
#pragma unroll
    for (int j = 0; j < NJ; ++j) fb[j] = *(const i32x4_t*)(buf + A_BYTES + swz(wn * 64 + j * 32 + (lane & 31), slot));
  };
  auto mma_all = [&](const i32x4_t (&fa)[MI], const i32x4_t (&fb)[NJ]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) mma_step<DT>(acc[i][j], fb[j], fa[i]);  // swapped: D^T[n][m]
  };
  if (s0 < s1) {
    if constexpr (PP) {
      unsigned pva[4], pvb[4];
      pp_offsets<TN>(la.ld_bytes, lb.ld_bytes, tid, pva, pvb);
      const unsigned bstep = TN ? 64u * lb.ld_bytes : 128u;
      const __amdgpu_buffer_rsrc_t rbb = TN ? make_tn_rsrc(p.B, bn, p.kb_rows, p.ldb * ES, ES) : lb.rsrc;
      pp_issue_first(smem, la.rsrc, rbb, pva, pvb, wave, s0, bstep);
      pp_mainloop<DT, PP, TN>(acc, smem, la.rsrc, rbb, pva, pvb, s0, s1, lane, wave, bstep);
    } else if constexpr (PIPE) {
      // Software-pipelined schedule: fragments of k-step k+1 are read while the MFMAs of k-step k run (two register
      // sets), and ONE barrier per slab - placed after the slab's last fragment read and before its last MFMA block -
      // serves both as "slab s+1 has landed" and "everybody is done reading slab s"; the DMA of slab s+2 is issued
      // right behind it and has a whole slab of MFMAs to land.
      i32x4_t fa0[MI], fb0[NJ], fa1[MI], fb1[NJ];
      issue(smem, s0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (s0 + 1 < s1) issue(smem + STAGE, s0 + 1);
      load_frags(smem, 0, fa0, fb0);
      // each group below = 6 fragment reads for the NEXT k-step + 8 MFMAs of the current one; the scheduling groups
      // interleave them one read per MFMA so a wave's matrix instructions never queue behind its own LDS reads
      // (+5 % on the fc6 shapes).  The last slab is peeled so the steady-state body is one branch-free block, which
      // lets the 4th group also take the next slab's DMA issue (8 buffer_load..lds) under its MFMAs.
#define DRN_INTERLEAVE()                                                     \
  _Pragma("unroll") for (int q_ = 0; q_ < 6; ++q_) {                           \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        \
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                        \
  }                                                                          \
  __builtin_amdgcn_sched_group_barrier(0x008, 2, 0)
      int s = s0;
      for (; s + 1 < s1; ++s) {
        char* cur = smem + ((s - s0) & 1) * STAGE;
        char* nxt = smem + (((s - s0) & 1) ^ 1) * STAGE;
        load_frags(cur, 1, fa1, fb1);
        mma_all(fa0, fb0);
        DRN_INTERLEAVE();
        load_frags(cur, 2, fa0, fb0);
        mma_all(fa1, fb1);
        DRN_INTERLEAVE();
        load_frags(cur, 3, fa1, fb1);
        mma_all(fa0, fb0);
        DRN_INTERLEAVE();
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // slab s+2 into the stage everybody just finished reading; past the end the last slab is fetched again into
        // a stage nobody will read (keeps this block branch-free)
        issue(cur, s + 2 < s1 ? s + 2 : s1 - 1);
        load_frags(nxt, 0, fa0, fb0);
        mma_all(fa1, fb1);
#pragma unroll
        for (int q_ = 0; q_ < 6; ++q_) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
      {  // last slab of this split: nothing left to fetch
        char* cur = smem + ((s - s0) & 1) * STAGE;
        load_frags(cur, 1, fa1, fb1);
        mma_all(fa0, fb0);
        DRN_INTERLEAVE();
        load_frags(cur, 2, fa0, fb0);
        mma_all(fa1, fb1);
        DRN_INTERLEAVE();
        load_frags(cur, 3, fa1, fb1);
        mma_all(fa0, fb0);
        DRN_INTERLEAVE();
        mma_all(fa1, fb1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the redundant tail fetches must land before LDS is reused
      }
#undef DRN_INTERLEAVE
    } else {
      issue(smem, s0);
      for (int s = s0; s < s1; ++s) {
        char* cur = smem + ((s - s0) & 1) * STAGE;
        char* nxt = smem + (((s - s0) & 1) ^ 1) * STAGE;
        if (s + 1 < s1) {
          issue(nxt, s + 1);
          asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          i32x4_t fa[MI], fb[NJ];
          load_frags(cur, ks, fa, fb);
          mma_all(fa, fb);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
    }
  }
  // D^T layout: lane -> m (A row) = lane&31, register r -> n = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float* C = p.C + (long)split * p.c_split_stride;
  const bool vec_ok = (p.ldc & 3) == 0 && (((uintptr_t)C) & 15) == 0;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = bm + wm * 128 + i * 32 + (lane & 31);
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = bn + (TN ? j * 128 + wn * 32 : wn * 64 + j * 32) + 8 * q + 4 * (lane >> 5);
        float* dst = C + (long)m * p.ldc + n;
        f32x4_t v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
        if (p.c_bf16) {
          bf16_t* d16 = (bf16_t*)p.C + (long)m * p.ldc + n;
          if (vec_ok && n + 4 <= p.N) {
            uint2 o;
            o.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
            o.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
            *(uint2*)d16 = o;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (n + e < p.N) d16[e] = f32_to_bf16(v[e]);
          }
        } else if (vec_ok && n + 4 <= p.N) {
          if (p.accumulate) { const f32x4_t o = *(const f32x4_t*)dst; v += o; }
          *(f32x4_t*)dst = v;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n + e < p.N) dst[e] = p.accumulate ? dst[e] + v[e] : v[e];
        }
      }
  }
}

// ------------------------------------------------------------------------------------------------
// PERSISTENT form of the 256x256 kernel (same tile, same LDS-DMA pipeline, same scheduling groups): the grid is one
// workgroup per CU and every workgroup walks its share of the (tile, K-split) list.
//   * A one-tile workgroup gives its CU back when it retires; with an HBM-streaming kernel (the optimizer pass) on
//     another stream, that kernel's small, long-lived workgroups take the freed registers and the next 128-KB-LDS /
//     400-VGPR GEMM workgroup cannot be placed there any more: the GEMM loses whole CUs ("overlap" measured as time
//     slicing in round 1).  A persistent workgroup keeps its CU; the streaming kernel runs in what is left over
//     (112 VGPRs per SIMD beside two 200-VGPR waves).
//   * The first slab of the NEXT tile is issued (LDS-DMA into stage 0) before the current tile's epilogue stores, so the
//     epilogue and the prologue latency overlap instead of costing a workgroup launch per tile.
// Work order: workgroup (xcd = bid & 7, idx = bid >> 3) takes elements idx, idx + nwg/8, ... of its XCD's contiguous
// chunk of the logical (tile, split) list - the same elements in the same temporal order as the one-tile grid under the
// dispatcher's round-robin, so the L2 reuse pattern of the XCD patch mapping is unchanged.
struct GemmWork { int bm, bn, s0, s1, split; __amdgpu_buffer_rsrc_t ra, rb; };  // one (tile, K-split) work item

// PAIR (round 3): TWO independent GEMMs in one persistent launch - the first `pair_wg0` workgroups of every XCD walk
// problem 0, the others problem 1 (drn_gemm_nt_pair splits them by work).  For two launches that each leave CUs idle:
// the fc7 weight gradient (128 tiles: half the CUs in one round) and the fc7 dX (64 tiles x 4 K-splits of half the
// length), 46 + 41 us one after the other.  (Two concurrent launches on a forked stream do the same on paper and cost
// 250 us in the captured step: the graph executor starts the branch late.)
// ACC (with SGDP; drn_gemm_tn_acc_sgd): the closing micro-step of a gradient-accumulation window - the tile's fp32 accumulators
// take the matching run of the fp32 gradient accumulator (p.sgd_acc) in the MFMA layout, where a lane owns 4 consecutive columns
// per register quad and a wave reads whole 128-byte lines of 32 rows, right in front of the bf16 rounding: one fp32 add, one
// rounding, the sum drn_gemm_tn (fp32 C, accumulate) + drn_cast2d would give.  The loads are plain epilogue loads behind the next
// tile's first slab (the compiler counts its own wait; the fragment registers are dead here), so SgdPipe and its vmcnt ladder
// are untouched.
template <int DT, int PP = 0, bool TN = false, bool PAIR = false, bool SGDP = false, bool ACC = false, bool GUARD = false>
__global__ __launch_bounds__(512) void gemm_nt256p_kernel(GemmParams p_in, GemmParams p2_in, int pair_wg0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool second = PAIR && (int)(blockIdx.x >> 3) >= pair_wg0;
  const GemmParams p = second ? p2_in : p_in;
  constexpr int ES = DT == DRN_BF16 ? 2 : 4;
  constexpr int BM = 256, BN = 256, MI = 4, NJ = 2;
  constexpr int A_BYTES = BM * 128, STAGE = (BM + BN) * 128;
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int tiles = tiles_m * tiles_n;
  const int total = tiles * p.nsplit;
  const int nslab = p.K * ES / 128;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int bid = blockIdx.x;
  const int per = PAIR ? (second ? (int)(gridDim.x >> 3) - pair_wg0 : pair_wg0) : (int)(gridDim.x >> 3);
  const int xcd = bid & 7, q = total >> 3, r = total & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  const int len = q + (xcd < r ? 1 : 0);
  int j = PAIR ? (second ? (bid >> 3) - pair_wg0 : (bid >> 3)) : (bid >> 3);
  if (j >= len) return;
  const unsigned lda_b = (unsigned)(p.lda * ES), ldb_b = (unsigned)(p.ldb * ES);
  unsigned voa[4], vob[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned row = i * 64 + (tid >> 3), ks = (tid & 7) ^ ((row >> 1) & 7);
    voa[i] = row * lda_b + ks * 16;
    vob[i] = row * ldb_b + ks * 16;
  }
  using Work = GemmWork;
  auto setup = [&](int logical, Work& w) {
    w.split = logical / tiles;
    int tm, tn;
    tile_coords(logical - w.split * tiles, tiles_m, tiles_n, tm, tn, p.gm);
    w.bm = tm * BM;
    w.bn = tn * BN;
    w.s0 = w.split * p.k_slabs_per_split;
    w.s1 = w.s0 + p.k_slabs_per_split < nslab ? w.s0 + p.k_slabs_per_split : nslab;
    w.ra = make_row_loader(p.A, w.bm, p.M, BM, p.lda * ES).rsrc;
    w.rb = TN ? make_tn_rsrc(p.B, w.bn, p.kb_rows, p.ldb * ES, ES) : make_row_loader(p.B, w.bn, p.N, BN, p.ldb * ES).rsrc;
  };
  const unsigned bstep = TN ? 64u * ldb_b : 128u;
  auto issue = [&](const Work& w, char* stage, int slab) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      char* dst = stage + (i * 64 + wave * 8) * 128;  // wave-uniform LDS base of this 1-KB piece
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w.ra, (__attribute__((address_space(3))) void*)dst, 16, voa[i], slab * 128, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w.rb, (__attribute__((address_space(3))) void*)(dst + A_BYTES), 16, vob[i], slab * 128, 0, 0);
    }
  };
  f32x16_t acc[MI][NJ];
  auto load_frags = [&](const char* buf, int ks, i32x4_t (&fa)[MI], i32x4_t (&fb)[NJ]) {
    const int slot = ks * 2 + (lane >> 5);
#pragma unroll
    for (int i = 0; i < MI; ++i) fa[i] = *(const i32x4_t*)(buf + swz(wm * 128 + i * 32 + (lane & 31), slot));
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) fb[jj] = *(const i32x4_t*)(buf + A_BYTES + swz(wn * 64 + jj * 32 + (lane & 31), slot));
  };
  auto mma_all = [&](const i32x4_t (&fa)[MI], const i32x4_t (&fb)[NJ]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) mma_step<DT>(acc[i][jj], fb[jj], fa[i]);  // swapped: D^T[n][m]
  };
  unsigned pva[4], pvb[4];
  if constexpr (PP) pp_offsets<TN>(lda_b, ldb_b, tid, pva, pvb);
  Work cur;
  setup(base + j, cur);
  if (cur.s0 < cur.s1) {
    if constexpr (PP) pp_issue_first(smem, cur.ra, cur.rb, pva, pvb, wave, cur.s0, bstep);
    else issue(cur, smem, cur.s0);
  }
  // SGDP: the optimizer step of the tile finished last rides in the next tile's mainloop (SgdPipe above)
  [[maybe_unused]] SgdPipe sp;
  [[maybe_unused]] bool have_prev = false;
  if constexpr (SGDP) {
    sp.w = p.sgd_w; sp.m = p.sgd_mom; sp.g = (const bf16_t*)p.C; sp.s = p.sgd_shadow;
    sp.step = (unsigned)(8 * p.sgd_ld * 4); sp.gstep = (unsigned)(8 * p.ldc * 2);
    sp.lr = p.sgd_seg->lr; sp.wd = p.sgd_seg->wd; sp.mom = p.sgd_momentum; sp.gs = p.sgd_grad_scale;
    sp.first = p.sgd_first_step;
    sp.skip = 0;
    if constexpr (GUARD) sp.skip = __builtin_amdgcn_readfirstlane(p.sgd_guard[0]);
    sp.off = sp.goff = 0;
  }
  for (;;) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) acc[i][jj][rr] = 0.f;
    const int s0 = cur.s0, s1 = cur.s1;
    if constexpr (PP) {
      if constexpr (SGDP) {
        if (have_prev) pp_mainloop<DT, PP, TN, true, GUARD>(acc, smem, cur.ra, cur.rb, pva, pvb, s0, s1, lane, wave, bstep, &sp);
        else pp_mainloop<DT, PP, TN>(acc, smem, cur.ra, cur.rb, pva, pvb, s0, s1, lane, wave, bstep);
      } else if (s0 < s1) pp_mainloop<DT, PP, TN>(acc, smem, cur.ra, cur.rb, pva, pvb, s0, s1, lane, wave, bstep);
    } else if (s0 < s1) {
      i32x4_t fa0[MI], fb0[NJ], fa1[MI], fb1[NJ];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // slab s0 (issued ahead of the previous tile's epilogue) has landed
      __builtin_amdgcn_s_barrier();
      if (s0 + 1 < s1) issue(cur, smem + STAGE, s0 + 1);
      load_frags(smem, 0, fa0, fb0);
#define DRN_INTERLEAVE()                                                     \
  _Pragma("unroll") for (int q_ = 0; q_ < 6; ++q_) {                           \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        \
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                        \
  }                                                                          \
  __builtin_amdgcn_sched_group_barrier(0x008, 2, 0)
      int s = s0;
      for (; s + 1 < s1; ++s) {
        char* cs = smem + ((s - s0) & 1) * STAGE;
        char* nx = smem + (((s - s0) & 1) ^ 1) * STAGE;
        load_frags(cs, 1, fa1, fb1);
        mma_all(fa0, fb0);
        DRN_INTERLEAVE();
        load_frags(cs, 2, fa0, fb0);
        mma_all(fa1, fb1);
        DRN_INTERLEAVE();
        load_frags(cs, 3, fa1, fb1);
        mma_all(fa0, fb0);
        DRN_INTERLEAVE();
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        issue(cur, cs, s + 2 < s1 ? s + 2 : s1 - 1);
        load_frags(nx, 0, fa0, fb0);
        mma_all(fa1, fb1);
#pragma unroll
        for (int q_ = 0; q_ < 6; ++q_) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
      {  // last slab of this (tile, split)
        char* cs = smem + ((s - s0) & 1) * STAGE;
        load_frags(cs, 1, fa1, fb1);
        mma_all(fa0, fb0);
        DRN_INTERLEAVE();
        load_frags(cs, 2, fa0, fb0);
        mma_all(fa1, fb1);
        DRN_INTERLEAVE();
        load_frags(cs, 3, fa1, fb1);
        mma_all(fa0, fb0);
        DRN_INTERLEAVE();
        mma_all(fa1, fb1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the redundant tail fetches must land before LDS is reused
      }
#undef DRN_INTERLEAVE
    }
    // ---- next work item: its first slab goes out before this tile's epilogue stores
    j += per;
    const bool more = j < len;
    Work nxt;
    if (more) {
      setup(base + j, nxt);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave is done reading both stages
      if (nxt.s0 < nxt.s1) {
        if constexpr (PP) pp_issue_first(smem, nxt.ra, nxt.rb, pva, pvb, wave, nxt.s0, bstep);
        else issue(nxt, smem, nxt.s0);
      }
    }
    const int bm = cur.bm, bn = cur.bn;
    // D^T layout: lane -> m (A row) = lane&31, register r -> n = (r&3) + 8*(r>>2) + 4*(lane>>5)
    if (p.c_bf16 && (p.ldc & 7) == 0 && (((uintptr_t)p.C) & 15) == 0) {
      // bf16 output (the fc6 dW gradient bucket: one epilogue per 32 K-slabs, 128 KB per tile): the MFMA layout gives a
      // lane 4 consecutive columns of 32 DIFFERENT rows, i.e. 8-byte stores scattered over 32 lines per instruction.
      // The tile goes through the free LDS stage instead, one 128-row half at a time (64 KB), and leaves as 16-byte
      // pieces of whole 512-byte rows.  8-byte chunk c of row r sits at chunk c ^ ((r & 31) << 1): the 32 rows of a
      // store instruction spread over all banks, and a reader's 16-byte pair stays adjacent.
      // LDS accesses are inline asm: the compiler orders every ds access it can see behind ALL pending LDS-DMA
      // (s_waitcnt vmcnt(0)), i.e. behind the next tile's slab that was just issued into the OTHER stage
      const unsigned ep = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)(smem + STAGE);
      bf16_t* C16 = (bf16_t*)p.C;
      // (the ~40 LDS / global offsets below are functions of the thread id alone: without this the compiler hoists them
      // out of the tile loop and keeps them alive through the mainloop - 204 -> 229 VGPRs, which would cost the conv
      // workgroups their place beside this kernel, see DESIGN 'trunk beside the GEMMs')
      int lane_e = lane, tid_e = tid;
      asm volatile("" : "+v"(lane_e), "+v"(tid_e));
      if (!more) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); }
      if constexpr (ACC) {
        static_assert(TN && SGDP, "the accumulating epilogue belongs to the fused TN dW + SGD launch (whole tiles)");
        const float* ga = p.sgd_acc + (long)(bm + wm * 128 + (lane_e & 31)) * p.sgd_acc_ld + bn + wn * 32 + 4 * (lane_e >> 5);
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const float* gi = ga + (long)(i * 32) * p.sgd_acc_ld;
          f32x4_t o[NJ][4];
#pragma unroll
          for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) o[jj][qq] = __builtin_nontemporal_load((const f32x4_t*)(gi + jj * 128 + 8 * qq));
#pragma unroll
          for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[i][jj][4 * qq + e] = acc[i][jj][4 * qq + e] + o[jj][qq][e];
        }
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (wm == half) {
#pragma unroll
          for (int i = 0; i < MI; ++i) {
            const int row = i * 32 + (lane_e & 31);
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
              for (int qq = 0; qq < 4; ++qq) {
                const int c = (TN ? jj * 32 + wn * 8 : wn * 16 + jj * 8) + 2 * qq + (lane_e >> 5);
                const unsigned long long o =
                    (unsigned long long)((uint32_t)f32_to_bf16(acc[i][jj][4 * qq]) | ((uint32_t)f32_to_bf16(acc[i][jj][4 * qq + 1]) << 16)) |
                    ((unsigned long long)((uint32_t)f32_to_bf16(acc[i][jj][4 * qq + 2]) | ((uint32_t)f32_to_bf16(acc[i][jj][4 * qq + 3]) << 16)) << 32);
                asm volatile("ds_write_b64 %0, %1" ::"v"(ep + row * 512 + ((c ^ ((row & 31) << 1)) << 3)), "v"(o) : "memory");
              }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (SGDP && (p.c_bf16 & 2)) {
          // (the fused dW + SGD launch: whole tiles only, and its 256 registers are spent anyway - four reads in flight per
          // trip instead of one read, one wait, one store eight times over)
#pragma unroll 1
          for (int it = 0; it < 8; it += 4) {
            i32x4_t v0, v1, v2, v3;
            const int r0_ = (it * 512 + tid_e) >> 5, pc_ = tid_e & 31;  // rows r0_, r0_ + 16, + 32, + 48: the same (row & 31) parity class shifts by 16
            asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                         : "v"(ep + (r0_) * 512 + ((pc_ ^ ((r0_) & 31)) << 4)), "v"(ep + (r0_ + 16) * 512 + ((pc_ ^ ((r0_ + 16) & 31)) << 4)),
                           "v"(ep + (r0_ + 32) * 512 + ((pc_ ^ ((r0_ + 32) & 31)) << 4)), "v"(ep + (r0_ + 48) * 512 + ((pc_ ^ ((r0_ + 48) & 31)) << 4))
                         : "memory");
            bf16_t* dst = C16 + (long)(bm + half * 128 + r0_) * p.ldc + bn + pc_ * 8;
            *(i32x4_t*)dst = v0;
            *(i32x4_t*)(dst + 16 * p.ldc) = v1;
            *(i32x4_t*)(dst + 32 * p.ldc) = v2;
            *(i32x4_t*)(dst + 48 * p.ldc) = v3;
          }
        } else
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {
          const int idx = it * 512 + tid_e;
          const int row = idx >> 5, pc = idx & 31;
          const int m = bm + half * 128 + row, n = bn + pc * 8;
          i32x4_t v;
          asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(ep + row * 512 + ((pc ^ (row & 31)) << 4)) : "memory");
          if (m < p.M) {
            bf16_t* dst = C16 + (long)m * p.ldc + n;
            if (n + 8 <= p.N) {
              *(i32x4_t*)dst = v;
            } else {
              const bf16_t* e8 = (const bf16_t*)&v;
#pragma unroll
              for (int e = 0; e < 8; ++e)
                if (n + e < p.N) dst[e] = e8[e];
            }
          }
        }
        if (half == 0) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); }
      }
    } else {
      float* C = p.C + (long)cur.split * p.c_split_stride;
      const bool vec_ok = (p.ldc & 3) == 0 && (((uintptr_t)C) & 15) == 0;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int m = bm + wm * 128 + i * 32 + (lane & 31);
        if (m >= p.M) continue;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int n = bn + (TN ? jj * 128 + wn * 32 : wn * 64 + jj * 32) + 8 * qq + 4 * (lane >> 5);
            float* dst = C + (long)m * p.ldc + n;
            f32x4_t v = {acc[i][jj][4 * qq], acc[i][jj][4 * qq + 1], acc[i][jj][4 * qq + 2], acc[i][jj][4 * qq + 3]};
            if (p.c_bf16) {
              bf16_t* d16 = (bf16_t*)p.C + (long)m * p.ldc + n;
              if (vec_ok && n + 4 <= p.N) {
                uint2 o;
                o.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
                o.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
                *(uint2*)d16 = o;
              } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (n + e < p.N) d16[e] = f32_to_bf16(v[e]);
              }
            } else if (vec_ok && n + 4 <= p.N) {
              if (p.accumulate) { const f32x4_t o = *(const f32x4_t*)dst; v += o; }
              *(f32x4_t*)dst = v;
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (n + e < p.N) dst[e] = p.accumulate ? dst[e] + v[e] : v[e];
            }
          }
      }
    }
    if constexpr (SGDP) {  // this tile's update: in the next tile's mainloop, or in the drain below
      sp.off = (unsigned)(((long)(bm + wave) * p.sgd_ld + bn + lane * 4) * 4);
      sp.goff = (unsigned)(((long)(bm + wave) * p.ldc + bn + lane * 4) * 2);
      have_prev = true;
    }
    if (!more) break;
    cur = nxt;
  }
  if constexpr (SGDP) {
    // drain: the update of the workgroup's LAST tile, two chunks (rows) in flight per trip
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's gradient stores of this tile have reached L2
    for (unsigned c = 0; c < 32; c += 2) {
      SgdRegs q0, q1;
      sgdp_load(sp, q0, sp.off + c * sp.step, sp.goff + c * sp.gstep);
      sgdp_load(sp, q1, sp.off + (c + 1) * sp.step, sp.goff + (c + 1) * sp.gstep);
      sgdp_apply_store<GUARD>(sp, q0, sp.off + c * sp.step);
      sgdp_apply_store<GUARD>(sp, q1, sp.off + (c + 1) * sp.step);
    }
  }
}

template <int DT, int BM, int BN>
int launch_gemm(const GemmParams& p, int splits, hipStream_t st) {
  const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  constexpr int smem = 2 * (BM + BN) * 128;
  auto k = gemm_nt_kernel<DT, BM, BN>;
  if (smem > 48 * 1024 && !drn_launch::allow_lds((const void*)k, smem)) return DRN_ERR_LAUNCH;
  hipLaunchKernelGGL(k, dim3(tiles, splits), dim3(256), smem, st, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// Every launch of the 256x256 kernels: 512 threads on both 64-KB LDS stages; the kernel, its grid and its arguments vary.
template <class Kernel, class... Args>
int launch256(Kernel k, dim3 grid, hipStream_t st, const Args&... args) {
  constexpr int smem = 2 * 512 * 128;
  if (!drn_launch::allow_lds((const void*)k, smem)) return DRN_ERR_LAUNCH;
  hipLaunchKernelGGL(k, grid, dim3(512), smem, st, args...);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// (dtype, DRN_TUNE_GEMM_PINGPONG) -> the <DT, PP> template arguments of the pipelined 256x256 kernels:
// f(integral_constant<int, DT>, integral_constant<int, PP>).  Only bf16 has ping-pong variants (PP 1 / 2 / 3).
template <class F>
int with_gemm256_variant(int dtype, int pingpong, F&& f) {
  using bf16 = std::integral_constant<int, DRN_BF16>;
  if (dtype == DRN_BF16 && pingpong == 1) return f(bf16{}, std::integral_constant<int, 1>{});
  if (dtype == DRN_BF16 && pingpong == 2) return f(bf16{}, std::integral_constant<int, 2>{});
  if (dtype == DRN_BF16 && pingpong == 3) return f(bf16{}, std::integral_constant<int, 3>{});
  return dtype == DRN_BF16 ? f(bf16{}, std::integral_constant<int, 0>{})
                           : f(std::integral_constant<int, DRN_F32>{}, std::integral_constant<int, 0>{});
}

using drn_launch::cu_count;

// Tile rows per group of the XCD patch mapping (tile_coords).  One XCD (32 CUs) works on 32 consecutive tiles of its
// chunk at a time: GM rows x 32/GM columns.  4-row groups were tuned on the fc6 forward in round 1 (PMC: 1214 -> 612 MB).
// For the fc6 dW (8 x 196 tiles) 8-row groups - every B panel streamed once per XCD instead of twice - were measured in
// round 2 and are WORSE: FETCH_SIZE 734 MB vs 646 MB (profiles/r2_04_pmc_fc6_dw_gm8.json vs r2_03_..._gm4.json): the
// 8-MB A operand (dP1^T) does not stay in the 4-MB L2 between rounds and is re-read 6 times per XCD (mostly from the
// Infinity Cache - the counter sits on the fabric side of L2, so it counts those too); step rate unchanged.  4 stays.
static int gemm256_group_rows(int M, int N, int splits) {
  (void)M; (void)N; (void)splits;
  return g_tune.gemm_group_rows > 0 ? g_tune.gemm_group_rows : 4;
}

// number of workgroups of the persistent launch, or 0 when the one-tile grid should be used
static int persistent_grid(long total) {
  if (!g_tune.gemm_persistent) return 0;
  const int nwg = g_tune.gemm_nwg > 0 ? g_tune.gemm_nwg : (cu_count() / 8) * 8;
  return (nwg >= 8 && total > nwg) ? nwg : 0;
}

}  // namespace

// Tail balancing of a persistent 256x256 launch (see drn_gemm_nt): number of leading output columns that form an exact
// number of rounds of `nwg` resident workgroups; N when nothing is peeled.
static long tail_split_main_cols(int M, int N, int splits, int nwg) {
  const int tm = (M + 255) / 256, tn = (N + 255) / 256;
  const long wg256 = (long)tm * tn * splits, rem = wg256 % nwg;
  if (!g_tune.gemm_tail_split || splits != 1 || rem == 0 || rem * 8 > (long)nwg * 3) return N;
  int a = nwg, b = tm;
  while (b) { const int t = a % b; a = b; b = t; }
  const int step = nwg / a;                   // tile columns per exact multiple of nwg tiles
  const int cols_main = (tn / step) * step;
  if (cols_main > 0 && (long)(tn - cols_main) * tm == rem) return (long)cols_main * 256;
  return N;
}

// shared body of drn_gemm_tn_sgd / drn_gemm_tn_acc_sgd (grad_acc == nullptr: the former, launch and arguments unchanged) and of
// their guarded forms (guard == nullptr: the unguarded instantiations, as before)
static int gemm_tn_sgd_entry(const void* A, const void* Bt, void* grad_bucket, const float* grad_acc, long ld_acc, int M, int N,
                             int K, int kb_rows, long lda, long ldb, long ldc, float* weights, float* momentum_buf, void* shadow,
                             long ld_w, const void* seg_dev, float momentum, int first_step, float grad_scale, const int* guard, void* stream) {
  if (!A || !Bt || !grad_bucket || !weights || !momentum_buf || !seg_dev || M <= 0 || N <= 0 || K <= 0 || kb_rows < 0 ||
      kb_rows > K)
    return DRN_ERR_ARG;
  if (lda < K || ldb < N || ldc < N || ld_w < N) return DRN_ERR_ARG;
  // (alignment is part of the shape class, not an argument error: the caller's unfused pair takes such buffers - ADVICE r4)
  if ((lda * 2) % 16 != 0 || (ldb * 2) % 16 != 0 ||
      (((uintptr_t)A | (uintptr_t)Bt | (uintptr_t)grad_bucket | (uintptr_t)weights | (uintptr_t)momentum_buf | (uintptr_t)shadow) & 15))
    return DRN_ERR_UNSUPPORTED;
  // shape class of the pipelined update: whole K slabs (one 8-row chunk of the previous tile rides in each; with fewer than 32
  // slabs - fewer than 2048 proposals - the rest follows the mainloop, exposed), whole tiles, a bf16 shadow, 32-bit byte
  // offsets, enough tiles for the persistent grid, the ping-pong mainloop
  if (K < 128 || (K & 63) || (M & 255) || (N & 255) || !shadow || (ldc & 7) || (ld_w & 3) || g_tune.gemm_pingpong != 1 ||
      (long)M * ld_w * 4 >= 0xFFFFFFF0L || (long)K * ldb * 2 >= 0xFFFFFFF0L)
    return DRN_ERR_UNSUPPORTED;
  if (grad_acc && ((ld_acc & 3) || (((uintptr_t)grad_acc) & 15) || (long)M * ld_acc * 4 >= 0xFFFFFFF0L)) return DRN_ERR_UNSUPPORTED;
  const long tiles = (long)(M / 256) * (N / 256);
  const int nwg = persistent_grid(tiles);
  if (!nwg) return DRN_ERR_UNSUPPORTED;
  GemmParams p{(const char*)A, (const char*)Bt, (float*)grad_bucket, M, N, K, lda, ldb, ldc, K * 2 / 128, 0, 0,
               weights, momentum_buf, (bf16_t*)shadow, (const SgdSeg*)seg_dev, momentum, grad_scale, first_step};
  p.sgd_ld = ld_w;
  p.c_bf16 = g_tune.sgdp_ep4 ? 3 : 1;  // (bit 1: four-at-a-time epilogue reads)
  p.nsplit = 1;
  p.gm = gemm256_group_rows(M, N, 1);
  p.kb_rows = kb_rows;
  p.sgd_guard = guard;
  hipStream_t st = (hipStream_t)stream;
  if (grad_acc) {
    p.sgd_acc = grad_acc;
    p.sgd_acc_ld = ld_acc;
    return guard ? launch256(gemm_nt256p_kernel<DRN_BF16, 1, true, false, true, true, true>, dim3(nwg), st, p, p, 0)
                 : launch256(gemm_nt256p_kernel<DRN_BF16, 1, true, false, true, true, false>, dim3(nwg), st, p, p, 0);
  }
  return guard ? launch256(gemm_nt256p_kernel<DRN_BF16, 1, true, false, true, false, true>, dim3(nwg), st, p, p, 0)
               : launch256(gemm_nt256p_kernel<DRN_BF16, 1, true, false, true, false, false>, dim3(nwg), st, p, p, 0);
}

extern "C" {

// Columns [0, n0) of an [M, N] output that drn_gemm_nt keeps for its persistent 256x256 launch; the columns from n0 on
// are the ones it peels off into a small-tile launch first (n0 == N: no peel, or another kernel takes the shape).
long drn_gemm_nt_main_cols(int M, int N, int splits) {
  if (M <= 0 || N <= 0 || splits < 1) return N;
  const long wg256 = (long)((M + 255) / 256) * ((N + 255) / 256) * splits;
  if (!((g_tune.force_tile == 256 || (g_tune.force_tile == 0 && wg256 >= 192)))) return N;
  const int nwg = persistent_grid(wg256);
  return nwg ? tail_split_main_cols(M, N, splits, nwg) : N;
}

// C[split][M,N] (fp32) = A[M,K] * B[N,K]^T over this split's K range.  See include/drn_wsod.h.
int drn_gemm_nt(const void* A, const void* B, void* C, int M, int N, int K, long lda, long ldb, long ldc, int dtype,
                int c_dtype, int splits, long c_split_stride, int accumulate, void* stream) {
  if (!A || !B || !C || M < 0 || N < 0 || K < 0) return DRN_ERR_ARG;
  if (M == 0 || N == 0) return DRN_OK;
  const int es = drn_esize(dtype);
  if (dtype != DRN_F32 && dtype != DRN_BF16) return DRN_ERR_ARG;
  if ((K * es) % 128 != 0 || (lda * es) % 16 != 0 || (ldb * es) % 16 != 0 || lda < K || ldb < K) return DRN_ERR_ARG;
  if (((uintptr_t)A | (uintptr_t)B) & 15) return DRN_ERR_ARG;
  if (splits < 1) return DRN_ERR_ARG;
  if (splits > 1 && accumulate) return DRN_ERR_ARG;
  if (c_dtype != DRN_F32 && c_dtype != DRN_BF16) return DRN_ERR_ARG;
  if (c_dtype == DRN_BF16 && (splits != 1 || accumulate)) return DRN_ERR_ARG;
  const int nslab = K * es / 128;
  GemmParams p{(const char*)A, (const char*)B, (float*)C, M, N, K, lda, ldb, ldc, (nslab + splits - 1) / splits,
               c_split_stride, accumulate};
  p.c_bf16 = c_dtype == DRN_BF16;
  p.nsplit = splits;
  p.gm = 4;
  hipStream_t st = (hipStream_t)stream;
  // 256x256 LDS-DMA kernel when it can put >= ~3/4 of the 256 CUs to work (1 workgroup of 128 KB LDS per CU);
  // otherwise the 128x128 / 64x64 register-staged kernels (more, smaller workgroups)
  const long wg256 = (long)((M + 255) / 256) * ((N + 255) / 256) * splits;
  const int force = g_tune.force_tile;
  const dim3 grid256((unsigned)(wg256 / splits), splits);  // one workgroup per 256x256 tile and K-split
  if (force == 255)  // the non-pipelined 256 kernel (kept for A/B comparison)
    return dtype == DRN_BF16 ? launch256(gemm_nt256_kernel<DRN_BF16, false>, grid256, st, p)
                             : launch256(gemm_nt256_kernel<DRN_F32, false>, grid256, st, p);
  if ((force == 256 || (force == 0 && wg256 >= 192)) && (((uintptr_t)C) & 3) == 0) {
    p.gm = gemm256_group_rows(M, N, splits);
    const int nwg = persistent_grid(wg256);
    if (nwg) {
      // Tail balancing.  The persistent kernel runs ceil(tiles / CUs) rounds: the fc6 dW row slab [1024 x 50176] is
      // 4 x 196 = 784 tiles = 3.06 rounds on 256 CUs, i.e. FOUR rounds with 240 CUs idle in the last one (measured:
      // 448 us for two slabs = 8 rounds of 56 us where 6.125 rounds of work exist).  When the last round is less
      // than 3/8 full, whole tile columns are peeled off so that the persistent launch is an exact number of rounds,
      // and the peeled columns (16 tiles of that slab) run first as their own launch of the small-tile kernel - many
      // short workgroups that fill every CU.  Same slab order and the same MFMA per output element in both kernels,
      // so the result is bit-identical to the unsplit launch (test_gemm_tail_split_bit_identical).
      const long n0 = tail_split_main_cols(M, N, splits, nwg);
      if (n0 < N) {
        GemmParams q = p;
        q.B = p.B + n0 * ldb * es;
        q.C = (float*)((char*)p.C + n0 * (p.c_bf16 ? 2 : 4));
        q.N = N - (int)n0;
        const bool small_t = (long)((M + 127) / 128) * ((q.N + 127) / 128) < 128;
        const int rc = dtype == DRN_BF16
                           ? (small_t ? launch_gemm<DRN_BF16, 64, 64>(q, 1, st) : launch_gemm<DRN_BF16, 128, 128>(q, 1, st))
                           : (small_t ? launch_gemm<DRN_F32, 64, 64>(q, 1, st) : launch_gemm<DRN_F32, 128, 128>(q, 1, st));
        if (rc != DRN_OK) return rc;
        p.N = (int)n0;
      }
    }
    return with_gemm256_variant(dtype, g_tune.gemm_pingpong, [&](auto dt, auto pp) {
      constexpr int DT = decltype(dt)::value, PP = decltype(pp)::value;
      return nwg ? launch256(gemm_nt256p_kernel<DT, PP>, dim3(nwg), st, p, p, 0)
                 : launch256(gemm_nt256_kernel<DT, true, PP>, grid256, st, p);
    });
  }
  // 64x64 tiles (4x the workgroups) when 128x128 tiles would not even give every CU one workgroup: these launches are
  // latency-bound per K slab, not MFMA-bound (the joint peel of the fc6 dW, [2048 x 1024] x K 2000: 128 tiles of 128 took
  // 31 us; bit-identical either way)
  const bool small = force == 64 || (force == 0 && (long)((M + 127) / 128) * ((N + 127) / 128) * splits < cu_count());
  if (dtype == DRN_BF16) return small ? launch_gemm<DRN_BF16, 64, 64>(p, splits, st) : launch_gemm<DRN_BF16, 128, 128>(p, splits, st);
  return small ? launch_gemm<DRN_F32, 64, 64>(p, splits, st) : launch_gemm<DRN_F32, 128, 128>(p, splits, st);
}

// C[M,N] = A[M,K] * Bt[K,N]: the B operand given K-major ("TN"), read by the 256x256 ping-pong kernels through
// transposing LDS reads.  Same tile, slab order and MFMA per output element as drn_gemm_nt on a materialised transpose of
// Bt (bit-identical: test_gemm_tn_equals_nt_on_the_transpose).  bf16 only.  See include/drn_wsod.h.
int drn_gemm_tn(const void* A, const void* Bt, void* C, int M, int N, int K, int kb_rows, long lda, long ldb, long ldc,
                int c_dtype, int splits, long c_split_stride, int accumulate, void* stream) {
  if (!A || !Bt || !C || M < 0 || N < 0 || K < 0 || kb_rows < 0 || kb_rows > K) return DRN_ERR_ARG;
  if (M == 0 || N == 0) return DRN_OK;
  if ((K * 2) % 128 != 0 || (lda * 2) % 16 != 0 || (ldb * 2) % 16 != 0 || lda < K || ldb < N) return DRN_ERR_ARG;
  if ((((uintptr_t)A | (uintptr_t)Bt) & 15) || (((uintptr_t)C) & 3)) return DRN_ERR_ARG;
  if (splits < 1 || (splits > 1 && accumulate)) return DRN_ERR_ARG;
  if (c_dtype != DRN_F32 && c_dtype != DRN_BF16) return DRN_ERR_ARG;
  if (c_dtype == DRN_BF16 && (splits != 1 || accumulate)) return DRN_ERR_ARG;
  if ((long)K * ldb * 2 >= 0xFFFFFFF0L) return DRN_ERR_UNSUPPORTED;  // one 32-bit buffer offset spans Bt
  const int nslab = K * 2 / 128;
  GemmParams p{(const char*)A, (const char*)Bt, (float*)C, M, N, K, lda, ldb, ldc, (nslab + splits - 1) / splits,
               c_split_stride, accumulate};
  p.c_bf16 = c_dtype == DRN_BF16;
  p.nsplit = splits;
  p.gm = gemm256_group_rows(M, N, splits);
  p.kb_rows = kb_rows;
  hipStream_t st = (hipStream_t)stream;
  const long wg256 = (long)((M + 255) / 256) * ((N + 255) / 256) * splits;
  if (const int nwg = persistent_grid(wg256)) return launch256(gemm_nt256p_kernel<DRN_BF16, 1, true>, dim3(nwg), st, p, p, 0);
  return launch256(gemm_nt256_kernel<DRN_BF16, true, 1, true>, dim3((unsigned)(wg256 / splits), splits), st, p);
}

// Two independent NT GEMMs (bf16 operands, fp32 outputs) in ONE persistent launch of the 256x256 ping-pong kernel: the
// workgroups of every XCD are divided between the problems in proportion to their work.  Same kernel arithmetic as two
// drn_gemm_nt calls (bit-identical).  Falls back to two calls when a problem is empty or the device has no 8-XCD grid.
int drn_gemm_nt_pair(const void* A0, const void* B0, void* C0, int M0, int N0, int K0, long lda0, long ldb0, long ldc0,
                     int splits0, long stride0, int accumulate0, const void* A1, const void* B1, void* C1, int M1, int N1,
                     int K1, long lda1, long ldb1, long ldc1, int splits1, long stride1, int accumulate1, void* stream) {
  auto two_calls = [&]() {
    const int rc = drn_gemm_nt(A0, B0, C0, M0, N0, K0, lda0, ldb0, ldc0, DRN_BF16, DRN_F32, splits0, stride0, accumulate0, stream);
    return rc != DRN_OK ? rc
                        : drn_gemm_nt(A1, B1, C1, M1, N1, K1, lda1, ldb1, ldc1, DRN_BF16, DRN_F32, splits1, stride1, accumulate1, stream);
  };
  if (M0 <= 0 || N0 <= 0 || M1 <= 0 || N1 <= 0 || !g_tune.gemm_persistent || g_tune.gemm_pingpong != 1 || g_tune.force_tile == 64 || g_tune.force_tile == 128)
    return two_calls();
  auto ok = [](const void* A, const void* B, void* C, int K, long lda, long ldb, int splits, int acc) {
    return A && B && C && K > 0 && (K * 2) % 128 == 0 && (lda * 2) % 16 == 0 && (ldb * 2) % 16 == 0 && lda >= K && ldb >= K &&
           !(((uintptr_t)A | (uintptr_t)B) & 15) && !(((uintptr_t)C) & 3) && splits >= 1 && !(splits > 1 && acc);
  };
  if (!ok(A0, B0, C0, K0, lda0, ldb0, splits0, accumulate0) || !ok(A1, B1, C1, K1, lda1, ldb1, splits1, accumulate1))
    return DRN_ERR_ARG;
  auto mk = [](const void* A, const void* B, void* C, int M, int N, int K, long lda, long ldb, long ldc, int splits, long stride,
               int acc) {
    const int nslab = K * 2 / 128;
    GemmParams p{(const char*)A, (const char*)B, (float*)C, M, N, K, lda, ldb, ldc, (nslab + splits - 1) / splits, stride, acc};
    p.nsplit = splits;
    p.gm = gemm256_group_rows(M, N, splits);
    return p;
  };
  const GemmParams p0 = mk(A0, B0, C0, M0, N0, K0, lda0, ldb0, ldc0, splits0, stride0, accumulate0);
  const GemmParams p1 = mk(A1, B1, C1, M1, N1, K1, lda1, ldb1, ldc1, splits1, stride1, accumulate1);
  const int nwg = (cu_count() / 8) * 8, per = nwg / 8;
  if (per < 2) return two_calls();
  const double w0 = (double)((M0 + 255) / 256) * ((N0 + 255) / 256) * splits0 * p0.k_slabs_per_split;
  const double w1 = (double)((M1 + 255) / 256) * ((N1 + 255) / 256) * splits1 * p1.k_slabs_per_split;
  int wg0 = (int)(per * w0 / (w0 + w1) + 0.5);
  wg0 = wg0 < 1 ? 1 : (wg0 > per - 1 ? per - 1 : wg0);
  return launch256(gemm_nt256p_kernel<DRN_BF16, 1, false, true>, dim3(nwg), (hipStream_t)stream, p0, p1, wg0);
}

// G[M,N] = A[M,K] . Bt[K,N] (bf16, the TN form of drn_gemm_tn) into the bf16 gradient bucket AND W <- SGD(W, momentum_buf, G)
// in the same launch: every workgroup applies the update of the tile it finished last inside the next tile's mainloop
// (SgdPipe).  DRN_ERR_UNSUPPORTED outside its shape class (the caller then runs drn_gemm_tn + drn_sgd_step_block).
int drn_gemm_tn_sgd(const void* A, const void* Bt, void* grad_bucket, int M, int N, int K, int kb_rows, long lda, long ldb,
                    long ldc, float* weights, float* momentum_buf, void* shadow, long ld_w, const void* seg_dev,
                    float momentum, int first_step, float grad_scale, void* stream) {
  return gemm_tn_sgd_entry(A, Bt, grad_bucket, nullptr, 0, M, N, K, kb_rows, lda, ldb, ldc, weights, momentum_buf, shadow, ld_w,
                           seg_dev, momentum, first_step, grad_scale, nullptr, stream);
}

// drn_gemm_tn_sgd under the anomaly guard: guard -> state[0] of drn_loss_guard (device memory, read once per workgroup).
// guard[0] == 0: drn_gemm_tn_sgd's bits.  guard[0] != 0: weights, momentum_buf and shadow keep their bits (the shadow is
// re-derived from the weights it mirrors: it must hold bf16(weights), as FusedSGD keeps it); grad_bucket is written as ever.
int drn_gemm_tn_sgd_guard(const void* A, const void* Bt, void* grad_bucket, int M, int N, int K, int kb_rows, long lda, long ldb,
                          long ldc, float* weights, float* momentum_buf, void* shadow, long ld_w, const void* seg_dev,
                          float momentum, int first_step, float grad_scale, const int* guard, void* stream) {
  if (!guard) return DRN_ERR_ARG;
  return gemm_tn_sgd_entry(A, Bt, grad_bucket, nullptr, 0, M, N, K, kb_rows, lda, ldb, ldc, weights, momentum_buf, shadow, ld_w,
                           seg_dev, momentum, first_step, grad_scale, guard, stream);
}

// The closing micro-step of a gradient-accumulation window (WSL.ITER_SIZE > 1: projects/WSL/tools/train_net.py:100-113 - every
// micro-iteration back-propagates loss / N, the optimizer steps once per window) for the fc6 weight (box_head.py:82-91's fc1) as
// ONE launch: drn_gemm_tn_sgd with G = bf16(grad_acc + A . Bt), the sum formed in fp32 and rounded once.  grad_acc (fp32,
// [M][ld_acc]) holds the window's earlier micro-steps (drn_gemm_tn, fp32 C, accumulate); it is read, never written.
int drn_gemm_tn_acc_sgd(const void* A, const void* Bt, const float* grad_acc, void* grad_bucket, int M, int N, int K, int kb_rows,
                        long lda, long ldb, long ld_acc, long ldc, float* weights, float* momentum_buf, void* shadow, long ld_w,
                        const void* seg_dev, float momentum, int first_step, float grad_scale, void* stream) {
  if (!grad_acc || ld_acc < N) return DRN_ERR_ARG;
  return gemm_tn_sgd_entry(A, Bt, grad_bucket, grad_acc, ld_acc, M, N, K, kb_rows, lda, ldb, ldc, weights, momentum_buf, shadow,
                           ld_w, seg_dev, momentum, first_step, grad_scale, nullptr, stream);
}

// drn_gemm_tn_acc_sgd under the anomaly guard (as drn_gemm_tn_sgd_guard)
int drn_gemm_tn_acc_sgd_guard(const void* A, const void* Bt, const float* grad_acc, void* grad_bucket, int M, int N, int K,
                              int kb_rows, long lda, long ldb, long ld_acc, long ldc, float* weights, float* momentum_buf,
                              void* shadow, long ld_w, const void* seg_dev, float momentum, int first_step, float grad_scale,
                              const int* guard, void* stream) {
  if (!grad_acc || ld_acc < N || !guard) return DRN_ERR_ARG;
  return gemm_tn_sgd_entry(A, Bt, grad_bucket, grad_acc, ld_acc, M, N, K, kb_rows, lda, ldb, ldc, weights, momentum_buf, shadow,
                           ld_w, seg_dev, momentum, first_step, grad_scale, guard, stream);
}

}  // extern "C"
