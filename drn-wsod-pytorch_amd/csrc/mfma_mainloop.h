// The MFMA mainloops of the GEMM (gemm.hip) and implicit-GEMM NHWC convolution (conv.hip) kernels for gfx950.
//
// One mainloop serves both and both compute dtypes:
//   * bf16 : v_mfma_f32_32x32x16_bf16, fp32 accumulate  (fast mode; BASELINE configs[1])
//   * fp32 : v_mfma_f32_32x32x2_f32 (exact fp32 fma chain; parity mode, losses within 1e-4)
// Tile BMxBN outputs, K consumed in 128-BYTE slabs per row (64 bf16 / 32 f32), so the LDS image
// and the global->LDS staging are byte-identical for both dtypes; only the MFMA issue differs.
// 256 threads = 4 waves (2x2), each wave owns (BM/2)x(BN/2) as 32x32 MFMA tiles.
// Staging: 16-B buffer loads (hardware bounds check => free zero fill of ragged M/N edges) into
// registers, issued one K-slab ahead, written to a 2-stage XOR-swizzled LDS ring after the MFMAs
// (issue-early / write-late), one barrier per slab. ds_read_b128 is conflict-free under the
// swizzle slot ^= (row>>1)&7 (rows are 128 B, a 256-B bank row holds two).
#pragma once
#include "drn_common.h"
#include "sgd_rule.h"

namespace {

template <int DT>
__device__ __forceinline__ void mma_step(f32x16_t& acc, const i32x4_t& a, const i32x4_t& b) {
  if constexpr (DT == DRN_BF16) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                  acc, 0, 0, 0);
  } else if constexpr (DT == DRN_FP8) {
    // a 16-byte fragment holds 16 fp8 k-values: two K=16 steps of v_mfma_f32_32x32x16_fp8_fp8 (8 bytes per lane each;
    // lanes 0-31 carry k 0-7, lanes 32-63 k 8-15 of a step).  A and B use the same byte -> k assignment, so any
    // assignment is a permutation of the contraction index.
    typedef long i64x2_t __attribute__((ext_vector_type(2)));
    const i64x2_t al = __builtin_bit_cast(i64x2_t, a), bl = __builtin_bit_cast(i64x2_t, b);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(al[0], bl[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(al[1], bl[1], acc, 0, 0, 0);
  } else {
    const f32x4_t af = __builtin_bit_cast(f32x4_t, a), bf = __builtin_bit_cast(f32x4_t, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bf[e], acc, 0, 0, 0);
  }
}

// fp8 at the fp8 RATE (round 3): v_mfma_scale_f32_32x32x64_f8f6f4 with both formats e4m3 and unit E8M0 scales (0x7f = 2^0),
// the only K = 64 fp8 MFMA on gfx950 - the non-scaled 32x32x16 form above runs at the bf16 rate (MI355X_MICROARCH.md,
// matrix-core table).  A lane's 32 operand bytes are two 16-byte fragments of consecutive k-steps; A and B use the same
// (lane half, byte) -> k assignment, so whatever the hardware's assignment is, it is a permutation of the contraction
// index, and fp8 x fp8 products are exact in fp32 (4-bit significands): only the fp32 summation order differs from the
// K = 16 form.
typedef int i32x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void mma_step64_fp8(f32x16_t& acc, const i32x4_t& a0, const i32x4_t& a1, const i32x4_t& b0,
                                               const i32x4_t& b1) {
  const i32x8_t A = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  const i32x8_t B = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, acc, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

template <int ROWS>
__device__ __forceinline__ void lds_store_tile(char* lds, const i32x4_t (&r)[ROWS / 32], int tid) {
  const int slot = tid & 7, r0 = tid >> 3;
#pragma unroll
  for (int p = 0; p < ROWS / 32; ++p) *(i32x4_t*)(lds + swz(r0 + 32 * p, slot)) = r[p];
}

// Plain row-major operand [rows][ld] read through a bounds-checked buffer descriptor.
struct RowLoader {
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned ld_bytes;
  template <int ROWS>
  __device__ __forceinline__ void load(i32x4_t (&r)[ROWS / 32], int slab, int tid) const {
    const unsigned slot = tid & 7, r0 = tid >> 3;
#pragma unroll
    for (int p = 0; p < ROWS / 32; ++p)
      r[p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (r0 + 32 * p) * ld_bytes + slot * 16, slab * 128, 0);
  }
};

__device__ __forceinline__ RowLoader make_row_loader(const char* base, long row0, int rows_total, int rows_tile,
                                                     long ld_bytes) {
  RowLoader l;
  long rem = (long)rows_total - row0;
  if (rem > rows_tile) rem = rows_tile;
  if (rem < 0) rem = 0;
  l.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(base + row0 * ld_bytes), 0, (unsigned)(rem * ld_bytes), 0x00020000);
  l.ld_bytes = (unsigned)ld_bytes;
  return l;
}

// Register-staged mainloop of the 64x64 / 128x128 kernels (GEMM and conv share it).  These tiles do little MFMA work
// per K-slab (one to four MFMAs per wave and k-step), so a slab's cost is the latency of its global loads unless they
// are issued far ahead: the staging registers form a statically indexed ring of DEPTH slabs - while slab i is
// multiplied out of LDS, slab i+DEPTH is being fetched and slab i+1 (fetched DEPTH-1 iterations ago) moves from its
// registers into the other LDS stage.
// STAGES = 1 (the 64x64 conv): ONE 16-KB LDS stage, refilled between two barriers, and a 3-deep register ring.  Measured
// (tools/coexist_bench.py and an LDS-size probe): a workgroup shares a CU with a 256x256 GEMM workgroup (128 KB LDS,
// 2 x 200 VGPRs per SIMD) only with < 32 KB of LDS and <= 112 registers per wave; the two-stage version is exactly 32 KB
// and 120 registers, so every conv launch of the frozen trunk used to wait for a GEMM workgroup to retire (a chain of ten
// res4 convs beside the fc6 GEMM: 475 us instead of 190).
#ifndef CONV_DEPTH1
#define CONV_DEPTH1 4  // register-ring depth of the single-LDS-stage 64x64 conv (98 VGPRs; 5 -> 114 > the 112 that co-reside with a GEMM workgroup)
#endif
// Register-staged mainloop (global -> ring of DEPTH register sets -> LDS -> MFMA).  The slab loop runs in two parts:
// a STEADY STATE of whole groups of DEPTH slabs in which every slab issues the loads of slab i + DEPTH and stores the
// registers of slab i + 1 unconditionally, then the last < 2 * DEPTH slabs with the bounds checks.  With the checks inside
// the only loop (round 1 / first half of round 2) the compiler's wait-count pass lost track of the ring across the
// branches and put `s_waitcnt vmcnt(0)` in front of every LDS store - it waited for the loads issued in the SAME
// iteration, i.e. the ring prefetched one slab ahead whatever its depth (which is why ring depth 3 / 4 / 5 all measured
// ~0.55 us per slab).  Branch-free, the waits become counted (vmcnt = loads of the DEPTH - 1 younger slabs).
template <int DT, int BM, int BN, class ALoader, class BLoader, int STAGES = 2, bool K64 = true>
__device__ __forceinline__ void mainloop(f32x16_t (&acc)[BM / 64][BN / 64], char* smem, ALoader& la,
                                         const BLoader& lb, int s0, int s1, int tid = threadIdx.x) {
  // tid: 0..255 within the four waves that share this tile's LDS stage (conv_nhwc_k2_kernel runs two such groups)
  constexpr int MI = BM / 64, NJ = BN / 64;
  constexpr int A_BYTES = BM * 128, STAGE = STAGES == 2 ? (BM + BN) * 128 : 0;
  constexpr int DEPTH = STAGES == 1 ? CONV_DEPTH1 : (BM <= 64 ? 4 : 3);
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  i32x4_t ra[DEPTH][BM / 32], rb[DEPTH][BN / 32];
  const int n = s1 - s0;
  if (n <= 0) return;
#pragma unroll
  for (int d = 0; d < DEPTH; ++d)
    if (d < n) {
      la.template load<BM>(ra[d], s0 + d, tid);
      lb.template load<BN>(rb[d], s0 + d, tid);
    }
  lds_store_tile<BM>(smem, ra[0], tid);
  lds_store_tile<BN>(smem + A_BYTES, rb[0], tid);
  __syncthreads();
  auto slab = [&](auto dtag, int i, auto fulltag) {
    constexpr int d = decltype(dtag)::value;
    constexpr bool FULL = decltype(fulltag)::value;
    char* cur = smem + (i & 1) * STAGE;
    char* nxt = smem + ((i & 1) ^ 1) * STAGE;
    if (FULL || i + DEPTH < n) {  // ring slot d held slab i, which already sits in LDS
      la.template load<BM>(ra[d], s0 + i + DEPTH, tid);
      lb.template load<BN>(rb[d], s0 + i + DEPTH, tid);
    }
    if constexpr (DT == DRN_FP8 && K64) {  // two k-steps per MFMA (K = 64 scaled form: the fp8 rate)
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        i32x4_t fa[2][MI], fb[2][NJ];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int slot = (k2 * 2 + h) * 2 + (lane >> 5);
#pragma unroll
          for (int ii = 0; ii < MI; ++ii)
            fa[h][ii] = *(const i32x4_t*)(cur + swz(wm * (BM / 2) + ii * 32 + (lane & 31), slot));
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            fb[h][j] = *(const i32x4_t*)(cur + A_BYTES + swz(wn * (BN / 2) + j * 32 + (lane & 31), slot));
        }
#pragma unroll
        for (int ii = 0; ii < MI; ++ii)
#pragma unroll
          for (int j = 0; j < NJ; ++j) mma_step64_fp8(acc[ii][j], fa[0][ii], fa[1][ii], fb[0][j], fb[1][j]);
      }
      // keep a slab's MFMAs in the slab (an empty volatile asm that "uses" the accumulators): left alone, the compiler
      // sinks the register-only K = 64 MFMAs out of their blocks to the end of the unrolled slab group and holds every
      // slab's fragments live until then (208 VGPRs for the 64x64 tile instead of ~120: no longer co-resident with a
      // 256x256 GEMM workgroup)
#pragma unroll
      for (int ii = 0; ii < MI; ++ii)
#pragma unroll
        for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(acc[ii][j]));
    } else {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      i32x4_t fa[MI], fb[NJ];
      const int slot = ks * 2 + (lane >> 5);
#pragma unroll
      for (int ii = 0; ii < MI; ++ii) fa[ii] = *(const i32x4_t*)(cur + swz(wm * (BM / 2) + ii * 32 + (lane & 31), slot));
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        fb[j] = *(const i32x4_t*)(cur + A_BYTES + swz(wn * (BN / 2) + j * 32 + (lane & 31), slot));
#pragma unroll
      for (int ii = 0; ii < MI; ++ii)
#pragma unroll
        for (int j = 0; j < NJ; ++j) mma_step<DT>(acc[ii][j], fa[ii], fb[j]);
    }
    }
    if (STAGES == 1) __syncthreads();  // every wave is done reading the only stage
    if (FULL || i + 1 < n) {
      lds_store_tile<BM>(nxt, ra[(d + 1) % DEPTH], tid);
      lds_store_tile<BN>(nxt + A_BYTES, rb[(d + 1) % DEPTH], tid);
    }
    __syncthreads();
  };
  int base = 0;
  for (; base + 2 * DEPTH <= n; base += DEPTH)  // every i here has i + DEPTH < n (and i + 1 < n)
    static_for<DEPTH>([&](auto dtag) { slab(dtag, base + decltype(dtag)::value, std::true_type{}); });
  for (; base < n; base += DEPTH)
    static_for<DEPTH>([&](auto dtag) {
      const int i = base + decltype(dtag)::value;
      if (i < n) slab(dtag, i, std::false_type{});
    });
}

// ------------------------------------------------------------------------------------------------
// PING-PONG mainloop of the 256x256 kernels (round 3; bf16).  Same tile, same wave layout (2 x 4 waves, 128x64 outputs per
// wave as 4x2 MFMA 32x32 tiles), same MFMA and the same k order per output element as the pipelined mainloop it replaces
// (bit-identical results), another SCHEDULE.  What the round-3 PMC passes said about the old one
// (profiles/r3_00_pmc_fwd.json, _dw.json): the MFMA pipes are 64 % / 56 % busy at the sustained clock, every wave is
// parked at a wait / barrier 40 % of its cycles and stalled at issue another 40-44 %, the LDS array is active 24 % of the
// CU cycles and sees no bank conflicts - operand FEED, not LDS bandwidth.  In the old loop all eight waves run the same
// stream in lock-step: the eight LDS-DMA issues of a slab (60-185 cycles each once the phase also carries fragment
// reads) sit in ONE k-step group of every wave at the same time, and at the single barrier per slab both waves of a SIMD
// are parked together, so nobody feeds the matrix pipe.  Here the two waves that share a SIMD (wave w and w + 4: the two
// rows of the 2 x 4 layout) run HALF A PHASE APART: a K slab is four phases of
//     [fragment reads + 2 LDS-DMA issues]  barrier  [8 MFMAs = one 64x32 quadrant x K 64, s_setprio 1]  barrier
// and the lower wave row enters the loop one barrier late, so while one wave of a SIMD multiplies, its partner reads
// fragments and issues DMA - the pipe always has a wave in its matrix section (cdna_hip_programming.md 8-phase
// template, restated for 32x32x16 MFMAs and the D^T epilogue of this file).
// LDS: a stage (64 KB) is four half tiles of 16 KB, each the rows ONE phase starts to read: A0 = the first 64 rows of both
// wave rows' 128-row blocks, B0 = the first 32 rows of the four wave columns' 64-row blocks, B1, A1 the second halves.
// Phase p of slab t stages ONE half tile of slab t + 1 (A0, B0, B1, A1: the order they are first read), 16 DMA pieces of
// 1 KB spread over the slab instead of one burst; a counted vmcnt(4) in phases 4, 1 and 2 retires exactly the half tile the
// NEXT phase starts to read and leaves the two younger ones in flight across the barriers.
// Hazards (the lower wave row runs one barrier interval late): a half tile is read one phase after the wait that
// retires it (every wave's wait precedes a barrier the reader passes); a half tile of stage b^1 is re-staged at phase p
// of slab t when its last fragment read was phase <= p of slab t - 1 - six or more barriers earlier.
constexpr int PP_A0 = 0, PP_B0 = 16384, PP_B1 = 32768, PP_A1 = 49152, PP_STAGE = 65536;

// per-thread source offsets of its two 16-byte chunks of every half tile (index = half * 2 + piece): the LDS image of a
// half tile is row-major [128][128 B], piece `pc` of thread tid lands in LDS row pc * 64 + tid / 8, slot tid & 7, and
// fetches the k-slot pre-swizzled with that row (same involution as the fragment reads)
//
// TN = true (round 3, the fc6 weight gradient reading the pooled matrix A [R][C*49] itself instead of a materialised A^T):
// the B operand arrives as Bt [k][n] row-major and is consumed through ds_read_b64_tr_b16, which hands lane l the 4-element
// COLUMN (l & 15) of a [4 k][16 n] block whose rows the 16 lanes of its group address freely, 8 bytes each.
//   * Wave columns: wave wn owns the 32-column blocks wn of the tile's two 128-column halves (b0: n = wn * 32 .., b1:
//     n = 128 + wn * 32 ..; the NT form owns 64 adjacent columns), so that the half tiles B0 / B1 of the staging order are
//     whole 256-byte row segments of Bt.
//   * LDS image of a half tile: 16 pieces of 1 KB, piece (k-step ks, quarter kq) = Bt rows ks * 16 + 4 * kq + j (j = 0..3)
//     x 128 columns, row pitch 256 B, the 32-byte column units u of row j stored at u ^ 2j.  One LDS-DMA instruction
//     fills one piece lane-linearly from four FULL 256-byte row segments (the first version fetched 16 rows x 64 bytes
//     per instruction and ran the fc6 dW slab at 206 us against 178 us for the NT form).
//   * A fragment half (k = 8 * (g >> 1) + 4 * i + j for lane group g) is one ds_read_b64_tr_b16: lanes 0-31 read piece
//     kq = i, lanes 32-63 piece kq = 2 + i, each group its 4 rows x 32 bytes at unit (2 * wn + (g & 1)) ^ 2j - the 32 lanes
//     of an LDS cycle cover 8 different units = all 64 banks once.
template <bool TN = false>
__device__ __forceinline__ void pp_offsets(unsigned lda_b, unsigned ldb_b, int tid, unsigned (&voa)[4], unsigned (&vob)[4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const unsigned row = pc * 64 + (tid >> 3), ks = (tid & 7) ^ ((row >> 1) & 7);
      const unsigned ga = pc * 128 + h * 64 + (tid >> 3);                             // A row: wave row pc, half h
      voa[h * 2 + pc] = ga * lda_b + ks * 16;
      if constexpr (TN) {
        const unsigned L = tid & 63, wv = tid >> 6;          // piece f = pc * 8 + wave: (ks = f >> 2, kq = f & 3)
        const unsigned ks_f = pc * 2 + (wv >> 2), kq_f = wv & 3;
        const unsigned j = L >> 4, pos = L & 15, u = (pos >> 1) ^ (2 * j);  // LDS row j, 16-byte position pos of 16
        const unsigned k = ks_f * 16 + kq_f * 4 + j;
        vob[h * 2 + pc] = k * ldb_b + h * 256 + u * 32 + (pos & 1) * 16;
      } else {
        const unsigned gb = (2 * pc + (tid >> 8)) * 64 + h * 32 + ((tid >> 3) & 31);  // B row: wave column 2 pc + tid / 256
        vob[h * 2 + pc] = gb * ldb_b + ks * 16;
      }
    }
}

template <int WHICH>  // 0: A0, 1: B0, 2: B1, 3: A1 - one half tile = 2 DMA pieces per thread
__device__ __forceinline__ void pp_issue(char* stage, __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb,
                                         const unsigned (&voa)[4], const unsigned (&vob)[4], int wave, int slab,
                                         unsigned bstep = 128) {  // bytes a K slab advances in B: 128 (NT) or 64 rows (TN)
  constexpr int off = WHICH == 0 ? PP_A0 : WHICH == 1 ? PP_B0 : WHICH == 2 ? PP_B1 : PP_A1;
  constexpr bool isA = WHICH == 0 || WHICH == 3;
  constexpr int h = (WHICH == 2 || WHICH == 3) ? 1 : 0;
#pragma unroll
  for (int pc = 0; pc < 2; ++pc) {
    char* dst = stage + off + (pc * 64 + wave * 8) * 128;  // wave-uniform LDS base of this 1-KB piece
    __builtin_amdgcn_raw_ptr_buffer_load_lds(isA ? ra : rb, (__attribute__((address_space(3))) void*)dst, 16,
                                             isA ? voa[h * 2 + pc] : vob[h * 2 + pc], isA ? slab * 128 : slab * bstep, 0, 0);
  }
}

#define PP_BARRIER()                        \
  do {                                      \
    __builtin_amdgcn_sched_barrier(0);      \
    __builtin_amdgcn_s_barrier();           \
    __builtin_amdgcn_sched_barrier(0);      \
  } while (0)

// prologue half: the four half tiles of slab `slab` into stage 0 (the persistent kernel issues it ahead of the previous
// tile's epilogue)
__device__ __forceinline__ void pp_issue_first(char* smem, __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb,
                                               const unsigned (&voa)[4], const unsigned (&vob)[4], int wave, int slab,
                                               unsigned bstep = 128) {
  pp_issue<0>(smem, ra, rb, voa, vob, wave, slab, bstep);
  pp_issue<1>(smem, ra, rb, voa, vob, wave, slab, bstep);
  pp_issue<2>(smem, ra, rb, voa, vob, wave, slab, bstep);
  pp_issue<3>(smem, ra, rb, voa, vob, wave, slab, bstep);
}

// ---- optimizer step of the PREVIOUS tile inside this tile's mainloop (round 4: drn_gemm_tn_sgd) ------------------------------
// The fc6 weight gradient leaves its GEMM as a bf16 tile of the gradient bucket (the persistent kernel's LDS-staged
// epilogue).  Instead of a second kernel that streams w / momentum / gradient / shadow behind it - HBM-bound phases with the
// matrix pipes idle, or a co-resident kernel competing for the same power budget in bursts - every workgroup applies the
// update of the tile it finished LAST while it multiplies the next one: a tile is 256 rows x 1 KB of fp32 weights, a K slab
// is 1/32 of the mainloop, so slab i carries chunk i = 8 rows (one per wave; a lane owns 4 consecutive parameters): three
// 16/16/8-byte loads (w, momentum, the bf16 gradient the workgroup itself wrote - visible after the vmcnt(0) + barrier at
// the head of the mainloop) issued in phase 1 of slab i, ~30 VALU instructions and three stores in phase 3 of slab i + 1,
// i.e. in the fragment-read phases, while the SIMD's other wave is in its MFMA phase.  HBM traffic becomes a steady
// stream under the MFMA work instead of a burst between launches, and the gradient is read back from L2, not from HBM.
// All of it is inline asm: the mainloop's LDS-DMA pipeline lives on hand-counted vmcnt waits, vector memory operations
// retire in order, and every wait below is the old count plus the optimizer operations issued behind the piece it guards:
//   phase 1 / 2: vmcnt(4) -> vmcnt(7)   (3 loads of this slab's phase 1)      phase 4: vmcnt(4) -> vmcnt(7) from slab 1 on
//   (3 stores of phase 3);  chunk i - 1's loads have 18 (slab 1: 15) younger operations when phase 3 of slab i needs them.
// Same arithmetic, element for element, as sgd_kernel on the bf16 bucket: both run sgd_rule.h (bit-identical: tests).
// GUARD (the anomaly guard, drn_loss_guard): a skipped step keeps ALL SIX memory operations of a chunk and selects the stored
// VALUES - w_old, m_old and the shadow word of w_old (the shadow is bf16(w) by construction) - so every count above holds
// unchanged; a predicated store would change what each wait guards.  The flag is wave-uniform (SgdPipe::skip).
struct SgdPipe {
  float* w; float* m; const bf16_t* g; bf16_t* s;  // bases (wave-uniform); in-place update
  unsigned off, step;    // byte offset of this lane's 16 B in chunk 0 of the tile (fp32 arrays), bytes per chunk (8 rows)
  unsigned goff, gstep;  // the same in the bf16 gradient bucket (8 B per lane); the shadow uses off / 2, step / 2
  float lr, wd, mom, gs;
  int first;
  int skip;  // GUARD: the step's loss was not finite - every chunk stores back what it loaded
};
typedef float f32x2_t_ __attribute__((ext_vector_type(2)));
struct SgdRegs { f32x4_t w, m; f32x2_t_ g; };

// (plain, compiler-visible accesses: the compiler's own counted vmcnt wait in front of the first use is exact - it counts
// the LDS-DMA pieces as the vector memory operations they are.  A first version issued them as inline asm with hand-placed
// waits: the compiler, taking an asm output for valid at once, spilled the registers to scratch right behind the loads.)
__device__ __forceinline__ void sgdp_load(const SgdPipe& sp, SgdRegs& r, unsigned off, unsigned goff) {
  r.w = __builtin_nontemporal_load((const f32x4_t*)((const char*)sp.w + off));
  r.m = __builtin_nontemporal_load((const f32x4_t*)((const char*)sp.m + off));
  r.g = __builtin_nontemporal_load((const f32x2_t_*)((const char*)sp.g + goff));
}
template <bool GUARD = false>
__device__ __forceinline__ void sgdp_apply_store(const SgdPipe& sp, const SgdRegs& r, unsigned off) {
#pragma clang fp contract(off)
  const f32x4_t gg = sgd_unpack_bf16x4(__builtin_bit_cast(u32x2_t, r.g));
  f32x4_t nb, nw;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const SgdNew u = sgd_rule(r.w[e], r.m[e], gg[e] * sp.gs, sp.lr, sp.wd, sp.mom, sp.first);
    nb[e] = u.b;
    nw[e] = u.w;
  }
  if constexpr (GUARD) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      nb[e] = sp.skip ? r.m[e] : nb[e];
      nw[e] = sp.skip ? r.w[e] : nw[e];
    }
  }
  const u32x2_t o = sgd_pack_shadow<u32x2_t>(nw);
  __builtin_nontemporal_store(nb, (f32x4_t*)((char*)sp.m + off));
  __builtin_nontemporal_store(nw, (f32x4_t*)((char*)sp.w + off));
  *(u32x2_t*)((char*)sp.s + (off >> 1)) = o;
}

// slabs [s0, s1), s0 < s1; slab s0 has been issued into stage 0 by pp_issue_first.  Every wave passes the same number of
// barriers (wave row 1 one extra in front, wave row 0 one extra behind).
// SGDP: the optimizer step of the previous tile rides along (above); VAR == 1.  s1 - s0 < 32: the chunks the loop has no
// slab for follow it, exposed.
template <int DT, int VAR, bool TN = false, bool SGDP = false, bool GUARD = false>
__device__ __forceinline__ void pp_mainloop(f32x16_t (&acc)[4][2], char* smem, __amdgpu_buffer_rsrc_t ra,
                                            __amdgpu_buffer_rsrc_t rb, const unsigned (&voa)[4], const unsigned (&vob)[4],
                                            int s0, int s1, int lane, int wave, unsigned bstep = 128,
                                            const SgdPipe* spp = nullptr) {
  SgdRegs srA, srB;  // chunk i is loaded into A (even slabs) / B (odd slabs) and applied one slab later
  const int wm = wave >> 2, wn = wave & 3;
  const int l31 = lane & 31, hi = lane >> 5, sw = (l31 >> 1) & 7;
  // LDS byte addresses of this lane's fragment of k-step ks inside the A0 / B0 half tile of the CURRENT stage; the other
  // half tiles are immediate offsets, the other stage one XOR per slab (in place: no second register set)
  unsigned oa[4], ob[4];
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    oa[ks] = lds0 + PP_A0 + (wm * 64 + l31) * 128 + (((ks * 2 + hi) ^ sw) << 4);
    const int tg = lane >> 4, tj = (lane >> 2) & 3, tc = lane & 3;  // TN: lane group, row of its [4][16] block, 8-byte piece
    ob[ks] = TN ? lds0 + PP_B0 + (ks * 4 + 2 * (tg >> 1)) * 1024 + tj * 256 + (((wn * 2 + (tg & 1)) ^ (2 * tj)) << 5) + tc * 8
                : lds0 + PP_B0 + (wn * 32 + l31) * 128 + (((ks * 2 + hi) ^ sw) << 4);
  }
  typedef __attribute__((address_space(3))) const i32x4_t* lds_v4;
  i32x4_t fa[2][4], fb[4];
  auto rdA = [&](int ks, int off) {
    fa[0][ks] = *(lds_v4)(uintptr_t)(oa[ks] + off);
    fa[1][ks] = *(lds_v4)(uintptr_t)(oa[ks] + off + 4096);
  };
  // TN: the transposing reads are INLINE ASM.  Through the builtin (__builtin_amdgcn_ds_read_tr16_b64_*) the compiler puts
  // `s_waitcnt vmcnt(0)` in front of every group of them - it orders the intrinsic behind ALL pending LDS-DMA, i.e. it
  // drains the half tiles that are meant to stay in flight across the phase (measured: the fc6 dW slab 194 us vs 178 us
  // for the NT form, SQ_WAIT_ANY 0.49 vs 0.36 of the wave cycles, same LDS array cycles and no bank conflicts -
  // profiles/r3_15_pmc_dw*.json).  The compiler therefore does not count them in lgkmcnt: a phase that reads only B
  // fragments waits for them itself (mm<true>: counted waits tied to the fragment registers), and phase 1 issues its B
  // reads FIRST - LDS returns in order, so the compiler's own waits for the A fragments behind them cover them.
  auto rdB = [&](int ks, int off) {
    if constexpr (TN) {
      typedef int i32x2_t __attribute__((ext_vector_type(2)));
      i32x2_t l2, h2;
      const unsigned addr = ob[ks] + off;
      asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(l2) : "v"(addr));
      asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(h2) : "v"(addr));
      fb[ks] = i32x4_t{l2[0], l2[1], h2[0], h2[1]};
    } else {
      fb[ks] = *(lds_v4)(uintptr_t)(ob[ks] + off);
    }
  };
  auto mm = [&](f32x16_t& c0, f32x16_t& c1, auto wait_b_tag) {
    constexpr bool WAIT_B = decltype(wait_b_tag)::value;  // TN, a phase whose only LDS reads are this phase's 8 tr reads
    if (VAR != 3) __builtin_amdgcn_s_setprio(1);
    // (the sched barriers keep each counted wait in front of ITS two MFMAs; left alone the scheduler hoists all four)
    if constexpr (TN && WAIT_B) asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(fb[0]));
    mma_step<DT>(c0, fb[0], fa[0][0]);  // swapped: D^T[n][m]
    mma_step<DT>(c1, fb[0], fa[1][0]);
    if constexpr (TN && WAIT_B) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(fb[1])); }
    mma_step<DT>(c0, fb[1], fa[0][1]);
    mma_step<DT>(c1, fb[1], fa[1][1]);
    if constexpr (TN && WAIT_B) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(fb[2])); }
    mma_step<DT>(c0, fb[2], fa[0][2]);
    mma_step<DT>(c1, fb[2], fa[1][2]);
    if constexpr (TN && WAIT_B) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fb[3])); }
    mma_step<DT>(c0, fb[3], fa[0][3]);
    mma_step<DT>(c1, fb[3], fa[1][3]);
    if (VAR != 3) __builtin_amdgcn_s_setprio(0);
  };
  constexpr std::false_type NOWAIT{};
  constexpr std::true_type WAITB{};
  // one 1-KB DMA piece: q = 0..7 in staging order A0.0 A0.1 B0.0 B0.1 B1.0 B1.1 A1.0 A1.1
  auto piece = [&](char* stage, auto qtag, int slab) {
    constexpr int q = decltype(qtag)::value;
    constexpr int which = q >> 1, pc = q & 1;
    constexpr int off = which == 0 ? PP_A0 : which == 1 ? PP_B0 : which == 2 ? PP_B1 : PP_A1;
    constexpr bool isA = which == 0 || which == 3;
    constexpr int h = (which == 2 || which == 3) ? 1 : 0;
    char* dst = stage + off + (pc * 64 + wave * 8) * 128;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(isA ? ra : rb, (__attribute__((address_space(3))) void*)dst, 16,
                                             isA ? voa[h * 2 + pc] : vob[h * 2 + pc], isA ? slab * 128 : slab * bstep, 0, 0);
  };
#define PP_PIECE(q) piece(nxt, std::integral_constant<int, q>{}, sn)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PP_BARRIER();
  if (wm == 1) PP_BARRIER();  // the lower wave row runs one barrier interval behind the upper one
  auto slab = [&](int s, SgdRegs& sr_ld, const SgdRegs& sr_use) __attribute__((always_inline)) {
    char* nxt = smem + (((s - s0) & 1) ^ 1) * PP_STAGE;
    const int sn = s + 1 < s1 ? s + 1 : s1 - 1;  // past the end: the last slab again, into a stage nobody reads
    // ---- phase 1: quadrant (a0, b0); reads in the order the MFMAs consume them (counted lgkmcnt waits)
    if constexpr (TN) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) rdB(ks, 0);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) rdA(ks, 0);
    } else {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) { rdB(ks, 0); rdA(ks, 0); }
    }
    if (VAR == 2) {  // rebalanced: the phase with 12 fragment reads issues no DMA (pieces 0 / 3 / 2 / 3 per phase)
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");  // B1 of this slab: A1's two pieces may stay in flight
    } else {
      PP_PIECE(0); PP_PIECE(1);
      if constexpr (SGDP) {
        const unsigned i_ = (unsigned)(s - s0);
        if (i_ < 32) {  // (32 chunks per tile; longer K loops - R > 2048 - carry nothing in their later slabs)
          sgdp_load(*spp, sr_ld, spp->off + i_ * spp->step, spp->goff + i_ * spp->gstep);
          asm volatile("s_waitcnt vmcnt(7)" ::: "memory");  // B1 of this slab (3 optimizer loads younger than the pieces)
        } else {
          asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        }
      } else {
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // B1 of this slab has landed (read in phase 2)
      }
    }
    PP_BARRIER();
    mm(acc[0][0], acc[1][0], NOWAIT);
    PP_BARRIER();
    // ---- phase 2: (a0, b1)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) rdB(ks, PP_B1 - PP_B0);
    if (VAR == 2) {
      PP_PIECE(0); PP_PIECE(1); PP_PIECE(2);
      asm volatile("s_waitcnt vmcnt(3)" ::: "memory");  // A1 of this slab (phase 3)
    } else {
      PP_PIECE(2); PP_PIECE(3);
      if constexpr (SGDP) {
        if ((unsigned)(s - s0) < 32) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");  // A1 of this slab; P0 P1 L L L P2 P3 may be in flight
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // A1 of this slab (phase 3)
    }
    PP_BARRIER();
    mm(acc[0][1], acc[1][1], WAITB);
    PP_BARRIER();
    // ---- phase 3: (a1, b1)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) rdA(ks, PP_A1 - PP_A0);
    if (VAR == 2) { PP_PIECE(3); PP_PIECE(4); } else { PP_PIECE(4); PP_PIECE(5); }
    if constexpr (SGDP) {
      const unsigned i_ = (unsigned)(s - s0);
      // chunk i - 1: its loads went out in phase 1 of the previous slab (18 vector memory operations ago; 15 in slab 1)
      if (i_ >= 1 && i_ <= 32) sgdp_apply_store<GUARD>(*spp, sr_use, spp->off + (i_ - 1) * spp->step);
    }
    PP_BARRIER();
    mm(acc[2][1], acc[3][1], NOWAIT);
    PP_BARRIER();
    // ---- phase 4: (a1, b0); b0 is read again (4 reads in a phase that has none) rather than kept: 16 registers, which
    // decide whether a trunk conv workgroup still fits beside this kernel (DESIGN 'trunk beside the GEMMs')
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) rdB(ks, 0);
    if (VAR == 2) { PP_PIECE(5); PP_PIECE(6); PP_PIECE(7); } else { PP_PIECE(6); PP_PIECE(7); }
    if constexpr (SGDP) {
      // A0 and B0 of the next slab; behind them P4 P5 [S S S] P6 P7 may be in flight (no stores yet in slab 0)
      if (s > s0 && s - s0 <= 32) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // A0 and B0 of the next slab (its phase 1)
    PP_BARRIER();
    mm(acc[2][0], acc[3][0], WAITB);
    PP_BARRIER();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { oa[ks] ^= PP_STAGE; ob[ks] ^= PP_STAGE; }
  };
  if constexpr (SGDP) {
    int s = s0;
    for (; s + 1 < s1; s += 2) {  // chunk i lives in A (even slabs) / B (odd slabs): static register sets
      slab(s, srA, srB);
      slab(s + 1, srB, srA);
    }
    if (s < s1) slab(s, srA, srB);  // (odd slab counts: R = 4000 is 63 slabs)
  } else {
    for (int s = s0; s < s1; ++s) slab(s, srA, srA);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the redundant tail fetches must land before LDS is reused
  if constexpr (SGDP) {
    // <= 32 slabs: the chunk loaded in phase 1 of the last slab is still due (set A after an even slab index, B after an odd
    // one).  FEWER than 32 slabs (fewer than 2048 proposals - real data): the loop carried one chunk per slab, chunks
    // S .. 31 of the previous tile are left - four in flight per trip here, exposed (the registers of the fragment pipeline
    // are dead at this point, the accumulators are not touched).
    const unsigned S = (unsigned)(s1 - s0);
    if (S <= 32) {
      if (S & 1) sgdp_apply_store<GUARD>(*spp, srA, spp->off + (S - 1) * spp->step);
      else sgdp_apply_store<GUARD>(*spp, srB, spp->off + (S - 1) * spp->step);
    }
    for (unsigned c = S; c < 32; c += 4) {
      SgdRegs q[4];
#pragma unroll
      for (unsigned j = 0; j < 4; ++j) {
        const unsigned cc = c + j < 32 ? c + j : 31;  // (clamped: a duplicate load, never applied)
        sgdp_load(*spp, q[j], spp->off + cc * spp->step, spp->goff + cc * spp->gstep);
      }
#pragma unroll
      for (unsigned j = 0; j < 4; ++j)
        if (c + j < 32) sgdp_apply_store<GUARD>(*spp, q[j], spp->off + (c + j) * spp->step);
    }
  }
  if (wm == 0) PP_BARRIER();
#undef PP_PIECE
}

}  // namespace
