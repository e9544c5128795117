// The optimizer for gfx950 (HBM-bound, fp32 arithmetic, deterministic reductions: fixed-order trees, no float atomics).  Built
// with -ffp-contract=off; the update rule itself is sgd_rule.h, shared with the fused fc6 dW + SGD launch (mfma_mainloop.h).
//
// Replaces (reference file:line):
//   sgd_step           torch.optim.SGD as built by detectron2/solver/build.py:93-137
//   grad_norms, clip   SOLVER.CLIP_GRADIENTS, detectron2/solver/build.py:19-90
//   loss_guard         the finite-loss check of detectron2/engine/train_loop.py:252-258
#include "drn_common.h"
#include "sgd_rule.h"
#include "tune.h"

namespace {

// p -= lr * (buf = mom*buf + (g + wd*p)); first step: buf = g + wd*p, with CLIP on the gradient (sgd_rule.h).  One launch over the
// flat parameter arena (blockIdx.y walks the segments, float4 lanes when the segment offset is 16-B aligned); the bf16 compute
// shadow (same flat layout) is refreshed in the same pass, so the weights are read once per step.
// GUARD (the anomaly guard): guard -> state[0] of drn_loss_guard; non-zero = the step's loss was not finite, and the whole
// launch leaves w / mom / shadow as they are (a wave-uniform early exit: no load, no store).
template <bool SHADOW, int GDT, int CLIP, bool GUARD>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ w, float* __restrict__ mom,
                                                  const void* __restrict__ gv, long goff, bf16_t* __restrict__ shadow,
                                                  const SgdSeg* segs, int nseg, float momentum, int first_step,
                                                  float grad_scale, float clip_value, const float* seg_norms,
                                                  const int* guard) {
  if constexpr (GUARD) {
    if (guard[0] != 0) return;
  }
  using GT = typename ElemOf<GDT>::type;
  const GT* g = (const GT*)gv - goff;  // arena element j <-> g[j]
  for (int s = blockIdx.y; s < nseg; s += gridDim.y) {
    const SgdSeg sg = segs[s];
    const float coef = clip_coef<CLIP>(clip_value, seg_norms, s);
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
    long done = 0;
    if ((sg.off & 3) == 0 && ((sg.off - goff) & 3) == 0) {
      const long nvec = sg.cnt >> 2;
      for (long i = tid; i < nvec; i += nthr)
        sgd_update4<SHADOW, GDT, CLIP>(w, mom, g, shadow, sg.off + 4 * i, sg, momentum, first_step, grad_scale, clip_value, coef);
      done = nvec << 2;
    }
    for (long i = done + tid; i < sg.cnt; i += nthr) {
      const long j = sg.off + i;
      const float d = clip_grad<CLIP>(ElemOf<GDT>::ld(g + j) * grad_scale, clip_value, coef);
      const SgdNew u = sgd_rule(w[j], first_step ? 0.f : mom[j], d, sg.lr, sg.wd, momentum, first_step);
      mom[j] = u.b;
      w[j] = u.w;
      if (SHADOW) shadow[j] = f32_to_bf16(u.w);
    }
  }
}

// The same update on a rectangular BLOCK of one 2-D parameter (rows r0..r1, columns c0..c1 of a [.., ld] tensor that starts at
// arena element sg.off): the fc6 weight gradient leaves its GEMM in COLUMN slabs (one exact round of the persistent
// kernel each, run_fc1_tail), and each slab's update starts the moment its GEMM is queued.  Arithmetic, access width
// and cache policy are sgd_kernel's (sgd_update4); only the index map differs (a row of the block is a contiguous run of
// cols / 4 16-byte vectors).  c0, cols, ld, sg.off and goff are multiples of 4 (launcher).
template <bool SHADOW, int GDT, int CLIP, bool GUARD>
__global__ __launch_bounds__(256) void sgd_block_kernel(float* __restrict__ w, float* __restrict__ mom,
                                                        const void* __restrict__ gv, long goff, bf16_t* __restrict__ shadow,
                                                        const SgdSeg* seg, int r0, int rows, int c0, int cols, long ld,
                                                        float momentum, int first_step, float grad_scale, float clip_value,
                                                        const float* seg_norms, const int* guard) {
  if constexpr (GUARD) {
    if (guard[0] != 0) return;  // (as sgd_kernel)
  }
  using GT = typename ElemOf<GDT>::type;
  const GT* g = (const GT*)gv - goff;
  const SgdSeg sg = seg[0];
  const float coef = clip_coef<CLIP>(clip_value, seg_norms, 0);  // the norm of the ONE tensor seg[0] describes
  const unsigned cv = (unsigned)cols >> 2, nvec = (unsigned)rows * cv;
  const unsigned nthr = gridDim.x * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += nthr) {
    const unsigned r = i / cv, c = i - r * cv;
    const long j = sg.off + (long)(r0 + (int)r) * ld + c0 + 4 * (long)c;
    sgd_update4<SHADOW, GDT, CLIP>(w, mom, g, shadow, j, sg, momentum, first_step, grad_scale, clip_value, coef);
  }
}

// Per-segment gradient norms for CLIP_NORM (torch.nn.utils.clip_grad_norm_ on ONE tensor: ||g * grad_scale||_p, p = 1 / 2 / inf, in
// fp32).  HBM-bound (fc6.weight: 411 MB fp32 / 205 MB as the bf16 bucket), so every segment is spread over the whole x grid like
// sgd_kernel's; NO float atomics and a FIXED order of addition (set_deterministic rests on the RoI backward being the package's only
// float-atomic kernel): thread -> wave butterfly -> LDS tree over the 4 waves -> partial[s][blockIdx.x] in the caller's workspace
// (grad_norm_partial_kernel), then ONE workgroup per segment adds the NORM_GX partials in a fixed order and takes the root
// (grad_norm_final_kernel).  The x grid is a constant, not a tuning knob: the same input gives the same bits on every run.
constexpr int NORM_GX = 512;  // 2 workgroups per CU x 4 x 16-byte loads per thread in flight = 32 KiB of HBM reads per CU
enum { NORM_INF = 0, NORM_L1 = 1, NORM_L2 = 2 };

template <int P>
__device__ __forceinline__ float norm_term(float x, float grad_scale) {
  const float d = x * grad_scale;
  if constexpr (P == NORM_L2) return d * d;
  return fabsf(d);
}
// sum for p = 1 / 2; for inf a maximum that keeps a NaN (torch's abs().max() does)
template <int P>
__device__ __forceinline__ float norm_join(float a, float b) {
  if constexpr (P == NORM_INF) return (a >= b || a != a) ? a : b;
  return a + b;
}
template <int P>
__device__ __forceinline__ float norm_block_join(float v, float* lds4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = norm_join<P>(v, __shfl_xor(v, o, 64));
  __syncthreads();  // (lds4 is reused by the next segment of the caller's loop)
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return norm_join<P>(norm_join<P>(lds4[0], lds4[1]), norm_join<P>(lds4[2], lds4[3]));
}

template <int GDT, int P>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const void* __restrict__ gv, long goff, const SgdSeg* segs, int nseg,
                                                                float grad_scale, float* __restrict__ partial) {
  using GT = typename ElemOf<GDT>::type;
  constexpr int VE = 16 / (int)sizeof(GT);  // elements of one 16-byte load
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  __shared__ float lds4[4];
  const GT* g = (const GT*)gv - goff;  // arena element j <-> g[j]
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
  for (int s = blockIdx.y; s < nseg; s += gridDim.y) {
    const SgdSeg sg = segs[s];
    float acc[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) acc[e] = 0.f;
    auto add_vec = [&](const u32x4_t x) {
      if constexpr (GDT == DRN_BF16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[2 * e] = norm_join<P>(acc[2 * e], norm_term<P>(__builtin_bit_cast(float, x[e] << 16), grad_scale));
          acc[2 * e + 1] = norm_join<P>(acc[2 * e + 1], norm_term<P>(__builtin_bit_cast(float, x[e] & 0xffff0000u), grad_scale));
        }
      } else {
        const f32x4_t f = __builtin_bit_cast(f32x4_t, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = norm_join<P>(acc[e], norm_term<P>(f[e], grad_scale));
      }
    };
    long done = 0;
    if ((reinterpret_cast<uintptr_t>(g + sg.off) & 15) == 0) {
      const u32x4_t* g4 = (const u32x4_t*)(g + sg.off);
      const long nvec = sg.cnt / VE;
      long i = tid;
      for (; i + 3 * nthr < nvec; i += 4 * nthr) {  // four independent loads in flight, added in index order
        const u32x4_t x0 = __builtin_nontemporal_load(g4 + i), x1 = __builtin_nontemporal_load(g4 + i + nthr);
        const u32x4_t x2 = __builtin_nontemporal_load(g4 + i + 2 * nthr), x3 = __builtin_nontemporal_load(g4 + i + 3 * nthr);
        add_vec(x0); add_vec(x1); add_vec(x2); add_vec(x3);
      }
      for (; i < nvec; i += nthr) add_vec(__builtin_nontemporal_load(g4 + i));
      done = nvec * VE;
    }
    float v;
    if constexpr (VE == 8) {
      v = norm_join<P>(norm_join<P>(norm_join<P>(acc[0], acc[1]), norm_join<P>(acc[2], acc[3])),
                       norm_join<P>(norm_join<P>(acc[4], acc[5]), norm_join<P>(acc[6], acc[7])));
    } else {
      v = norm_join<P>(norm_join<P>(acc[0], acc[1]), norm_join<P>(acc[2], acc[3]));
    }
    for (long i = done + tid; i < sg.cnt; i += nthr) v = norm_join<P>(v, norm_term<P>(ElemOf<GDT>::ld(g + sg.off + i), grad_scale));
    v = norm_block_join<P>(v, lds4);
    if (threadIdx.x == 0) partial[(long)s * gridDim.x + blockIdx.x] = v;
  }
}

template <int P>
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const float* __restrict__ partial, int npart, float* __restrict__ norms) {
  __shared__ float lds4[4];
  const float* p = partial + (long)blockIdx.x * npart;
  float v = 0.f;
  for (int i = threadIdx.x; i < npart; i += 256) v = norm_join<P>(v, p[i]);
  v = norm_block_join<P>(v, lds4);
  if (threadIdx.x == 0) norms[blockIdx.x] = P == NORM_L2 ? sqrtf(v) : v;
}

// The anomaly guard's check (detectron2/engine/train_loop.py:252-258: `losses = sum(loss_dict.values())`, then
// `if not torch.isfinite(losses).all(): raise FloatingPointError`): one wave forms the fp32 sum of the step's loss scalars in
// list order and tests isfinite(sum) - +inf + -inf and an overflowing sum of finite terms are bad, as there.  The pointers
// travel in the kernel arguments (no device table to keep alive or to re-upload).  state[0] = skip flag (read by the guarded
// update kernels), [1] = calls seen, [2] = index of the first bad call or -1, [3] = bad calls; written by lane 0 alone.
enum { GUARD_RAISE = 1, GUARD_SKIP = 2, GUARD_MAX_LOSSES = 16 };
struct LossPtrs { const float* p[GUARD_MAX_LOSSES]; };
__global__ __launch_bounds__(64) void loss_guard_kernel(LossPtrs lp, int n, int mode, int window_first, int* state) {
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < GUARD_MAX_LOSSES; ++i)  // (unrolled: static indices into the argument block)
    if (i < n) sum = sum + lp.p[i][0];
  const bool bad = (__builtin_bit_cast(unsigned, sum) & 0x7f800000u) == 0x7f800000u;  // !isfinite: inf or NaN
  if (threadIdx.x == 0) {
    const int flag = state[0], calls = state[1], first_bad = state[2];
    // raise: sticky for ever.  skip: a bad micro-step discards its whole accumulation window and nothing more
    const bool keep = mode == GUARD_RAISE ? flag != 0 : (flag != 0 && !window_first);
    state[0] = (bad || keep) ? 1 : 0;
    state[1] = calls + 1;
    if (bad) {
      if (first_bad < 0) state[2] = calls;
      state[3] = state[3] + 1;
    }
  }
}

// What drn_sgd_step* and drn_sgd_step_block* require alike (every failure is DRN_ERR_ARG; segs = the device segment table).
bool sgd_args_ok(const float* weights, const float* momentum_buf, const void* grads, int grad_dtype, const void* shadow,
                 int shadow_dtype, const void* segs, int clip_mode, float clip_value, const float* seg_norms) {
  if (!weights || !momentum_buf || !grads || !segs) return false;
  if (shadow && shadow_dtype != DRN_BF16) return false;
  if (grad_dtype != DRN_F32 && grad_dtype != DRN_BF16) return false;
  if (clip_mode < CLIP_NONE || clip_mode > CLIP_NORM || (clip_mode == CLIP_NORM && !seg_norms)) return false;
  return clip_mode == CLIP_NONE || clip_value >= 0.f;  // (a NaN clip_value fails)
}

// The 24 instantiations of an update kernel, selected once: launch(shadow, grad dtype, clip mode, guard) receives each choice
// as a std::integral_constant, i.e. as a compile-time value.
template <int V> using int_c = std::integral_constant<int, V>;
template <class F>
void sgd_dispatch(bool shadow, int grad_dtype, int clip_mode, bool guard, F launch) {
  const auto pick = [](bool v, auto f) { if (v) f(std::true_type{}); else f(std::false_type{}); };
  pick(shadow, [&](auto sh) { pick(grad_dtype == DRN_BF16, [&](auto bf) { pick(guard, [&](auto gu) {
    const int_c<decltype(bf)::value ? DRN_BF16 : DRN_F32> gd;
    if (clip_mode == CLIP_VALUE) launch(sh, gd, int_c<CLIP_VALUE>{}, gu);
    else if (clip_mode == CLIP_NORM) launch(sh, gd, int_c<CLIP_NORM>{}, gu);
    else launch(sh, gd, int_c<CLIP_NONE>{}, gu);
  }); }); });
}

// g_tune.sgd_grid workgroups (x) of the optimizer kernel; each runs a grid-stride loop, i.e. lives for the whole launch.  At most two
// 256-thread workgroups (34 VGPRs) fit on a CU beside a resident 256x256 GEMM workgroup.
// segs_dev: device array of {int64 off, int64 cnt, float lr, float wd} (24 bytes each).  shadow (optional):
// bf16 array with the arena's flat layout, refreshed in the same pass.
int sgd_step_launch(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                    int shadow_dtype, const void* segs_dev, int nseg, float momentum, int first_step, float grad_scale,
                    int clip_mode, float clip_value, const float* seg_norms, const int* guard, void* stream) {
  if (nseg < 1 || !sgd_args_ok(weights, momentum_buf, grads, grad_dtype, shadow, shadow_dtype, segs_dev, clip_mode, clip_value,
                               seg_norms))
    return DRN_ERR_ARG;
  const dim3 grid(g_tune.sgd_grid, nseg < 32 ? nseg : 32), block(256);
  sgd_dispatch(shadow != nullptr, grad_dtype, clip_mode, guard != nullptr, [&](auto sh, auto gd, auto cl, auto gu) {
    hipLaunchKernelGGL((sgd_kernel<sh, gd, cl, gu>), grid, block, 0, (hipStream_t)stream, weights, momentum_buf, grads, grad_off,
                       (bf16_t*)shadow, (const SgdSeg*)segs_dev, nseg, momentum, first_step, grad_scale, clip_value, seg_norms, guard);
  });
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// drn_sgd_step on a rectangular block of ONE 2-D tensor: seg_dev = that tensor's {offset, count, lr, wd} entry (lr / wd are
// read on the device: a captured launch follows the schedule), the block = rows r0 .. r0+rows, columns c0 .. c0+cols of
// its [count / ld][ld] view.
int sgd_step_block_launch(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                          int shadow_dtype, const void* seg_dev, int r0, int rows, int c0, int cols, long ld, float momentum,
                          int first_step, float grad_scale, int clip_mode, float clip_value, const float* seg_norms,
                          const int* guard, void* stream) {
  if (r0 < 0 || rows < 0 || c0 < 0 || cols < 0 || ld < c0 + cols ||
      !sgd_args_ok(weights, momentum_buf, grads, grad_dtype, shadow, shadow_dtype, seg_dev, clip_mode, clip_value, seg_norms))
    return DRN_ERR_ARG;
  if ((c0 & 3) || (cols & 3) || (ld & 3) || (grad_off & 3)) return DRN_ERR_UNSUPPORTED;  // (the tensor's offset: checked by the caller's table)
  if ((long)rows * (cols >> 2) >= (1L << 32)) return DRN_ERR_UNSUPPORTED;
  if (rows == 0 || cols == 0) return DRN_OK;
  const dim3 grid(g_tune.sgd_grid), block(256);
  sgd_dispatch(shadow != nullptr, grad_dtype, clip_mode, guard != nullptr, [&](auto sh, auto gd, auto cl, auto gu) {
    hipLaunchKernelGGL((sgd_block_kernel<sh, gd, cl, gu>), grid, block, 0, (hipStream_t)stream, weights, momentum_buf, grads,
                       grad_off, (bf16_t*)shadow, (const SgdSeg*)seg_dev, r0, rows, c0, cols, ld, momentum, first_step, grad_scale,
                       clip_value, seg_norms, guard);
  });
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // namespace

extern "C" {

int drn_sgd_step(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                 int shadow_dtype, const void* segs_dev, int nseg, float momentum, int first_step, float grad_scale,
                 void* stream) {
  return sgd_step_launch(weights, momentum_buf, grads, grad_dtype, grad_off, shadow, shadow_dtype, segs_dev, nseg, momentum,
                         first_step, grad_scale, CLIP_NONE, 0.f, nullptr, nullptr, stream);
}

// drn_sgd_step with SOLVER.CLIP_GRADIENTS applied to g * grad_scale, per segment (sgd_kernel's CLIP parameter): clip_mode 0 = none
// (drn_sgd_step's bits), 1 = value, 2 = norm with seg_norms[nseg] from drn_grad_norms (device memory, read by the kernel)
int drn_sgd_step_clip(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                      int shadow_dtype, const void* segs_dev, int nseg, float momentum, int first_step, float grad_scale,
                      int clip_mode, float clip_value, const float* seg_norms, void* stream) {
  return sgd_step_launch(weights, momentum_buf, grads, grad_dtype, grad_off, shadow, shadow_dtype, segs_dev, nseg, momentum,
                         first_step, grad_scale, clip_mode, clip_value, seg_norms, nullptr, stream);
}

// drn_sgd_step_clip under the anomaly guard: guard -> state[0] of drn_loss_guard (device memory).  guard[0] == 0:
// drn_sgd_step_clip's bits; guard[0] != 0: weights, momentum_buf and shadow keep their bits.  A skipped FIRST step leaves
// momentum_buf untouched - the caller creates it as zeros, and a later first_step = 0 update on zeros computes what a first step would.
int drn_sgd_step_guard(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                       int shadow_dtype, const void* segs_dev, int nseg, float momentum, int first_step, float grad_scale,
                       int clip_mode, float clip_value, const float* seg_norms, const int* guard, void* stream) {
  if (!guard) return DRN_ERR_ARG;
  return sgd_step_launch(weights, momentum_buf, grads, grad_dtype, grad_off, shadow, shadow_dtype, segs_dev, nseg, momentum,
                         first_step, grad_scale, clip_mode, clip_value, seg_norms, guard, stream);
}

int drn_sgd_step_block(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                       int shadow_dtype, const void* seg_dev, int r0, int rows, int c0, int cols, long ld, float momentum,
                       int first_step, float grad_scale, void* stream) {
  return sgd_step_block_launch(weights, momentum_buf, grads, grad_dtype, grad_off, shadow, shadow_dtype, seg_dev, r0, rows, c0,
                               cols, ld, momentum, first_step, grad_scale, CLIP_NONE, 0.f, nullptr, nullptr, stream);
}

// drn_sgd_step_block with the clipping of drn_sgd_step_clip; seg_norms -> the norm of the ONE tensor seg_dev describes
int drn_sgd_step_block_clip(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                            int shadow_dtype, const void* seg_dev, int r0, int rows, int c0, int cols, long ld, float momentum,
                            int first_step, float grad_scale, int clip_mode, float clip_value, const float* seg_norms,
                            void* stream) {
  return sgd_step_block_launch(weights, momentum_buf, grads, grad_dtype, grad_off, shadow, shadow_dtype, seg_dev, r0, rows, c0,
                               cols, ld, momentum, first_step, grad_scale, clip_mode, clip_value, seg_norms, nullptr, stream);
}

// drn_sgd_step_block_clip under the anomaly guard (as drn_sgd_step_guard)
int drn_sgd_step_block_guard(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                             int shadow_dtype, const void* seg_dev, int r0, int rows, int c0, int cols, long ld, float momentum,
                             int first_step, float grad_scale, int clip_mode, float clip_value, const float* seg_norms,
                             const int* guard, void* stream) {
  if (!guard) return DRN_ERR_ARG;
  return sgd_step_block_launch(weights, momentum_buf, grads, grad_dtype, grad_off, shadow, shadow_dtype, seg_dev, r0, rows, c0,
                               cols, ld, momentum, first_step, grad_scale, clip_mode, clip_value, seg_norms, guard, stream);
}

// workspace of drn_grad_norms: one fp32 partial per (segment, x workgroup).  Host-only.
long drn_grad_norms_ws_bytes(int nseg) { return nseg < 1 ? 0 : (long)nseg * NORM_GX * (long)sizeof(float); }

// norms[s] = || grads[segment s] * grad_scale ||_p (norm_type 1, 2, or 0 = inf), grads read as drn_sgd_step reads them: two
// launches, no host synchronisation (capturable), no atomics
int drn_grad_norms(const void* grads, int grad_dtype, long grad_off, const void* segs_dev, int nseg, int norm_type,
                   float grad_scale, float* norms, void* workspace, long workspace_bytes, void* stream) {
  if (!grads || !segs_dev || !norms || !workspace || nseg < 1) return DRN_ERR_ARG;
  if (grad_dtype != DRN_F32 && grad_dtype != DRN_BF16) return DRN_ERR_ARG;
  if (norm_type != NORM_L1 && norm_type != NORM_L2 && norm_type != NORM_INF) return DRN_ERR_UNSUPPORTED;
  if (workspace_bytes < drn_grad_norms_ws_bytes(nseg)) return DRN_ERR_ARG;
  dim3 grid(NORM_GX, nseg < 32 ? nseg : 32), block(256);
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  const auto launch = [&](auto gd, auto p) {
    hipLaunchKernelGGL((grad_norm_partial_kernel<gd, p>), grid, block, 0, st, grads, grad_off, (const SgdSeg*)segs_dev, nseg,
                       grad_scale, partial);
    hipLaunchKernelGGL((grad_norm_final_kernel<p>), dim3(nseg), block, 0, st, (const float*)partial, NORM_GX, norms);
  };
  const auto by_norm = [&](auto gd) {
    if (norm_type == NORM_L1) launch(gd, int_c<NORM_L1>{});
    else if (norm_type == NORM_L2) launch(gd, int_c<NORM_L2>{});
    else launch(gd, int_c<NORM_INF>{});
  };
  if (grad_dtype == DRN_BF16) by_norm(int_c<DRN_BF16>{}); else by_norm(int_c<DRN_F32>{});
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// The device-side anomaly guard: losses = HOST array of n <= 16 device pointers to the step's fp32 loss scalars (copied into the
// launch's arguments); mode 1 = raise (the flag is sticky), 2 = skip (flag = bad_now || (flag && !window_first)); state =
// int32[4] in device memory, initialised by the caller to {0, 0, -1, 0}.  One launch of one wave; no sync, no allocation.
int drn_loss_guard(const void* const* losses, int n, int mode, int window_first, int* state, void* stream) {
  if (!losses || !state || n < 1 || n > GUARD_MAX_LOSSES || (mode != GUARD_RAISE && mode != GUARD_SKIP)) return DRN_ERR_ARG;
  LossPtrs lp;
  for (int i = 0; i < GUARD_MAX_LOSSES; ++i) {
    lp.p[i] = (const float*)losses[i < n ? i : 0];
    if (!lp.p[i]) return DRN_ERR_ARG;
  }
  hipLaunchKernelGGL(loss_guard_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, lp, n, mode, window_first ? 1 : 0, state);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
