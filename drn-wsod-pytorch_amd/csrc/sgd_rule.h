// The SGD update rule, defined once: torch.optim.SGD as built by detectron2/solver/build.py:93-137 on the gradient as SGD.step
// sees it:  d = clip(g * grad_scale);  d = d + wd * w  (wd != 0);  b = first ? d : momentum * m + d;  w' = w - lr * b;  shadow = bf16(w')
// sgd_kernel / sgd_block_kernel (optim.hip) and the fused fc6 dW + SGD launch (sgdp_apply_store, mfma_mainloop.h) run this code,
// which is what keeps them bit-identical.  Every piece turns FMA contraction off for itself: the header is included by units
// built with contraction on (gemm.hip) and off (optim.hip), and the oracle rounds after every operation.
#pragma once
#include "drn_common.h"

typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));

// CLIP (SOLVER.CLIP_GRADIENTS, detectron2/solver/build.py:19-90: each parameter = each segment on its own, on the gradient
// as SGD.step sees it = g * grad_scale): CLIP_NONE is the kernel's arithmetic as it was (the two clip arguments are passed,
// never read); CLIP_VALUE clamps to +-clip_value (torch.nn.utils.clip_grad_value_); CLIP_NORM scales by min(clip_value * (1 / (norm + 1e-6)), 1) with the segment's norm read from
// seg_norms (drn_grad_norms; torch.nn.utils.clip_grad_norm_ on one tensor).  NaNs pass through both as through torch.clamp.
enum { CLIP_NONE = 0, CLIP_VALUE = 1, CLIP_NORM = 2 };
template <int CLIP>
__device__ __forceinline__ float clip_coef(float clip_value, const float* seg_norms, int s) {
#pragma clang fp contract(off)
  if constexpr (CLIP == CLIP_NORM) {
    // torch forms `max_norm / (total_norm + 1e-6)` as reciprocal(total_norm + 1e-6) * max_norm (Tensor.__rtruediv__): two roundings,
    // restated as such - a true division differs in the last bit for a quarter of the norms
    const float coef = (1.f / (seg_norms[s] + 1e-6f)) * clip_value;
    return coef > 1.f ? 1.f : coef;
  }
  return 1.f;
}
template <int CLIP>
__device__ __forceinline__ float clip_grad(float d, float clip_value, float coef) {
#pragma clang fp contract(off)
  if constexpr (CLIP == CLIP_VALUE) return d > clip_value ? clip_value : (d < -clip_value ? -clip_value : d);
  if constexpr (CLIP == CLIP_NORM) return d * coef;
  return d;
}

// four bf16 gradients (8 bytes of a bucket) -> fp32
__device__ __forceinline__ f32x4_t sgd_unpack_bf16x4(u32x2_t x) {
  return f32x4_t{__builtin_bit_cast(float, x.x << 16), __builtin_bit_cast(float, x.x & 0xffff0000u),
                 __builtin_bit_cast(float, x.y << 16), __builtin_bit_cast(float, x.y & 0xffff0000u)};
}
// four new weights -> their 8 bytes of the bf16 shadow (RNE).  V2 = the two words as the caller stores them: uint2 (the kernels)
// and u32x2_t (the fused launch) hold the same bits but are scheduled differently, and each user keeps its instruction stream
template <class V2>
__device__ __forceinline__ V2 sgd_pack_shadow(f32x4_t nw) {
  V2 o;
  o.x = (uint32_t)f32_to_bf16(nw[0]) | ((uint32_t)f32_to_bf16(nw[1]) << 16);
  o.y = (uint32_t)f32_to_bf16(nw[2]) | ((uint32_t)f32_to_bf16(nw[3]) << 16);
  return o;
}

// The rule on one element.  d = the gradient after grad_scale and clipping; m is not used on a first step.
struct SgdNew { float b, w; };  // the new momentum and the new weight
__device__ __forceinline__ SgdNew sgd_rule(float w, float m, float d, float lr, float wd, float momentum, int first) {
#pragma clang fp contract(off)
  if (wd != 0.f) d = d + wd * w;
  const float b = first ? d : momentum * m + d;
  return {b, w - lr * b};
}

// The rule on the four parameters at arena element j (j and j - goff are multiples of 4; g is biased so that arena element
// j <-> g[j]): 16-byte accesses (8 for bf16), the momentum not read on a first step.  w / momentum / gradient are streamed
// once per step: non-temporal accesses keep them from evicting the GEMM operands (and the freshly written bf16 shadow, which
// the next fc6 forward reads) from L2 / Infinity Cache (+1.4 % step rate).
template <bool SHADOW, int GDT, int CLIP>
__device__ __forceinline__ void sgd_update4(float* __restrict__ w, float* __restrict__ mom,
                                            const typename ElemOf<GDT>::type* __restrict__ g, bf16_t* __restrict__ shadow,
                                            long j, const SgdSeg& sg, float momentum, int first_step, float grad_scale,
                                            float clip_value, float coef) {
#pragma clang fp contract(off)
  const f32x4_t pw = __builtin_nontemporal_load((const f32x4_t*)(w + j));
  f32x4_t gg;
  if constexpr (GDT == DRN_BF16) gg = sgd_unpack_bf16x4(__builtin_nontemporal_load((const u32x2_t*)(g + j)));
  else gg = __builtin_nontemporal_load((const f32x4_t*)(g + j));
  f32x4_t mm = {0.f, 0.f, 0.f, 0.f};
  if (!first_step) mm = __builtin_nontemporal_load((const f32x4_t*)(mom + j));
  f32x4_t nb, nw;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const SgdNew u = sgd_rule(pw[e], mm[e], clip_grad<CLIP>(gg[e] * grad_scale, clip_value, coef), sg.lr, sg.wd, momentum, first_step);
    nb[e] = u.b;
    nw[e] = u.w;
  }
  __builtin_nontemporal_store(nb, (f32x4_t*)(mom + j));
  __builtin_nontemporal_store(nw, (f32x4_t*)(w + j));
  if (SHADOW) *(uint2*)(shadow + j) = sgd_pack_shadow<uint2>(nw);
}
