// CSCROIHeads on the device (projects/WSL/wsl/modeling/roi_heads/roi_heads_csc.py + wsl/layers/csrc/csc/csc_cuda.cu):
//   drn_csc_cpg       image-gradient map of one class: max over the colour channels of |d score_c / d image|, divided by
//                     its maximum                                              roi_heads_csc.py:456-464
//   drn_csc_weights   threshold -> summed-area table -> per-ROI frame / context contrast -> normalisation to [-1, 1] ->
//                     blend with the image-level prediction (one class)      csc_cuda.cu:132-161, :184-350, :398-535
//   drn_csc_loss      the two weighted image-level BCE losses and d loss / d logits through the WSDDN score product,
//                     or (mode 1) d (sum_r score[r, c*]) / d logits, the seed of the image-gradient pass
//                                                                           fast_rcnn.py:887-931, roi_heads_csc.py:441-455
//   drn_csc_{seed,cpg,weights,loss}_batch   the same bodies per image / per (image, class) pair of an image batch
//                     (CSCROIHeads.enable_image_batches; the definition is this package's, include/drn_wsod.h)
//   drn_csc_stats     the table of the reference's `Statistic` log (third_party/cpg_stats.py), counted on the device
//                     (CSCROIHeads.enable_csc_stats)                         fast_rcnn.py:910-918
// The reference runs the table, the normalisation and the blend on the HOST (three device<->host copies per class and
// a cudaDeviceSynchronize); here everything stays on the stream.  Integer / index work (threshold, counts, rounded box
// corners) is bit-exact with oracle/csc_ops.c; this file builds with -ffp-contract=off, and `/` / sqrtf() are the
// correctly rounded ones (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; __fsqrt_rn is the NATIVE sqrt).
#include <float.h>

#include "drn_common.h"
#include "../../include/drn_wsod.h"

namespace {

constexpr int CSC_T = 1024;

// ---- image-gradient map -----------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void csc_absmax_kernel(const void* dimg, int cpad, int C, long npx, float* map,
                                                         unsigned* gmax) {
  using E = ElemOf<DT>;
  float best = 0.f;
  for (long px = (long)blockIdx.x * blockDim.x + threadIdx.x; px < npx; px += (long)gridDim.x * blockDim.x) {
    const typename E::type* p = (const typename E::type*)dimg + px * cpad;
    float m = fabsf(E::ld(p));
    for (int c = 1; c < C; ++c) m = fmaxf(m, fabsf(E::ld(p + c)));
    map[px] = m;
    best = fmaxf(best, m);
  }
  best = wave_max(best);
  if ((threadIdx.x & 63) == 0) atomicMax(gmax, __float_as_uint(best));  // non-negative floats order like their bits
}

__global__ __launch_bounds__(256) void csc_scale_kernel(float* map, long npx, const unsigned* gmax) {
  const float mx = __uint_as_float(*gmax);
  for (long px = (long)blockIdx.x * blockDim.x + threadIdx.x; px < npx; px += (long)gridDim.x * blockDim.x)
    map[px] = map[px] / mx;
}

// ---- thresholded summed-area table --------------------------------------------------------------------------------
// rows: one workgroup per row, every thread counts a contiguous run, block scan of the run counts, second sweep writes
// the running count.  columns: one thread per column.  Counts are integers < 2^24, so fp32 adds are exact in any order.
__device__ __forceinline__ void csc_rowscan_row(const float* src, float* dst, int W, float thr, int* sc) {
  const int tid = threadIdx.x;
  const int per = (W + 255) / 256, x0 = min(W, tid * per), x1 = min(W, x0 + per);
  int cnt = 0;
  for (int x = x0; x < x1; ++x) cnt += src[x] >= thr ? 1 : 0;
  sc[tid] = cnt;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = tid >= o ? sc[tid - o] : 0;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  int run = sc[tid] - cnt;
  for (int x = x0; x < x1; ++x) {
    run += src[x] >= thr ? 1 : 0;
    dst[x] = (float)run;
  }
}

__global__ __launch_bounds__(256) void csc_rowscan_kernel(const float* cpg, float* table, int W, float thr) {
  __shared__ int sc[256];
  const int y = blockIdx.x;
  csc_rowscan_row(cpg + (long)y * W, table + (long)y * W, W, thr, sc);
}

__global__ __launch_bounds__(256) void csc_colscan_kernel(float* table, int H, int W) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= W) return;
  float acc = 0.f;
  for (int y = 0; y < H; ++y) {
    acc += table[(long)y * W + x];
    table[(long)y * W + x] = acc;
  }
}

// ---- CSCPool + normalisation + blend (one class, one workgroup) ---------------------------------------------------
__device__ __forceinline__ float csc_box_sum(const float* t, int width, int hs, int ws, int he, int we) {
  const float a1 = t[(long)he * width + we];
  const float a2 = (ws - 1 >= 0) ? t[(long)he * width + (ws - 1)] : 0.f;
  const float a3 = (hs - 1 >= 0) ? t[(long)(hs - 1) * width + we] : 0.f;
  const float a4 = (hs - 1 >= 0 && ws - 1 >= 0) ? t[(long)(hs - 1) * width + (ws - 1)] : 0.f;
  return a1 - a2 - a3 + a4;
}

__device__ __forceinline__ int csc_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// csc_cuda.cu:184-350 (T = float; the expressions written with double literals there are double here)
__device__ float csc_pool_one(const float* table, int height_im, int width_im, const float* roi, int area_sqrt,
                              float context_scale) {
  int wstart = (int)roundf(roi[1]), hstart = (int)roundf(roi[2]), wend = (int)roundf(roi[3]), hend = (int)roundf(roi[4]);
  wstart = csc_clampi(wstart, 0, width_im - 1);
  hstart = csc_clampi(hstart, 0, height_im - 1);
  wend = csc_clampi(wend, 0, width_im - 1);
  hend = csc_clampi(hend, 0, height_im - 1);
  float width_roi = (float)(wend - wstart), height_roi = (float)(hend - hstart);
  float width_roi_inner = (float)(1.0 * width_roi / context_scale);
  float height_roi_inner = (float)(1.0 * height_roi / context_scale);
  float width_roi_outer = (float)(1.0 * width_roi * context_scale);
  float height_roi_outer = (float)(1.0 * height_roi * context_scale);
  const float wcenter = (float)(1.0 * (wend + wstart) / 2.0);
  const float hcenter = (float)(1.0 * (hend + hstart) / 2.0);
  const int wstart_inner = (int)round(wcenter - width_roi_inner / 2.0);
  const int hstart_inner = (int)round(hcenter - height_roi_inner / 2.0);
  const int wend_inner = (int)round(wcenter + width_roi_inner / 2.0);
  const int hend_inner = (int)round(hcenter + height_roi_inner / 2.0);
  const int wstart_outer = (int)round(fmax(wcenter - width_roi_outer / 2.0, 0.0));
  const int hstart_outer = (int)round(fmax(hcenter - height_roi_outer / 2.0, 0.0));
  const int wend_outer = (int)round(fmin(wcenter + width_roi_outer / 2.0, width_im - 1.0));
  const int hend_outer = (int)round(fmin(hcenter + height_roi_outer / 2.0, height_im - 1.0));
  width_roi = (float)(wend - wstart + 1);
  height_roi = (float)(hend - hstart + 1);
  width_roi_inner = (float)(wend_inner - wstart_inner + 1);
  height_roi_inner = (float)(hend_inner - hstart_inner + 1);
  width_roi_outer = (float)(wend_outer - wstart_outer + 1);
  height_roi_outer = (float)(hend_outer - hstart_outer + 1);
  const float sum_roi = csc_box_sum(table, width_im, hstart, wstart, hend, wend);
  const float sum_inner = csc_box_sum(table, width_im, hstart_inner, wstart_inner, hend_inner, wend_inner);
  const float sum_outer = csc_box_sum(table, width_im, hstart_outer, wstart_outer, hend_outer, wend_outer);
  const float area_roi = height_roi * width_roi;
  const float area_inner = height_roi_inner * width_roi_inner;
  const float area_outer = height_roi_outer * width_roi_outer;
  const float area_frame = fmaxf(area_roi - area_inner, 1.f);
  const float area_context = fmaxf(area_outer - area_roi, 1.f);
  const float sum_frame = sum_roi - sum_inner;
  const float sum_context = sum_outer - sum_roi;
  if (area_sqrt)
    return sum_frame / sqrtf(area_frame) - sum_context / sqrtf(area_context);
  return sum_frame / area_frame - sum_context / area_context;
}

// fixed-order block reduction of one value per thread (tree over LDS): same result on every run
template <int OP>  // 0 max, 1 min, 2 sum
__device__ __forceinline__ float csc_block_reduce(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = CSC_T / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const float a = red[tid], b = red[tid + o];
      red[tid] = OP == 0 ? fmaxf(a, b) : OP == 1 ? fminf(a, b) : a + b;
    }
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ void csc_pool_body(const float* table, int H, int W, const float* rois, int M,
                                              const float* scores, int K, int c, int area_sqrt, float context_scale,
                                              float* Wout, float* red) {
  const int tid = threadIdx.x;
  float vmax = 0.f, vmin = 0.f, ssum = 0.f;
  for (int r = tid; r < M; r += CSC_T) {
    const float v = csc_pool_one(table, H, W, rois + 5 * (long)r, area_sqrt, context_scale);
    Wout[(long)r * K + c] = v;
    vmax = fmaxf(vmax, v);
    vmin = fminf(vmin, v);
    ssum += scores[(long)r * K + c];
  }
  const float max_value = csc_block_reduce<0>(vmax, red);
  const float min_value = csc_block_reduce<1>(vmin, red);
  const float pred = csc_block_reduce<2>(ssum, red);  // torch.sum(pred_class_logits, dim=0)[c], unclamped
  for (int r = tid; r < M; r += CSC_T) {
    float v = Wout[(long)r * K + c];
    if (max_value > 0 && min_value < 0)
      v = v > 0 ? v / max_value : v / (-min_value);
    else if (max_value > 0 && min_value == 0)
      v = v / max_value;
    else
      v = 1.0f;
    const float a = pred * v, b = (1 - pred) * 1;
    Wout[(long)r * K + c] = a + b;
  }
}

__global__ __launch_bounds__(CSC_T) void csc_pool_kernel(const float* table, int H, int W, const float* rois, int M,
                                                         const float* scores, int K, int c, int area_sqrt,
                                                         float context_scale, float* Wout) {
  __shared__ float red[CSC_T];
  csc_pool_body(table, H, W, rois, M, scores, K, c, area_sqrt, context_scale, Wout, red);
}

// ---- losses / seeds through the WSDDN product s[r,c] = softmax_c(cls)[r,c] * softmax_r(det)[r,c] -------------------
struct CscLossParams {
  const float* logits; long ld; int c_cls, c_det, K, M;
  const float* scores; const float* rowsm; const float* W; const float* onehot;
  int mode, cstar, mean_loss;
  float* loss; float* dlogits; long ld_d;
};

// SCALE: `dscale` multiplies every dlogits entry once more (drn_csc_loss_batch: 1.f / n_img; its seed mode: 1.f, exact)
template <int LPR, bool SCALE>
__device__ __forceinline__ void csc_loss_body(const CscLossParams& p, float dscale,
                                              float (*red)[LPR * (LPR == 64 ? 2 : 1)]) {
  constexpr int RPP = CSC_T / LPR, CPL = LPR == 64 ? 2 : 1;
  const int l = threadIdx.x % LPR, ph = threadIdx.x / LPR, K = p.K, M = p.M;
  int col[CPL];
  bool ok[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) { col[j] = l + j * LPR; ok[j] = col[j] < K; }
  // column reduce over the row phases, fixed order; every thread of a column gets the result
  auto colreduce = [&](float (&v)[CPL], bool is_max) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CPL; ++j) red[ph][col[j]] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      float acc = is_max ? -FLT_MAX : 0.f;
      for (int q = 0; q < RPP; ++q) acc = is_max ? fmaxf(acc, red[q][col[j]]) : acc + red[q][col[j]];
      v[j] = acc;
    }
  };
  auto lanesum = [&](float v) {
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LPR);
    return v;
  };
  float cmax[CPL], csum[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) { cmax[j] = -FLT_MAX; csum[j] = 0.f; }
  for (int r = ph; r < M; r += RPP)
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (ok[j]) cmax[j] = fmaxf(cmax[j], p.logits[(long)r * p.ld + p.c_det + col[j]]);
  colreduce(cmax, true);
  for (int r = ph; r < M; r += RPP)
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (ok[j]) csum[j] += expf(p.logits[(long)r * p.ld + p.c_det + col[j]] - cmax[j]);
  colreduce(csum, false);
  float gp[CPL], gn[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) { gp[j] = 0.f; gn[j] = 0.f; }
  if (p.mode == 0) {
    float sp[CPL], sn[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) { sp[j] = 0.f; sn[j] = 0.f; }
    for (int r = ph; r < M; r += RPP)
#pragma unroll
      for (int j = 0; j < CPL; ++j)
        if (ok[j]) {
          const float s = p.scores[(long)r * K + col[j]], w = p.W ? p.W[(long)r * K + col[j]] : 1.f;
          sp[j] += s * fmaxf(w, 0.f);
          sn[j] += s * fmaxf(-w, 0.f);
        }
    colreduce(sp, false);
    colreduce(sn, false);
    const float norm = p.mean_loss ? 1.f / (float)K : 1.f;  // F.binary_cross_entropy reduction; / PL.size(0) = 1 image
    float lp = 0.f, ln = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      if (!ok[j]) continue;
      const float y = p.onehot[col[j]];
      // torch.clamp(x, 1e-20, 1.0 - 1e-20): the upper bound IS 1.0 in fp32; the gradient passes inside the closed range
      const float xp = fminf(fmaxf(sp[j], 1e-20f), 1.0f), xn = fminf(fmaxf(sn[j], 1e-20f), 1.0f);
      // F.binary_cross_entropy: -(y * max(log x, -100) + (1 - y) * max(log1p(-x), -100))
      lp += -(y * fmaxf(logf(xp), -100.f) + (1.f - y) * fmaxf(log1pf(-xp), -100.f));
      ln += -fmaxf(log1pf(-xn), -100.f);  // NL = 0
      // binary_cross_entropy backward: (x - y) / max((1 - x) * x, 1e-12)
      gp[j] = (sp[j] >= 1e-20f && sp[j] <= 1.0f) ? (xp - y) / fmaxf((1.f - xp) * xp, 1e-12f) * norm : 0.f;
      gn[j] = (sn[j] >= 1e-20f && sn[j] <= 1.0f) ? xn / fmaxf((1.f - xn) * xn, 1e-12f) * norm : 0.f;
    }
    lp = lanesum(lp);
    ln = lanesum(ln);
    if (threadIdx.x == 0) { p.loss[0] = lp * norm; p.loss[1] = ln * norm; }
  }
  if (!p.dlogits) return;
  auto gw = [&](int r, int j) -> float {  // d(objective) / d score[r, col[j]]
    if (p.mode == 1) return col[j] == p.cstar ? 1.f : 0.f;
    const float w = p.W ? p.W[(long)r * K + col[j]] : 1.f;
    return gp[j] * fmaxf(w, 0.f) + gn[j] * fmaxf(-w, 0.f);
  };
  float T[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) T[j] = 0.f;
  for (int r = ph; r < M; r += RPP)
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (ok[j]) T[j] += gw(r, j) * p.scores[(long)r * K + col[j]];
  colreduce(T, false);
  // d cls[r,j] = G[r,j] s[r,j] - a[r,j] * sum_k G[r,k] s[r,k];   d det[r,c] = G[r,c] s[r,c] - b[r,c] * T[c]
  for (int r = ph; r < M; r += RPP) {
    float gs[CPL], dot = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) { gs[j] = ok[j] ? gw(r, j) * p.scores[(long)r * K + col[j]] : 0.f; dot += gs[j]; }
    dot = lanesum(dot);
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (ok[j]) {
        const float b = expf(p.logits[(long)r * p.ld + p.c_det + col[j]] - cmax[j]) / csum[j];
        const float dc = gs[j] - p.rowsm[(long)r * K + col[j]] * dot, dd = gs[j] - b * T[j];
        p.dlogits[(long)r * p.ld_d + p.c_cls + col[j]] = SCALE ? dc * dscale : dc;
        p.dlogits[(long)r * p.ld_d + p.c_det + col[j]] = SCALE ? dd * dscale : dd;
      }
  }
}

template <int LPR>
__global__ __launch_bounds__(CSC_T) void csc_loss_kernel(CscLossParams p) {
  __shared__ float red[CSC_T / LPR][LPR * (LPR == 64 ? 2 : 1)];
  csc_loss_body<LPR, false>(p, 1.f, red);
}

// ---- image batches (CSCROIHeads.enable_image_batches; the definition is in include/drn_wsod.h) ----------------------
// Every kernel below runs the single-image body above on one image's rows / one image's crop, so its results are the
// single-image entry's bit for bit.  What the host cannot see (a row range, a size or a class read from device memory
// that is out of range) skips the image or the pair: nothing of it is written.
struct CscBatchLossParams {
  CscLossParams p;         // pointers of the whole batch, M = all rows; onehot [n_img][K]
  const int* img_off;      // [n_img + 1]
  const long* slot_cls;    // mode 1: class of each image in this slot, -1 = none
  float* loss_img;         // mode 0: [n_img][2]
  int n_img;
};

template <int LPR>
__global__ __launch_bounds__(CSC_T) void csc_loss_batch_kernel(CscBatchLossParams q) {
  __shared__ float red[CSC_T / LPR][LPR * (LPR == 64 ? 2 : 1)];
  const int i = blockIdx.x;
  CscLossParams p = q.p;
  const int o0 = q.img_off[i], o1 = q.img_off[i + 1], K = p.K;
  if (o0 < 0 || o1 > p.M || o1 <= o0) {
    if (p.mode == 0 && threadIdx.x < 2) q.loss_img[2 * i + threadIdx.x] = __int_as_float(0x7fc00000);  // NaN: the mean shows it
    return;
  }
  p.M = o1 - o0;
  p.logits += (long)o0 * p.ld;
  p.scores += (long)o0 * K;
  p.rowsm += (long)o0 * K;
  if (p.W) p.W += (long)o0 * K;
  if (p.dlogits) p.dlogits += (long)o0 * p.ld_d;
  float dscale = 1.f;
  if (p.mode == 1) {
    const long c = q.slot_cls[i];
    if (c < 0 || c >= K) {  // no class in this slot: the d/dx pass carries an exact zero for the image
      for (long e = threadIdx.x; e < (long)p.M * K; e += CSC_T) {
        const long r = e / K;
        const int k = (int)(e - r * K);
        p.dlogits[r * p.ld_d + p.c_cls + k] = 0.f;
        p.dlogits[r * p.ld_d + p.c_det + k] = 0.f;
      }
      return;
    }
    p.cstar = (int)c;
  } else {
    p.onehot += (long)i * K;
    p.loss = q.loss_img + 2 * i;
    dscale = 1.f / (float)q.n_img;
  }
  csc_loss_body<LPR, true>(p, dscale, red);
}

// loss[j] = (float)((sum over images i, ascending, of (double)loss_img[i][j]) / n): one thread per loss, fixed order
__global__ __launch_bounds__(64) void csc_batch_mean_kernel(const float* loss_img, float* loss, int n_img) {
  const int j = threadIdx.x;
  if (j >= 2) return;
  double acc = 0.0;
  for (int i = 0; i < n_img; ++i) acc += (double)loss_img[2 * i + j];
  loss[j] = (float)(acc / (double)n_img);
}

struct CscCpgBatchParams {
  const void* dimg;        // [n_img][Hmax][Wmax][cpad]
  int cpad, C, n_img, Hmax, Wmax, K;
  const long* hw;          // [n_img][2]
  const long* slot_cls;    // [n_img]
  const long* map_off;     // [n_img]: image i's [K][H_i][W_i] block of `maps`, in floats
  float* maps;
  unsigned* gmax;          // [n_img]
};

// the map of image i's slot class and its crop -> false: nothing to do for this image
__device__ __forceinline__ bool csc_cpg_image(const CscCpgBatchParams& q, int i, int& H, int& W, float*& map) {
  const long c = q.slot_cls[i];
  H = (int)q.hw[2 * i];
  W = (int)q.hw[2 * i + 1];
  if (c < 0 || c >= q.K || H < 1 || W < 1 || H > q.Hmax || W > q.Wmax) return false;
  map = q.maps + q.map_off[i] + c * (long)H * W;
  return true;
}

template <int DT>
__global__ __launch_bounds__(256) void csc_absmax_batch_kernel(CscCpgBatchParams q) {
  using E = ElemOf<DT>;
  const int i = blockIdx.y;
  int H, W;
  float* map;
  if (!csc_cpg_image(q, i, H, W, map)) return;
  const long npx = (long)H * W;
  const typename E::type* img = (const typename E::type*)q.dimg + (long)i * q.Hmax * q.Wmax * q.cpad;
  float best = 0.f;
  for (long px = (long)blockIdx.x * blockDim.x + threadIdx.x; px < npx; px += (long)gridDim.x * blockDim.x) {
    const long y = px / W, x = px - y * W;  // the crop: rows beyond H and columns beyond W of the padded tensor are never read
    const typename E::type* p = img + (y * q.Wmax + x) * q.cpad;
    float m = fabsf(E::ld(p));
    for (int c = 1; c < q.C; ++c) m = fmaxf(m, fabsf(E::ld(p + c)));
    map[px] = m;
    best = fmaxf(best, m);
  }
  best = wave_max(best);
  if ((threadIdx.x & 63) == 0) atomicMax(q.gmax + i, __float_as_uint(best));  // max is exact in any order
}

__global__ __launch_bounds__(256) void csc_scale_batch_kernel(CscCpgBatchParams q) {
  const int i = blockIdx.y;
  int H, W;
  float* map;
  if (!csc_cpg_image(q, i, H, W, map)) return;
  const long npx = (long)H * W;
  const float mx = __uint_as_float(q.gmax[i]);
  for (long px = (long)blockIdx.x * blockDim.x + threadIdx.x; px < npx; px += (long)gridDim.x * blockDim.x)
    map[px] = map[px] / mx;
}

struct CscPairParams {
  const float* maps; const long* map_off; const long* hw; const long* pairs; const long* tab_off;
  float* tables;
  int n_img, K, Hmax, Wmax, M;
  const int* img_off;
};

// pair p = (image, class) -> false: skipped
__device__ __forceinline__ bool csc_pair(const CscPairParams& q, int p, int& i, int& c, int& H, int& W) {
  const long li = q.pairs[2 * p], lc = q.pairs[2 * p + 1];
  if (li < 0 || li >= q.n_img || lc < 0 || lc >= q.K) return false;
  i = (int)li;
  c = (int)lc;
  H = (int)q.hw[2 * i];
  W = (int)q.hw[2 * i + 1];
  return H >= 1 && W >= 1 && H <= q.Hmax && W <= q.Wmax;
}

// grid (Hmax, pairs): one workgroup per (row, pair), the single-image row scan
__global__ __launch_bounds__(256) void csc_rowscan_batch_kernel(CscPairParams q, float thr) {
  __shared__ int sc[256];
  int i, c, H, W;
  if (!csc_pair(q, blockIdx.y, i, c, H, W)) return;
  const int y = blockIdx.x;
  if (y >= H) return;
  const float* map = q.maps + q.map_off[i] + (long)c * H * W;
  csc_rowscan_row(map + (long)y * W, q.tables + q.tab_off[blockIdx.y] + (long)y * W, W, thr, sc);
}

// grid (ceil(Wmax / 64), pairs): 64 columns x 16 row segments per workgroup.  Every thread sums its segment of its column,
// the 16 segment sums of a column are prefix-added through LDS, a second sweep writes the running count.  Integer counts
// < 2^24 in fp32: exact in any order, so the table is csc_colscan_kernel's.
__global__ __launch_bounds__(CSC_T) void csc_colscan_batch_kernel(CscPairParams q) {
  constexpr int SEG = CSC_T / 64;
  __shared__ float part[SEG][64];
  int i, c, H, W;
  if (!csc_pair(q, blockIdx.y, i, c, H, W)) return;
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6, x = blockIdx.x * 64 + lane;
  if (blockIdx.x * 64 >= W) return;  // (the whole workgroup: no barrier is left behind)
  float* t = q.tables + q.tab_off[blockIdx.y];
  const int per = (H + SEG - 1) / SEG, y0 = min(H, seg * per), y1 = min(H, y0 + per);
  float acc = 0.f;
  if (x < W)
    for (int y = y0; y < y1; ++y) acc += t[(long)y * W + x];
  part[seg][lane] = acc;
  __syncthreads();
  acc = 0.f;
  for (int s = 0; s < seg; ++s) acc += part[s][lane];
  if (x < W)
    for (int y = y0; y < y1; ++y) {
      acc += t[(long)y * W + x];
      t[(long)y * W + x] = acc;
    }
}

// grid (pairs): csc_pool_kernel on the rows of the pair's image, its boxes clamped to the image's own (H_i, W_i)
__global__ __launch_bounds__(CSC_T) void csc_pool_batch_kernel(CscPairParams q, const float* rois, const float* scores,
                                                               int area_sqrt, float context_scale, float* Wout) {
  __shared__ float red[CSC_T];
  int i, c, H, W;
  if (!csc_pair(q, blockIdx.x, i, c, H, W)) return;
  const int o0 = q.img_off[i], o1 = q.img_off[i + 1];
  if (o0 < 0 || o1 > q.M || o1 <= o0) return;
  csc_pool_body(q.tables + q.tab_off[blockIdx.x], H, W, rois + 5 * (long)o0, o1 - o0, scores + (long)o0 * q.K, q.K, c,
                area_sqrt, context_scale, Wout + (long)o0 * q.K, red);
}

// ---- weight statistics (CSCROIHeads.enable_csc_stats; "CSC weight statistics" in include/drn_wsod.h) ----------------------
// Two launches.  csc_stats_image_kernel: one workgroup per image; the image's rows of scores / W travel through LDS in tiles
// of whole rows (every global read runs along K, all 1024 threads load), and one thread per (column, quantity) walks the
// tile row by row - so each of the three sums of a column is ONE fp64 chain in ascending row order, whatever the tile or the
// grid is.
// It writes one record per (image, class): nothing is accumulated across images here.  csc_stats_fold_kernel: one workgroup,
// thread c folds the images' records of class c into the table in ascending image order (plain fp64 / int64 adds: the
// stream orders the launches, no atomics are needed).
constexpr int CSC_ST_TILE = 4096;  // floats of one LDS tile per tensor: >= 32 whole rows at K = 128
constexpr int CSC_ST_REC = 6;      // 8-byte words per (image, class) record: pred, pos, neg (fp64), #pos, #neg, #zero (int64)

__device__ __forceinline__ float csc_clampf(float v, float lo, float hi) {  // torch.clamp: a NaN stays a NaN
  return v < lo ? lo : (v > hi ? hi : v);
}

// part: per image 1 + CSC_ST_REC * K words; word 0 = R (0: the image's row range is invalid, nothing of it counts)
__global__ __launch_bounds__(CSC_T) void csc_stats_image_kernel(const float* scores, const float* W, const int* img_off,
                                                                int M, int K, long long* part) {
  __shared__ float ts[CSC_ST_TILE], tw[CSC_ST_TILE];
  const int i = blockIdx.x, tid = threadIdx.x;
  long long* rec = part + (long)i * (1 + CSC_ST_REC * K);
  const int o0 = img_off[i], o1 = img_off[i + 1];
  if (o0 < 0 || o1 > M || o1 <= o0) {  // (the whole workgroup: no barrier is left behind)
    if (tid == 0) rec[0] = 0;
    return;
  }
  // thread (what, c) = (tid / 128, tid % 128): the four quantities of a column - the score sum, the two weighted sums, the
  // sign counts - are four chains in four different waves, each of them ascending over the rows
  const int R = o1 - o0, rpt = CSC_ST_TILE / K, what = tid >> 7, c = tid & 127;
  const bool mine = what < 4 && c < K;
  double acc = 0.0;
  int npos = 0, nneg = 0;
  for (int r0 = 0; r0 < R; r0 += rpt) {
    const int nr = min(rpt, R - r0), n = nr * K;
    const long base = ((long)o0 + r0) * K;
    for (int e = tid; e < n; e += CSC_T) {
      ts[e] = scores[base + e];
      tw[e] = W[base + e];
    }
    __syncthreads();
    if (mine) {
      if (what == 0) {
#pragma unroll 8
        for (int r = 0; r < nr; ++r) acc += (double)ts[r * K + c];
      } else if (what == 1) {  // (the product of two floats is exact in fp64)
#pragma unroll 8
        for (int r = 0; r < nr; ++r) acc += (double)ts[r * K + c] * (double)fmaxf(tw[r * K + c], 0.f);
      } else if (what == 2) {
#pragma unroll 8
        for (int r = 0; r < nr; ++r) acc += (double)ts[r * K + c] * (double)fmaxf(-tw[r * K + c], 0.f);
      } else {
#pragma unroll 8
        for (int r = 0; r < nr; ++r) {
          const float w = tw[r * K + c];
          npos += w > 0.f ? 1 : 0;
          nneg += w < 0.f ? 1 : 0;  // -0.0 and NaN are neither: they count as zero weights
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) rec[0] = R;
  if (!mine) return;
  long long* q = rec + 1 + CSC_ST_REC * c;
  double* qd = (double*)q;
  if (what == 0) {
    qd[0] = (double)csc_clampf((float)acc, 1e-6f, (float)(1.0 - 1e-6));  // predict_probs_img, fast_rcnn.py:959-961
  } else if (what < 3) {
    qd[what] = (double)csc_clampf((float)acc, 1e-20f, 1.0f);             // csc_loss :900-908 (1.0 - 1e-20 IS 1.0 in fp32)
  } else {
    q[3] = npos;
    q[4] = nneg;
    q[5] = (long long)R - npos - nneg;
  }
}

// table: DRN_CSC_STATS_HEAD int64 words (steps, num_img), DRN_CSC_STATS_INT int64 fields [K], DRN_CSC_STATS_FP fp64 fields [K]
__global__ __launch_bounds__(128) void csc_stats_fold_kernel(const long long* part, const float* onehot, const long* slots,
                                                             int n_slots, int n_img, int K, long long* table) {
  __shared__ unsigned char act[DRN_CSC_MAX_IMAGES][128];
  const int c = threadIdx.x;
  for (int e = c; e < DRN_CSC_MAX_IMAGES * 128; e += 128) (&act[0][0])[e] = 0;
  __syncthreads();
  for (int e = c; e < n_slots * n_img; e += 128) {  // slot rows [n_slots][n_img]: the class image i builds a map for, or -1
    const long k = slots[e];
    if (k >= 0 && k < K) act[e % n_img][k] = 1;
  }
  __syncthreads();
  if (c == 0) {
    long long ni = 0;
    for (int i = 0; i < n_img; ++i) ni += part[(long)i * (1 + CSC_ST_REC * K)] > 0 ? 1 : 0;
    table[0] += 1;
    table[1] += ni;
  }
  if (c >= K) return;
  long long* ti = table + DRN_CSC_STATS_HEAD;
  double* tf = (double*)(table + DRN_CSC_STATS_HEAD + (long)DRN_CSC_STATS_INT * K);
  for (int i = 0; i < n_img; ++i) {  // ascending image order: every image is one UpdateIterStats call
    const long long* rec = part + (long)i * (1 + CSC_ST_REC * K);
    const long long R = rec[0];
    if (R <= 0 || !(onehot[(long)i * K + c] > 0.5f)) continue;  // cpg_stats.py:60
    const long long* q = rec + 1 + CSC_ST_REC * c;
    const double* qd = (const double*)q;
    ti[0 * K + c] += 1;      // ori_label
    ti[1 * K + c] += R;      // ori_num_roi
    tf[0 * K + c] += qd[0];  // ori_pred
    if (!act[i][c]) continue;
    ti[2 * K + c] += 1;      // csc_label
    ti[3 * K + c] += R;      // csc_num_roi
    ti[4 * K + c] += q[3];   // csc_roi_pos
    ti[5 * K + c] += q[4];   // csc_roi_neg
    ti[6 * K + c] += q[5];   // csc_roi_zero
    tf[1 * K + c] += qd[0];  // csc_pred
    tf[2 * K + c] += qd[1];  // csc_pred_pos
    tf[3 * K + c] += qd[2];  // csc_pred_neg
  }
}

}  // namespace

extern "C" {

// d score_c / d image (NHWC, `cpad` stored channels of which the first C are colours) -> cpg [H*W] fp32.
// scratch: one 32-bit word.  roi_heads_csc.py:456-464 (abs, max over dim 1, divide by the maximum).
int drn_csc_cpg(const void* dimg, int dtype, int cpad, int C, int H, int W, float* cpg, void* scratch, void* stream) {
  if (!dimg || !cpg || !scratch || C < 1 || C > cpad || H < 1 || W < 1) return DRN_ERR_ARG;
  if (dtype != DRN_F32 && dtype != DRN_BF16) return DRN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const long npx = (long)H * W;
  if (hipMemsetAsync(scratch, 0, 4, st) != hipSuccess) return DRN_ERR_LAUNCH;
  const int grid = (int)((npx + 255) / 256 < 2048 ? (npx + 255) / 256 : 2048);
  if (dtype == DRN_F32)
    hipLaunchKernelGGL((csc_absmax_kernel<DRN_F32>), dim3(grid), dim3(256), 0, st, dimg, cpad, C, npx, cpg, (unsigned*)scratch);
  else
    hipLaunchKernelGGL((csc_absmax_kernel<DRN_BF16>), dim3(grid), dim3(256), 0, st, dimg, cpad, C, npx, cpg, (unsigned*)scratch);
  hipLaunchKernelGGL(csc_scale_kernel, dim3(grid), dim3(256), 0, st, cpg, npx, (const unsigned*)scratch);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// one labelled class c: cpg [H*W] -> W[:, c] of W [M][K].  table: [H*W] floats of scratch.  scores [M][K] are the MIL
// scores (their column sum is the image-level prediction the weights are blended with).  csc_cuda.cu:398-535.
int drn_csc_weights(const float* cpg, int H, int W, float fg_threshold, const float* rois, int M, const float* scores,
                    int K, int c, int area_sqrt, float context_scale, float* table, float* Wout, void* stream) {
  if (!cpg || !rois || !scores || !table || !Wout || H < 1 || W < 1 || M < 1 || K < 1 || c < 0 || c >= K) return DRN_ERR_ARG;
  if ((long)H * W >= (1L << 24)) return DRN_ERR_UNSUPPORTED;  // fp32 counts stay exact below 2^24 pixels (as the reference's)
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(csc_rowscan_kernel, dim3(H), dim3(256), 0, st, cpg, table, W, 1.f * fg_threshold);
  hipLaunchKernelGGL(csc_colscan_kernel, dim3((W + 255) / 256), dim3(256), 0, st, table, H, W);
  hipLaunchKernelGGL(csc_pool_kernel, dim3(1), dim3(CSC_T), 0, st, (const float*)table, H, W, rois, M, scores, K, c,
                     area_sqrt, context_scale, Wout);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// mode 0: loss[0] = loss_cls_pos, loss[1] = loss_cls_neg (W may be null = all ones: past WSL.CSC_MAX_ITER) and
//         dlogits[:, cls | det columns] = d (loss_pos + loss_neg) / d logits
// mode 1: dlogits = d (sum_r score[r, cstar]) / d logits (loss untouched)
// One image (the reference head reads image_sizes[0] / gt_classes_img_oh[0]); K <= 128.
int drn_csc_loss(const float* logits, long ld, int c_cls, int c_det, int K, int M, const float* scores,
                 const float* row_softmax, const float* W, const float* onehot, int mode, int cstar, int mean_loss,
                 float* loss, float* dlogits, long ld_d, void* stream) {
  if (!logits || !scores || !row_softmax || K < 1 || K > 128 || M < 1 || (mode != 0 && mode != 1)) return DRN_ERR_ARG;
  if (mode == 0 && (!onehot || !loss)) return DRN_ERR_ARG;
  if (mode == 1 && (!dlogits || cstar < 0 || cstar >= K)) return DRN_ERR_ARG;
  CscLossParams p{logits, ld, c_cls, c_det, K, M, scores, row_softmax, W, onehot, mode, cstar, mean_loss, loss, dlogits, ld_d};
  hipStream_t st = (hipStream_t)stream;
  if (K <= 32)
    hipLaunchKernelGGL((csc_loss_kernel<32>), dim3(1), dim3(CSC_T), 0, st, p);
  else
    hipLaunchKernelGGL((csc_loss_kernel<64>), dim3(1), dim3(CSC_T), 0, st, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// ---- image batches: see "CSC on image batches" in include/drn_wsod.h ----
static int csc_batch_limits(int n_img, int K) {
  if (n_img < 1 || K < 1) return DRN_ERR_ARG;
  if (n_img > DRN_CSC_MAX_IMAGES || K > 128) return DRN_ERR_UNSUPPORTED;
  return DRN_OK;
}

int drn_csc_seed_batch(const float* logits, long ld, int c_cls, int c_det, int K, const float* scores,
                       const float* row_softmax, const int* img_off, int n_img, int M, const long* slot_cls,
                       float* dlogits, long ld_d, void* stream) {
  if (const int rc = csc_batch_limits(n_img, K)) return rc;
  if (!logits || !scores || !row_softmax || !img_off || !slot_cls || !dlogits || M < n_img) return DRN_ERR_ARG;
  CscBatchLossParams q{};
  q.p = CscLossParams{logits, ld, c_cls, c_det, K, M, scores, row_softmax, nullptr, nullptr, 1, 0, 0, nullptr, dlogits, ld_d};
  q.img_off = img_off; q.slot_cls = slot_cls; q.loss_img = nullptr; q.n_img = n_img;
  hipStream_t st = (hipStream_t)stream;
  if (K <= 32)
    hipLaunchKernelGGL((csc_loss_batch_kernel<32>), dim3(n_img), dim3(CSC_T), 0, st, q);
  else
    hipLaunchKernelGGL((csc_loss_batch_kernel<64>), dim3(n_img), dim3(CSC_T), 0, st, q);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_csc_cpg_batch(const void* dimg, int dtype, int cpad, int C, int n_img, int Hmax, int Wmax, const long* hw,
                      const long* slot_cls, int K, const long* map_off, float* maps, void* scratch, void* stream) {
  if (const int rc = csc_batch_limits(n_img, K)) return rc;
  if (!dimg || !hw || !slot_cls || !map_off || !maps || !scratch || C < 1 || C > cpad || Hmax < 1 || Wmax < 1) return DRN_ERR_ARG;
  if (dtype != DRN_F32 && dtype != DRN_BF16) return DRN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(scratch, 0, 4 * (size_t)n_img, st) != hipSuccess) return DRN_ERR_LAUNCH;
  const long npx = (long)Hmax * Wmax;
  const dim3 grid((unsigned)((npx + 255) / 256 < 2048 ? (npx + 255) / 256 : 2048), (unsigned)n_img);
  CscCpgBatchParams q{dimg, cpad, C, n_img, Hmax, Wmax, K, hw, slot_cls, map_off, maps, (unsigned*)scratch};
  if (dtype == DRN_F32)
    hipLaunchKernelGGL((csc_absmax_batch_kernel<DRN_F32>), grid, dim3(256), 0, st, q);
  else
    hipLaunchKernelGGL((csc_absmax_batch_kernel<DRN_BF16>), grid, dim3(256), 0, st, q);
  hipLaunchKernelGGL(csc_scale_batch_kernel, grid, dim3(256), 0, st, q);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_csc_weights_batch(const float* maps, const long* map_off, const long* hw, int n_img, int Hmax, int Wmax,
                          long max_px, const long* pairs, const long* tab_off, int n_pairs, float fg_threshold,
                          const float* rois, const int* img_off, int M, const float* scores, int K, int area_sqrt,
                          float context_scale, float* tables, float* Wout, void* stream) {
  if (const int rc = csc_batch_limits(n_img, K)) return rc;
  if (!maps || !map_off || !hw || !pairs || !tab_off || !rois || !img_off || !scores || !tables || !Wout || Hmax < 1 ||
      Wmax < 1 || max_px < 1 || max_px > (long)Hmax * Wmax || n_pairs < 0 || n_pairs > n_img * K || M < n_img)
    return DRN_ERR_ARG;
  if (max_px >= (1L << 24)) return DRN_ERR_UNSUPPORTED;  // fp32 counts stay exact below 2^24 pixels per image
  if (n_pairs == 0) return DRN_OK;
  hipStream_t st = (hipStream_t)stream;
  CscPairParams q{maps, map_off, hw, pairs, tab_off, tables, n_img, K, Hmax, Wmax, M, img_off};
  hipLaunchKernelGGL(csc_rowscan_batch_kernel, dim3(Hmax, n_pairs), dim3(256), 0, st, q, 1.f * fg_threshold);
  hipLaunchKernelGGL(csc_colscan_batch_kernel, dim3((Wmax + 63) / 64, n_pairs), dim3(CSC_T), 0, st, q);
  hipLaunchKernelGGL(csc_pool_batch_kernel, dim3(n_pairs), dim3(CSC_T), 0, st, q, rois, scores, area_sqrt, context_scale,
                     Wout);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_csc_loss_batch(const float* logits, long ld, int c_cls, int c_det, int K, const float* scores,
                       const float* row_softmax, const float* W, const float* onehot, const int* img_off, int n_img, int M,
                       int mean_loss, float* loss_img, float* loss, float* dlogits, long ld_d, void* stream) {
  if (const int rc = csc_batch_limits(n_img, K)) return rc;
  if (!logits || !scores || !row_softmax || !onehot || !img_off || !loss_img || !loss || M < n_img) return DRN_ERR_ARG;
  CscBatchLossParams q{};
  q.p = CscLossParams{logits, ld, c_cls, c_det, K, M, scores, row_softmax, W, onehot, 0, 0, mean_loss, nullptr, dlogits, ld_d};
  q.img_off = img_off; q.slot_cls = nullptr; q.loss_img = loss_img; q.n_img = n_img;
  hipStream_t st = (hipStream_t)stream;
  if (K <= 32)
    hipLaunchKernelGGL((csc_loss_batch_kernel<32>), dim3(n_img), dim3(CSC_T), 0, st, q);
  else
    hipLaunchKernelGGL((csc_loss_batch_kernel<64>), dim3(n_img), dim3(CSC_T), 0, st, q);
  hipLaunchKernelGGL(csc_batch_mean_kernel, dim3(1), dim3(64), 0, st, (const float*)loss_img, loss, n_img);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// ---- weight statistics: see "CSC weight statistics" in include/drn_wsod.h ----
int drn_csc_stats(const float* scores, const float* W, int K, const int* img_off, int n_img, int M, const float* onehot,
                  const long* slots, int n_slots, void* scratch, long* table, void* stream) {
  if (const int rc = csc_batch_limits(n_img, K)) return rc;
  if (!scores || !W || !img_off || !onehot || !scratch || !table || M < n_img || n_slots < 0 || n_slots > K ||
      (n_slots > 0 && !slots))
    return DRN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(csc_stats_image_kernel, dim3(n_img), dim3(CSC_T), 0, st, scores, W, img_off, M, K, (long long*)scratch);
  hipLaunchKernelGGL(csc_stats_fold_kernel, dim3(1), dim3(128), 0, st, (const long long*)scratch, onehot, slots, n_slots,
                     n_img, K, (long long*)table);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
