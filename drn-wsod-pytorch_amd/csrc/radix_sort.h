// Stable LSD radix-sort passes shared by detect.hip (candidates by descending score) and cocoeval.hip (detections by
// score, then by integer keys: (image, category) pair or category).  Every pass is stable, so successive passes over
// different keys give the composite order.  Each translation unit gets its own copy of the kernels.
#pragma once
#include "drn_common.h"

namespace {

// ---- stable descending sort of the candidates by score (round 3: own kernels, replaces hipcub::DeviceRadixSort) ------
// torchvision's nms orders candidates with scores.sort(stable, descending); the value sorted along is the candidate's
// index, so "stable descending" = ascending on the key ~asc(score) with ties in index order - exactly what an LSD radix
// sort with stable passes delivers.  Three passes of 11 / 11 / 10 bits over the n = count[0] live candidates (the
// count stays on the device: grids are sized for `cap`, tiles beyond n retire at once):
//   sort_hist_kernel    per-tile digit histogram (LDS atomics: counts are order-free)      -> hist[digit][tile]
//   sort_scan_kernel    one workgroup: exclusive prefix over (digit-major, tile-minor)     -> hist becomes offsets
//   sort_scatter_kernel per tile, 256 elements per round IN INDEX ORDER: a lane's rank among equal digits = equal
//                       digits of earlier rounds (run[d]) + of earlier waves this round (cnt[w][d]) + of earlier lanes of
//                       its wave (ballot match over the digit's bits) - no atomics decide an order, so every pass is
//                       stable and the result is a function of the input alone
constexpr int SORT_THREADS = 256, SORT_ROUNDS = 16, SORT_TILE = SORT_THREADS * SORT_ROUNDS, SORT_BINS = 2048;

__device__ __forceinline__ unsigned sort_key_desc(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  const unsigned asc = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);  // ascending total order on the bits
  return ~asc;
}

struct SortPass {
  const float* score;      // pass 0: keys are derived from the scores and the value is the index itself
  const unsigned* key_in; const int* val_in;
  unsigned* key_out; int* val_out;
  int* hist;               // [SORT_BINS][tiles]
  const int* count;
  int tiles, shift, bits, first;
};

__device__ __forceinline__ unsigned sort_load_key(const SortPass& p, int i) {
  return p.first ? sort_key_desc(p.score[i]) : p.key_in[i];
}

__global__ __launch_bounds__(SORT_THREADS) void sort_hist_kernel(SortPass p) {
  __shared__ int h[SORT_BINS];
  const int n = p.count[0], tile = blockIdx.x, nb = 1 << p.bits;
  for (int d = threadIdx.x; d < nb; d += SORT_THREADS) h[d] = 0;
  __syncthreads();
  const int t0 = tile * SORT_TILE;
  if (t0 < n)
    for (int j = 0; j < SORT_ROUNDS; ++j) {
      const int i = t0 + j * SORT_THREADS + threadIdx.x;
      if (i < n) atomicAdd(&h[(sort_load_key(p, i) >> p.shift) & (nb - 1)], 1);
    }
  __syncthreads();
  for (int d = threadIdx.x; d < nb; d += SORT_THREADS) p.hist[(long)d * p.tiles + tile] = h[d];
}

// exclusive prefix of hist in (digit, tile) order; one workgroup of 1024 threads, two digits per thread at most
__global__ __launch_bounds__(1024) void sort_scan_kernel(SortPass p) {
  __shared__ int tot[SORT_BINS];
  __shared__ int wsum[16];
  const int nb = 1 << p.bits;
  for (int d = threadIdx.x; d < SORT_BINS; d += 1024) {
    int s = 0;
    if (d < nb)
      for (int t = 0; t < p.tiles; ++t) s += p.hist[(long)d * p.tiles + t];
    tot[d] = s;
  }
  __syncthreads();
  // block-wide exclusive scan of tot[0 .. 2048): thread t owns digits 2t, 2t+1
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int a = tot[2 * threadIdx.x], b = tot[2 * threadIdx.x + 1];
  int v = a + b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  if (lane == 63) wsum[w] = v;
  __syncthreads();
  int base = 0;
  for (int q = 0; q < w; ++q) base += wsum[q];
  const int excl = base + v - (a + b);
  __syncthreads();
  tot[2 * threadIdx.x] = excl;
  tot[2 * threadIdx.x + 1] = excl + a;
  __syncthreads();
  for (int d = threadIdx.x; d < nb; d += 1024) {
    int run = tot[d];
    for (int t = 0; t < p.tiles; ++t) {
      const long k = (long)d * p.tiles + t;
      const int c = p.hist[k];
      p.hist[k] = run;
      run += c;
    }
  }
}

__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(SortPass p) {
  __shared__ int run[SORT_BINS];                     // this tile's next output slot per digit
  __shared__ int cnt[SORT_THREADS / 64][SORT_BINS];  // per wave and round; every entry is reset by whoever set it
  const int n = p.count[0], tile = blockIdx.x, nb = 1 << p.bits;
  const int t0 = tile * SORT_TILE;
  if (t0 >= n) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int d = threadIdx.x; d < nb; d += SORT_THREADS) {
    run[d] = p.hist[(long)d * p.tiles + tile];
#pragma unroll
    for (int q = 0; q < SORT_THREADS / 64; ++q) cnt[q][d] = 0;
  }
  __syncthreads();
  for (int j = 0; j < SORT_ROUNDS; ++j) {
    const int i = t0 + j * SORT_THREADS + threadIdx.x;
    const bool valid = i < n;
    unsigned key = 0;
    int val = 0, d = 0;
    if (valid) {
      key = sort_load_key(p, i);
      val = p.first ? i : p.val_in[i];
      d = (key >> p.shift) & (nb - 1);
    }
    // lanes of this wave with the same digit (and valid)
    unsigned long long m = __ballot(valid);
    for (int b = 0; b < p.bits; ++b) {
      const unsigned long long bal = __ballot((d >> b) & 1);
      m &= ((d >> b) & 1) ? bal : ~bal;
    }
    const int lrank = __popcll(m & ((1ULL << lane) - 1ULL));
    const bool leader = valid && lrank == 0;
    if (leader) cnt[w][d] = __popcll(m);
    __syncthreads();
    if (valid) {
      int pos = run[d] + lrank;
      for (int q = 0; q < w; ++q) pos += cnt[q][d];
      p.key_out[pos] = key;
      p.val_out[pos] = val;
    }
    __syncthreads();
    if (leader) {
      atomicAdd(&run[d], cnt[w][d]);  // integer adds commute: run[d] is the same whatever order the waves arrive in
      cnt[w][d] = 0;
    }
    __syncthreads();
  }
}

}  // namespace
