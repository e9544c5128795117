// Host-side plumbing over radix_sort.h shared by the evaluators (cocoeval.hip, voceval.hip): ping-pong sort buffers
// carved from a caller's workspace, one stable pass, "then by an integer key" passes, and the segment table of a sorted
// key array.  Each translation unit gets its own copy of the kernels.
#pragma once
#include "radix_sort.h"

namespace {

__global__ void set_int_kernel(int* p, int v) { p[0] = v; }

// key_out[j] = src[val[j]]: the next (integer) key of the elements in their current order.  Keys outside [0, nkeys) are
// the caller's error; they are clamped so that no segment table is indexed out of bounds.
__global__ void gather_key_kernel(const int* __restrict__ src, const int* __restrict__ val, unsigned* __restrict__ key_out,
                                  int n, int nkeys) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned k = (unsigned)src[val[j]];
  key_out[j] = k < (unsigned)nkeys ? k : (unsigned)(nkeys - 1);
}

// off[p] = first j with key[j] >= p, for p in [0, nseg]; key ascending, key[j] in [0, nseg)
__global__ void seg_bounds_kernel(const unsigned* __restrict__ key, int n, int nseg, int* __restrict__ off) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > n) return;
  const int prev = j == 0 ? -1 : (int)key[j - 1];
  int cur = j == n ? nseg : (int)key[j];
  if (cur > nseg) cur = nseg;
  for (int p = prev + 1; p <= cur; ++p) off[p] = j;
}

struct SortBufs {
  unsigned* key[2];
  int* val[2];
  int* hist;
  int* count;
  int tiles;
};

void sort_pass(const SortBufs& b, int from, const float* score, int shift, int bits, hipStream_t st) {
  SortPass sp{score, b.key[from], b.val[from], b.key[from ^ 1], b.val[from ^ 1], b.hist, b.count, b.tiles, shift, bits,
              score != nullptr};
  hipLaunchKernelGGL(sort_hist_kernel, dim3(b.tiles), dim3(SORT_THREADS), 0, st, sp);
  hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, st, sp);
  hipLaunchKernelGGL(sort_scatter_kernel, dim3(b.tiles), dim3(SORT_THREADS), 0, st, sp);
}

inline int key_bits(long nkeys) {
  int nbits = 1;
  while (nbits < 31 && (1L << nbits) < nkeys) ++nbits;
  return nbits;
}

// number of passes sort_int_passes runs for keys in [0, nkeys): known on the host, so is the buffer that holds the result
inline int int_passes(long nkeys) { return (key_bits(nkeys) + 10) / 11; }

// stable ascending by the integer keys already in b.key[cur], in [0, nkeys); returns the buffer that holds the result
int sort_int_passes(const SortBufs& b, int cur, int nkeys, hipStream_t st) {
  const int nbits = key_bits(nkeys);
  for (int shift = 0; shift < nbits; shift += 11) {
    const int bits = nbits - shift < 11 ? nbits - shift : 11;
    sort_pass(b, cur, nullptr, shift, bits, st);
    cur ^= 1;
  }
  return cur;
}

// then stable ascending by the integer key src[value], src[] in [0, nkeys); returns the buffer that holds the result
int sort_by_int(const SortBufs& b, int cur, const int* src, int nkeys, int n, hipStream_t st) {
  if (n > 0)
    hipLaunchKernelGGL(gather_key_kernel, dim3((n + 255) / 256), dim3(256), 0, st, src, b.val[cur], b.key[cur], n,
                       nkeys);
  return sort_int_passes(b, cur, nkeys, st);
}

inline int sort_tiles(int n) { return ((n < 1 ? 1 : n) + SORT_TILE - 1) / SORT_TILE; }

struct Carve {
  char* w;
  char* end;
  template <typename T>
  T* take(long count) {
    T* p = (T*)w;
    w += ((count * (long)sizeof(T) + 15) / 16) * 16;
    return p;
  }
};

SortBufs carve_sort(Carve& c, int n) {
  SortBufs b;
  const long m = n < 1 ? 1 : n;
  b.tiles = sort_tiles(n);
  b.key[0] = c.take<unsigned>(m);
  b.key[1] = c.take<unsigned>(m);
  b.val[0] = c.take<int>(m);
  b.val[1] = c.take<int>(m);
  b.hist = c.take<int>((long)SORT_BINS * b.tiles);
  b.count = c.take<int>(4);
  return b;
}

}  // namespace
