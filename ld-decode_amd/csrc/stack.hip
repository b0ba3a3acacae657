// Disc stacking: several decodes of one disc merged into one .tbc, pixel by pixel from the
// sources that had no dropout there.  BUILD-DEFINED (tests/stack_ref.py
// is the numpy restatement): the snapshot this project follows has no stacker.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "field_rec.hpp"

namespace ldg {

constexpr int STACK_MAX_SRC = LDG_STACK_MAX_SOURCES;
constexpr int STACK_RUNS_STRIDE = MAX_LINES * LDG_MAX_DROPOUTS_PER_LINE * 2;   // int16 per (frame, source, parity)
constexpr int STACK_SENT = 0x3fffffff;      // the key of a source that is no candidate: sorts last
constexpr int STACK_THREADS = 128;

// compare-exchange network of Batcher's odd-even merge sort over n keys (any n); every
// index is a compile-time constant once the loops are unrolled, so v stays in registers
template <int N>
__device__ __forceinline__ void stack_sort(int (&v)[N]) {
#pragma unroll
  for (int p = 1; p < N; p <<= 1) {
#pragma unroll
    for (int k = p; k >= 1; k >>= 1) {
#pragma unroll
      for (int j = k % p; j <= N - 1 - k; j += 2 * k) {
#pragma unroll
        for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); i++) {
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            const int a = v[i + j], b = v[i + j + k];
            v[i + j] = a < b ? a : b;
            v[i + j + k] = a < b ? b : a;
          }
        }
      }
    }
  }
}

// v[idx] of an ascending v without a dynamic register index: the largest of v[0..idx]
template <int N>
__device__ __forceinline__ int stack_sel(const int (&v)[N], int idx) {
  int r = v[0];
#pragma unroll
  for (int k = 1; k < N; k++) {
    const int c = k <= idx ? v[k] : 0;
    r = c > r ? c : r;
  }
  return r;
}

// (num + d / 2) / d for 0 <= num < 2^21, 1 <= d <= 16: a float quotient (exact operands, a
// relative error of a few 2^-24, so off by one at the most) and one correction step
__device__ __forceinline__ int stack_div_round(int num, int d) {
  num += d >> 1;
  int q = (int)((float)num * __frcp_rn((float)d));
  const int r = num - q * d;
  q += r >= d ? 1 : 0;
  q -= r < 0 ? 1 : 0;
  return q;
}

// one output pixel: val[s] the sources' pixels, cand the candidates (bit s; never 0)
template <int N>
__device__ __forceinline__ int stack_pixel(const int (&val)[N], uint32_t cand, int mode, int T) {
  int key[N];
  int sum = 0;
#pragma unroll
  for (int s = 0; s < N; s++) {
    const bool c = (cand >> s) & 1u;
    key[s] = c ? val[s] : STACK_SENT;
    sum += c ? val[s] : 0;
  }
  const int m = __popc(cand);
  if (mode == LDG_STACK_MEAN) return stack_div_round(sum, m);
  stack_sort<N>(key);
  const int med = (stack_sel<N>(key, (m - 1) >> 1) + stack_sel<N>(key, m >> 1) + 1) >> 1;
  if (mode == LDG_STACK_MEDIAN) return med;
  int ks = 0, kc = 0;
#pragma unroll
  for (int k = 0; k < N; k++) {
    // |key - med| <= T; a sentinel is far outside
    const bool in = (uint32_t)(key[k] - med + T) <= (uint32_t)(2 * T);
    ks += in ? key[k] : 0;
    kc += in ? 1 : 0;
  }
  return kc ? stack_div_round(ks, kc) : med;
}

struct StackArgs {
  const uint16_t* src;     // [n_src] sources, src_stride pixels apart; each [n_frames][H][W] packed
  int64_t src_stride;      // a multiple of 8 pixels: every source shares out's 16-byte phase
  const uint32_t* rowinfo; // [n_frames][H]: bits 0..15 the sources present for the frame, bit 31: one of them has
                           // a run in this row (made by the host from present and counts: one scalar load a row)
  const int16_t* runs;     // [n_frames][n_src][2][MAX_LINES][8][2], or NULL: no runs anywhere
  const int32_t* counts;   // [n_frames][n_src][2][MAX_LINES]
  uint16_t* out;           // [n_frames][H][W] packed
  int32_t n_src, W, H, ntsc, mode, threshold;
};

// V pixels of one row from x0: V == 8 through 16-byte loads and one 16-byte store (the
// caller guarantees the alignment), V == 1 through 2-byte ones (a row's head and tail)
template <int N, int V>
__device__ __forceinline__ void stack_span(const StackArgs& A, int64_t row0, int x0, uint32_t pmask, int base,
                                           const int32_t* c0, const int32_t* rr) {
  constexpr int NW = V == 8 ? 4 : 1;
  uint32_t raw[N][NW];
#pragma unroll
  for (int s = 0; s < N; s++) {
#pragma unroll
    for (int w = 0; w < NW; w++) raw[s][w] = 0;
    if ((pmask >> s) & 1u) {                       // wave-uniform
      const uint16_t* p = A.src + (int64_t)s * A.src_stride + row0 + x0;
      if constexpr (V == 8) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        raw[s][0] = q.x;
        raw[s][1] = q.y;
        raw[s][2] = q.z;
        raw[s][3] = q.w;
      } else {
        raw[s][0] = *p;
      }
    }
  }
  // the sources with a run over each pixel
  uint32_t drop[V];
#pragma unroll
  for (int j = 0; j < V; j++) drop[j] = 0;
  if (c0) {                                        // some present source has a run in this row
#pragma unroll
    for (int s = 0; s < N; s++) {
      int n = ((pmask >> s) & 1u) ? c0[(int64_t)s * 2 * MAX_LINES] : 0;
      n = n > LDG_MAX_DROPOUTS_PER_LINE ? LDG_MAX_DROPOUTS_PER_LINE : n;
      for (int k = 0; k < n; k++) {                // wave-uniform trip count
        const int32_t w = rr[(int64_t)s * STACK_RUNS_STRIDE + k];   // (startx, endx) as one 32-bit word
        int sx = (int16_t)(w & 0xffff), ex = (int16_t)(w >> 16);
        if (sx < 0) sx = 0;
        if (ex > A.W) ex = A.W;
#pragma unroll
        for (int j = 0; j < V; j++) drop[j] |= (x0 + j >= sx && x0 + j < ex) ? (1u << s) : 0u;
      }
    }
  }
  uint32_t res[V];
#pragma unroll
  for (int j = 0; j < V; j++) {
    int val[N];
#pragma unroll
    for (int s = 0; s < N; s++) val[s] = (int)((raw[s][j >> 1] >> (16 * (j & 1))) & 0xffffu);
    uint32_t cand = pmask & ~drop[j];
    if (cand == 0) cand = pmask;                   // every source lost it: a residual dropout
    // the burst flag pixels are base's: of one candidate every mode gives the value itself
    if (A.ntsc && x0 + j < 2) cand = 1u << base;
    res[j] = (uint32_t)stack_pixel<N>(val, cand, A.mode, A.threshold);
  }
  uint16_t* o = A.out + row0 + x0;
  if constexpr (V == 8) {
    uint4 q;
    q.x = res[0] | (res[1] << 16);
    q.y = res[2] | (res[3] << 16);
    q.z = res[4] | (res[5] << 16);
    q.w = res[6] | (res[7] << 16);
    *reinterpret_cast<uint4*>(o) = q;
  } else {
    *o = (uint16_t)res[0];
  }
}

// grid: (H frame rows, n frames) x STACK_THREADS threads, one workgroup per frame row, so
// the sources present and their run counts are uniform: a row without runs takes one
// branch and never looks at a run or a count.  N: the source slots the kernel is unrolled
// for (>= n_src; the slots past n_src are absent).  The frames are packed (a PAL row is 2270
// bytes), so a row starts on any 2-byte phase of 16: its first (-row0 mod 8) pixels and
// the rest past the last whole group of 8 go through 2-byte accesses, the groups between
// through 16-byte ones.  The sources and the output share one packed layout from 16-byte
// aligned bases, so one phase holds for all of them.
template <int N>
__global__ __launch_bounds__(STACK_THREADS) void ldg_k_stack(StackArgs A) {
  const int f = blockIdx.y, y = blockIdx.x;
  const int p = y & 1, r = y >> 1;
  const uint32_t info = A.rowinfo[(int64_t)f * A.H + y];
  const uint32_t pmask = info & ((1u << N) - 1u) & 0xffffu;
  if (pmask == 0) return;                          // (refused by the host: never reached)
  const int base = __ffs(pmask) - 1;
  const int32_t *c0 = nullptr, *rr = nullptr;
  if (info >> 31) {
    // this row's entries of source 0; source s lies two entries (the two parities) on per s
    const int64_t e0 = ((int64_t)f * A.n_src) * 2 + p;
    c0 = A.counts + e0 * MAX_LINES + r;
    rr = reinterpret_cast<const int32_t*>(A.runs + e0 * STACK_RUNS_STRIDE) + r * LDG_MAX_DROPOUTS_PER_LINE;
  }
  const int64_t row0 = ((int64_t)f * A.H + y) * A.W;
  const int head = (int)((8 - (row0 & 7)) & 7);    // pixels before the first 16-byte boundary
  const int ng = (A.W - head) >> 3;                // whole groups of 8
  const int tail0 = head + 8 * ng;
  for (int g = threadIdx.x; g < ng; g += STACK_THREADS)
    stack_span<N, 8>(A, row0, head + 8 * g, pmask, base, c0, rr);
  const int ne = head + (A.W - tail0);             // head and tail pixels, at most 14
  // from the last thread down: the second wave, which has the fewer groups of 8
  const int t = STACK_THREADS - 1 - (int)threadIdx.x;
  if (t < ne) {
    stack_span<N, 1>(A, row0, t < head ? t : tail0 + (t - head), pmask, base, c0, rr);
  }
}

}  // namespace ldg
