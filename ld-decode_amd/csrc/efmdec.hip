// EFM run lengths -> F3 frames -> CIRC -> 44.1 kHz PCM.  BUILD-DEFINED (DESIGN.md section 7d,
// row F8; tests/efmdec_ref.py is the numpy restatement): the snapshot this project follows
// has the code table as data and no decoder.  Integers throughout; the GPU equals the
// restatement byte for byte.
//
//   ldg_k_efmdec_runsum   the tiles' sums of run lengths (ldg_k_efm_scan over them gives the
//                         64-bit transition positions' tile offsets)
//   ldg_k_efmdec_cand     the positions; the sync candidates (11, 11), counted then written
//   ldg_k_efmdec_confirm  candidates with another at +-588 (binary search), counted / written
//   ldg_k_efmdec_frames   frames per confirmed candidate (coasting), counted / written
//   ldg_k_efmdec_finish   where the next call restarts (efmdec_plan.hpp)
//   ldg_k_efmdec_symbols  a wave per frame: its channel bits in LDS, 33 lanes look them up
//   ldg_k_efmdec_c1 / c2  a thread per frame, GF(2^8) log / antilog tables in LDS
//   ldg_k_efmdec_pcm      delay, sample map, flags;  ldg_k_efmdec_conceal  the output
//
// The count / scan / write shape, wg_scan and ldg_k_efm_scan are efm.hip's.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "efmdec_plan.hpp"

namespace ldg {
namespace efmdec {

using ldg::efm::wg_scan;

constexpr int RUN_TILE = 1024;          // run lengths per workgroup (four a thread)
constexpr int SYM_FRAMES = 4;           // frames (waves) per symbol workgroup
constexpr int MASK_WORDS = 20;          // 588 bits
constexpr int GF_BYTES = 768;           // antilog[512] (doubled: no modulo after an add), log[256]

enum {                                  // counters (unsigned long long each), one call's
  K_BAD = 0, K_C1_PASS, K_C1_FIXED, K_C1_ERASED, K_C2_PASS, K_C2_FIXED, K_C2_SOLVED, K_C2_FAILED, K_C2_UNSOLVED,
  K_FLAGGED, K_AVERAGED, K_MUTED, K_COASTED, K_BREAKS, K_COUNT
};

__device__ __forceinline__ void count(unsigned long long* cnt, int which, bool yes) {
  // one atomic per wave and counter
  const unsigned long long m = __ballot(yes);
  if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(cnt + which, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void ldg_k_efmdec_runsum(const uint8_t* __restrict__ rl, int64_t n,
                                                           int32_t* __restrict__ sums) {
  __shared__ int32_t sh[256];
  const int64_t i0 = (int64_t)blockIdx.x * RUN_TILE + 4 * threadIdx.x;
  int32_t s = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) s += i0 + r < n ? rl[i0 + r] : 0;
  int32_t total;
  wg_scan<int32_t, 256>(s, sh, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// WRITE == false: pos[i] = pos0 + the run lengths before i (pos[n] too), and the tile's count
// of candidates (rl[i] == rl[i + 1] == 11, at pos[i]).  WRITE == true: the candidates, in order.
template <bool WRITE>
__global__ __launch_bounds__(256) void ldg_k_efmdec_cand(const uint8_t* __restrict__ rl, int64_t n, int64_t pos0,
                                                         const int64_t* __restrict__ toffs, int64_t* __restrict__ pos,
                                                         int32_t* __restrict__ ccnt, const int64_t* __restrict__ coffs,
                                                         int64_t* __restrict__ cand) {
  __shared__ int32_t sh[256];
  const int64_t i0 = (int64_t)blockIdx.x * RUN_TILE + 4 * threadIdx.x;
  int32_t r[5], s = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) r[k] = i0 + k < n ? rl[i0 + k] : 0;
#pragma unroll
  for (int k = 0; k < 4; k++) s += r[k];
  int32_t total;
  const int32_t ex = wg_scan<int32_t, 256>(s, sh, &total);
  int64_t p = pos0 + toffs[blockIdx.x] + ex;
  int64_t at[4];
  int32_t c = 0;
  bool is[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    at[k] = p;
    is[k] = i0 + k + 1 < n && r[k] == 11 && r[k + 1] == 11;
    c += is[k] ? 1 : 0;
    if (!WRITE && i0 + k < n) {
      pos[i0 + k] = p;
      if (i0 + k == n - 1) pos[n] = p + r[k];
    }
    p += r[k];
  }
  const int32_t rank = wg_scan<int32_t, 256>(c, sh, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) ccnt[blockIdx.x] = total;
    return;
  }
  int64_t o = coffs[blockIdx.x] + rank;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (is[k]) cand[o++] = at[k];
}

__device__ __forceinline__ bool has(const int64_t* __restrict__ v, int64_t n, int64_t x) {
  const int64_t k = lower_bound(v, n, x);
  return k < n && v[k] == x;
}

// a candidate per thread: confirmed when another sits at exactly +-588
template <bool WRITE>
__global__ __launch_bounds__(256) void ldg_k_efmdec_confirm(const int64_t* __restrict__ cand, int64_t nc,
                                                            int32_t* __restrict__ cnt, const int64_t* __restrict__ offs,
                                                            int64_t* __restrict__ conf) {
  __shared__ int32_t sh[256];
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t c = 0;
  bool ok = false;
  if (j < nc) {
    c = cand[j];
    ok = has(cand, nc, c + FRAME_BITS) || has(cand, nc, c - FRAME_BITS);
  }
  int32_t total;
  const int32_t rank = wg_scan<int32_t, 256>(ok ? 1 : 0, sh, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
  } else if (ok) {
    conf[offs[blockIdx.x] + rank] = c;
  }
}

// a confirmed candidate per thread: its frames (efmdec_plan.hpp frames_of); pend: pos[n]
template <bool WRITE>
__global__ __launch_bounds__(256) void ldg_k_efmdec_frames(const int64_t* __restrict__ conf, int64_t nconf,
                                                           const int64_t* __restrict__ pend, int64_t emit_from,
                                                           int final_, int32_t* __restrict__ cnt,
                                                           const int64_t* __restrict__ offs, int64_t* __restrict__ starts,
                                                           unsigned long long* __restrict__ counters) {
  __shared__ int32_t sh[256];
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t end = *pend;
  const Window w{emit_from, final_ ? NEVER : end - SETTLE, end, final_};
  int brk = 0;
  const int64_t m = k < nconf ? frames_of(conf, nconf, k, w, &brk) : 0;
  int32_t total;
  const int32_t rank = wg_scan<int32_t, 256>((int32_t)m, sh, &total);   // m <= 7350, 256 of them fit
  if (!WRITE) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    return;
  }
  const int64_t o = offs[blockIdx.x] + rank;
  for (int64_t j = 0; j < m; j++) starts[o + j] = conf[k] + FRAME_BITS * j;
  if (m > 1) atomicAdd(counters + K_COASTED, (unsigned long long)(m - 1));
  if (brk) atomicAdd(counters + K_BREAKS, 1ull);
}

__global__ void ldg_k_efmdec_finish(const int64_t* __restrict__ pos, int64_t nrun, const int64_t* __restrict__ cand,
                                    int64_t ncand, const int64_t* __restrict__ conf, int64_t nconf, int64_t emit_from,
                                    int final_, GridOut* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  const int64_t end = pos[nrun];
  const Window w{emit_from, final_ ? NEVER : end - SETTLE, end, final_};
  GridOut g;
  finish(pos, nrun, cand, ncand, conf, nconf, w, &g);
  *out = g;
}

// Frame f of starts[0 .. nf): symbol s is the 14 bits from start + 27 + 17 s, MSB first,
// through the inverse table.  Symbol 0 (subcode) stays u16; a symbol 1..32 that is no data
// word becomes 0 and counts.  pos[0 .. npos) ascend; every frame's bits lie below pos[npos - 1].
__global__ __launch_bounds__(64 * SYM_FRAMES) void ldg_k_efmdec_symbols(const int64_t* __restrict__ pos, int64_t npos,
                                                                       const int64_t* __restrict__ starts, int64_t nf,
                                                                       const uint16_t* __restrict__ inv,
                                                                       uint16_t* __restrict__ sub, uint8_t* __restrict__ f3,
                                                                       unsigned long long* __restrict__ counters) {
  __shared__ uint32_t mask[SYM_FRAMES][MASK_WORDS];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * SYM_FRAMES + wv;
  if (lane < MASK_WORDS) mask[wv][lane] = 0;
  __syncthreads();
  const bool live = f < nf;
  int64_t s = 0;
  if (live) {
    s = starts[f];
    for (int64_t i = lower_bound(pos, npos, s + 27) + lane; i < npos; i += 64) {
      const int64_t b = pos[i] - s;
      if (b >= FRAME_BITS) break;
      atomicOr(&mask[wv][b >> 5], 1u << (b & 31));
    }
  }
  __syncthreads();
  bool bad = false;
  if (live && lane < 33) {
    const int o = 27 + 17 * lane;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 14; j++) v = v << 1 | (mask[wv][(o + j) >> 5] >> ((o + j) & 31) & 1u);
    const uint16_t sym = inv[v];
    if (lane == 0) {
      sub[f] = sym;
    } else {
      bad = sym > 255;
      f3[f * 32 + lane - 1] = bad ? (uint8_t)0 : (uint8_t)sym;
    }
  }
  count(counters, K_BAD, bad);
}

// ---- GF(2^8), polynomial 0x11d, alpha = 2 --------------------------------------------------

struct GF {
  const uint8_t* t;     // LDS: antilog[512], log[256]
  __device__ __forceinline__ uint32_t ex(int i) const { return t[i]; }
  __device__ __forceinline__ int lg(uint32_t a) const { return t[512 + a]; }
  __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) const { return (a && b) ? t[lg(a) + lg(b)] : 0u; }
  __device__ __forceinline__ uint32_t div(uint32_t a, uint32_t b) const { return a ? t[lg(a) + 255 - lg(b)] : 0u; }   // b != 0
};

__device__ __forceinline__ void gf_load(uint8_t* sh, const uint8_t* __restrict__ g) {
  for (int i = threadIdx.x; i < GF_BYTES; i += blockDim.x) sh[i] = g[i];
  __syncthreads();
}

__device__ __forceinline__ uint32_t xt(uint32_t a) { return ((a << 1) ^ ((a & 0x80u) ? 0x11du : 0u)) & 0xffu; }

// S_k = sum c[i] alpha^(k (N - 1 - i)), by Horner
template <int N>
__device__ __forceinline__ void syndromes(const uint32_t (&c)[N], uint32_t (&S)[4]) {
  S[0] = S[1] = S[2] = S[3] = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    S[0] ^= c[i];
    S[1] = xt(S[1]) ^ c[i];
    S[2] = xt(xt(S[2])) ^ c[i];
    S[3] = xt(xt(xt(S[3]))) ^ c[i];
  }
}

// the one error the syndromes name: its index in the word, or -1 (S all non-zero, the three
// ratios equal alpha^p, p < N)
template <int N>
__device__ __forceinline__ int single_error(const GF& G, const uint32_t (&S)[4]) {
  if (!S[0] || !S[1] || !S[2] || !S[3]) return -1;
  const int l0 = G.lg(S[0]), l1 = G.lg(S[1]), l2 = G.lg(S[2]), l3 = G.lg(S[3]);
  const int p = (l1 - l0 + 255) % 255;
  if ((l2 - l1 + 255) % 255 != p || (l3 - l2 + 255) % 255 != p || p >= N) return -1;
  return N - 1 - p;
}

__device__ __forceinline__ void store_row28(uint8_t* __restrict__ dst, const uint32_t (&w)[28], int p0, uint32_t v0, int p1,
                                            uint32_t v1, int p2, uint32_t v2, int p3, uint32_t v3) {
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);           // rows of 28 bytes: four-byte aligned
#pragma unroll
  for (int q = 0; q < 7; q++) {
    uint32_t x = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int j = 4 * q + b;
      uint32_t v = w[j];
      v ^= j == p0 ? v0 : 0u;
      v ^= j == p1 ? v1 : 0u;
      v ^= j == p2 ? v2 : 0u;
      v ^= j == p3 ? v3 : 0u;
      x |= v << (8 * b);
    }
    d[q] = x;
  }
}

// C1 of local frames 1 .. nf - 1: u = (even symbols of the frame before, odd of this one),
// parity inverted; a clean word passes, one error is corrected, anything else erases the 28
// outputs (flag 1; the symbols pass through).  Counted from local frame count_from on.
__global__ __launch_bounds__(256) void ldg_k_efmdec_c1(const uint8_t* __restrict__ f3, int64_t nf, const uint8_t* __restrict__ gf,
                                                       int64_t count_from, uint8_t* __restrict__ c1, uint8_t* __restrict__ c1f,
                                                       unsigned long long* __restrict__ counters) {
  __shared__ uint8_t sh[GF_BYTES];
  gf_load(sh, gf);
  const GF G{sh};
  const int64_t i = 1 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < nf;
  int what = -1;
  if (live) {
    const uint32_t* a = reinterpret_cast<const uint32_t*>(f3 + (i - 1) * 32);
    const uint32_t* b = reinterpret_cast<const uint32_t*>(f3 + i * 32);
    uint32_t u[32];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const uint32_t x = a[q], y = b[q];
      u[4 * q] = x & 255u;
      u[4 * q + 1] = y >> 8 & 255u;
      u[4 * q + 2] = x >> 16 & 255u;
      u[4 * q + 3] = y >> 24;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      u[12 + k] ^= 255u;
      u[28 + k] ^= 255u;
    }
    uint32_t S[4];
    syndromes<32>(u, S);
    int p = -1;
    if ((S[0] | S[1] | S[2] | S[3]) == 0) {
      what = K_C1_PASS;
    } else {
      p = single_error<32>(G, S);
      what = p >= 0 ? K_C1_FIXED : K_C1_ERASED;
    }
    uint32_t w[28];
#pragma unroll
    for (int j = 0; j < 28; j++) w[j] = u[j];
    store_row28(c1 + i * 28, w, p, S[0], -1, 0, -1, 0, -1, 0);
    c1f[i] = what == K_C1_ERASED ? 1 : 0;
  }
  const bool cnt = live && i >= count_from;
  count(counters, K_C1_PASS, cnt && what == K_C1_PASS);
  count(counters, K_C1_FIXED, cnt && what == K_C1_FIXED);
  count(counters, K_C1_ERASED, cnt && what == K_C1_ERASED);
}

// C2 of local frames 109 .. nf - 1: symbol j from C1 frame n - 4 (27 - j).  No erasure: up to
// two errors.  One to four erasures: solved from the first e syndromes, accepted when all four
// then vanish.  More: passed through, the erased ones flagged.  A failed word flags all.
__global__ __launch_bounds__(256) void ldg_k_efmdec_c2(const uint8_t* __restrict__ c1, const uint8_t* __restrict__ c1f, int64_t nf,
                                                       const uint8_t* __restrict__ gf, int64_t count_from,
                                                       uint8_t* __restrict__ c2, uint32_t* __restrict__ c2f,
                                                       unsigned long long* __restrict__ counters) {
  __shared__ uint8_t sh[GF_BYTES];
  gf_load(sh, gf);
  const GF G{sh};
  const int64_t i = C2_FIRST + (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < nf;
  int what = -1;
  if (live) {
    uint32_t w[28], S[4];
    uint32_t er = 0;
    int e = 0, ej[4] = {-1, -1, -1, -1};
#pragma unroll
    for (int j = 0; j < 28; j++) {
      const int64_t src = i - 4 * (27 - j);
      w[j] = c1[src * 28 + j];
      if (c1f[src]) {
        er |= 1u << j;
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (e == q) ej[q] = j;
        e++;
      }
    }
    syndromes<28>(w, S);
    int cp[4] = {-1, -1, -1, -1};
    uint32_t cv[4] = {0, 0, 0, 0}, flags = 0;
    if (e == 0) {
      if ((S[0] | S[1] | S[2] | S[3]) == 0) {
        what = K_C2_PASS;
      } else {
        what = K_C2_FAILED;
        const int p = single_error<28>(G, S);
        if (p >= 0) {
          cp[0] = p;
          cv[0] = S[0];
          what = K_C2_FIXED;
        } else {
          const uint32_t det = G.mul(S[0], S[2]) ^ G.mul(S[1], S[1]);
          if (det) {
            const uint32_t s1 = G.div(G.mul(S[0], S[3]) ^ G.mul(S[1], S[2]), det);
            const uint32_t s2 = G.div(G.mul(S[1], S[3]) ^ G.mul(S[2], S[2]), det);
            int nr = 0, r0 = -1, r1 = -1;
#pragma unroll
            for (int j = 0; j < 28; j++) {
              const uint32_t x = G.ex(27 - j);
              if ((G.mul(x, x) ^ G.mul(s1, x) ^ s2) == 0) {
                if (nr == 0) r0 = j;
                else if (nr == 1) r1 = j;
                nr++;
              }
            }
            if (nr == 2) {
              const uint32_t x1 = G.ex(27 - r0), x2 = G.ex(27 - r1);
              const uint32_t y1 = G.div(G.mul(S[0], x2) ^ S[1], x1 ^ x2), y2 = S[0] ^ y1;
              const uint32_t x1s = G.mul(x1, x1), x2s = G.mul(x2, x2);
              const uint32_t t2 = S[2] ^ G.mul(y1, x1s) ^ G.mul(y2, x2s);
              const uint32_t t3 = S[3] ^ G.mul(y1, G.mul(x1s, x1)) ^ G.mul(y2, G.mul(x2s, x2));
              if ((t2 | t3) == 0) {
                cp[0] = r0;
                cv[0] = y1;
                cp[1] = r1;
                cv[1] = y2;
                what = K_C2_FIXED;
              }
            }
          }
        }
        if (what == K_C2_FAILED) flags = 0x0fffffffu;
      }
    } else if (e <= 4) {
      // sum_q Y_q X_q^k = S_k, k < e: elimination without pivoting (a Vandermonde matrix's
      // leading minors are Vandermonde determinants of distinct X: never zero)
      uint32_t X[4], A[4][5];
#pragma unroll
      for (int q = 0; q < 4; q++) X[q] = q < e ? G.ex(27 - ej[q]) : 0u;
#pragma unroll
      for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          uint32_t v = 1;
#pragma unroll
          for (int m = 0; m < 4; m++)
            if (m < k) v = G.mul(v, X[q]);
          A[k][q] = (k < e && q < e) ? v : (k == q ? 1u : 0u);
        }
        A[k][4] = k < e ? S[k] : 0u;
      }
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const uint32_t d = A[c][c];
#pragma unroll
        for (int q = 0; q < 5; q++) A[c][q] = G.div(A[c][q], d);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          if (r == c) continue;
          const uint32_t fct = A[r][c];
#pragma unroll
          for (int q = 0; q < 5; q++) A[r][q] ^= G.mul(fct, A[c][q]);
        }
      }
      uint32_t T[4] = {S[0], S[1], S[2], S[3]};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        uint32_t xp = 1;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (q < e) T[k] ^= G.mul(A[q][4], xp);
          xp = G.mul(xp, X[q]);
        }
      }
      if ((T[0] | T[1] | T[2] | T[3]) == 0) {
        what = K_C2_SOLVED;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          cp[q] = q < e ? ej[q] : -1;
          cv[q] = A[q][4];
        }
      } else {
        what = K_C2_FAILED;
        flags = 0x0fffffffu;
      }
    } else {
      what = K_C2_UNSOLVED;
      flags = er;
    }
    store_row28(c2 + i * 28, w, cp[0], cv[0], cp[1], cv[1], cp[2], cv[2], cp[3], cv[3]);
    c2f[i] = flags;
  }
  const bool cnt = live && i >= count_from;
  count(counters, K_C2_PASS, cnt && what == K_C2_PASS);
  count(counters, K_C2_FIXED, cnt && what == K_C2_FIXED);
  count(counters, K_C2_SOLVED, cnt && what == K_C2_SOLVED);
  count(counters, K_C2_FAILED, cnt && what == K_C2_FAILED);
  count(counters, K_C2_UNSOLVED, cnt && what == K_C2_UNSOLVED);
}

// Samples of local frames 111 .. nf - 1, a thread per (frame, sample t of 6, channel): byte
// pair at position p (high byte first) of C2 word n (p < 12) or n - 2 (p >= 16); flagged if
// either byte is.  raw / rawf: [(frame - 111) * 6 + t][channel].
__global__ __launch_bounds__(256) void ldg_k_efmdec_pcm(const uint8_t* __restrict__ c2, const uint32_t* __restrict__ c2f, int64_t nf,
                                                        int16_t* __restrict__ raw, uint8_t* __restrict__ rawf) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (nf - LATENCY) * 12) return;
  const int64_t i = LATENCY + q / 12;
  const int r = (int)(q % 12), t = r >> 1, ch = r & 1;
  const int p = ((t & 1) ? 16 : 0) + (t >> 1) * 2 + 6 * ch;
  const int64_t src = p >= 16 ? i - 2 : i;
  const uint32_t hi = c2[src * 28 + p], lo = c2[src * 28 + p + 1];
  raw[q] = (int16_t)(uint16_t)(hi << 8 | lo);
  rawf[q] = (uint8_t)((c2f[src] >> p | c2f[src] >> (p + 1)) & 1u);
}

// Output element q of n (sample, channel interleaved) is raw element first + q of nraw: a
// flagged sample between unflagged neighbours of its channel becomes their mean (arithmetic
// shift), any other flagged sample 0.
__global__ __launch_bounds__(256) void ldg_k_efmdec_conceal(const int16_t* __restrict__ raw, const uint8_t* __restrict__ rawf,
                                                            int64_t nraw, int64_t first, int64_t n, int16_t* __restrict__ pcm,
                                                            uint8_t* __restrict__ flg, unsigned long long* __restrict__ counters) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool flagged = false, avg = false;
  if (q < n) {
    const int64_t r = first + q;
    int16_t v = raw[r];
    flagged = rawf[r] != 0;
    if (flagged) {
      avg = r - 2 >= 0 && r + 2 < nraw && !rawf[r - 2] && !rawf[r + 2];
      v = avg ? (int16_t)(((int32_t)raw[r - 2] + (int32_t)raw[r + 2]) >> 1) : (int16_t)0;
    }
    pcm[q] = v;
    flg[q] = flagged ? 1 : 0;
  }
  count(counters, K_FLAGGED, flagged);
  count(counters, K_AVERAGED, avg);
  count(counters, K_MUTED, flagged && !avg);
}

}  // namespace efmdec
}  // namespace ldg
