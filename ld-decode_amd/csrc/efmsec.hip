// EFM data sectors: the C2 output -> bytes with per-byte erasures -> the 2352-byte sector grid
// -> descramble -> EDC -> the Reed-Solomon product code (CD-ROM mode 1, ECMA-130).
// BUILD-DEFINED (tests/efmsec_ref.py is the numpy restatement):
// the snapshot this project follows has no sector decoder.  Integers throughout; the GPU equals
// the restatement byte for byte.
//
//   ldg_k_efmsec_gather   C2 rows and flags -> the bytes of the .efm.pcm file before concealment
//                         and a flag per byte
//   ldg_k_efmsec_cand     the candidates (00 FF x 10 00), counted then written
//   ldg_k_efmsec_confirm  candidates with another at +-2352 (binary search), counted / written
//   ldg_k_efmsec_sectors  sectors per confirmed candidate (coasting), counted / written
//   ldg_k_efmsec_finish   where the next call restarts (efmsec_plan.hpp)
//   ldg_k_efmsec_fix      a workgroup per sector: sync, descramble, EDC, rounds of P and Q
//
// The count / scan / write shape, wg_scan and ldg_k_efm_scan are efm.hip's; the field (0x11d,
// alpha = 2), its tables and the counting are efmdec.hip's.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "efmsec_plan.hpp"

namespace ldg {
namespace efmsec {

using ldg::efm::wg_scan;
using ldg::efmdec::GF;
using ldg::efmdec::GF_BYTES;

constexpr int CAND_TILE = 1024;         // byte positions per workgroup (four a thread)
constexpr int FIX_THREADS = 256;
constexpr int EDC_BYTES = 2064;         // the EDC covers bytes 0..2063
constexpr int EDC_LANES = 172;          // twelve bytes a lane
constexpr int EDC_CHUNK = 12;
constexpr uint32_t EDC_POLY = 0xD8018001u;
constexpr int MAX_ROUNDS = 8;

enum { ST_GOOD = 0, ST_CORRECTED = 1, ST_BAD = 2, ST_OTHER = 3 };

enum {                                  // counters (unsigned long long each), one call's
  K_COASTED = 0, K_BREAKS, K_GOOD, K_CORRECTED, K_BAD, K_OTHER, K_P_FIXED, K_Q_FIXED, K_ERASED, K_COUNT
};

struct Rec {                            // ldg_efmsec_rec
  int32_t status, rounds, erased;
  uint8_t minute, second, frame, mode;
};

// Byte b of nb: local frame first + b / 24 of the C2 rows, byte b % 24 of its 24 -- L0 R0 L1 R1
// .. L5 R5, low byte then high byte.  The high byte of a sample is C2 position p, the low byte
// p + 1, of row n (p < 12) or n - 2 (p >= 16); first >= 111, so row n - 2 exists.
__global__ __launch_bounds__(256) void ldg_k_efmsec_gather(const uint8_t* __restrict__ c2, const uint32_t* __restrict__ c2f,
                                                           int64_t first, int64_t nb, uint8_t* __restrict__ by,
                                                           uint8_t* __restrict__ er) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  const int64_t i = first + b / 24;
  const int r = (int)(b % 24), t = r >> 2, ch = (r >> 1) & 1;
  const int p = ((t & 1) ? 16 : 0) + (t >> 1) * 2 + 6 * ch + ((r & 1) ? 0 : 1);
  const int64_t src = p >= 16 ? i - 2 : i;
  by[b] = c2[src * 28 + p];
  er[b] = (uint8_t)(c2f[src] >> p & 1u);
}

// WRITE == false: the tile's count of candidates (bytes i .. i + 11 of the nb held are the
// pattern).  WRITE == true: their positions pos0 + i, in order.
template <bool WRITE>
__global__ __launch_bounds__(256) void ldg_k_efmsec_cand(const uint8_t* __restrict__ by, int64_t nb, int64_t pos0,
                                                         int32_t* __restrict__ ccnt, const int64_t* __restrict__ coffs,
                                                         int64_t* __restrict__ cand) {
  __shared__ int32_t sh[256];
  const int64_t i0 = (int64_t)blockIdx.x * CAND_TILE + 4 * threadIdx.x;
  uint32_t v[15];
#pragma unroll
  for (int k = 0; k < 15; k++) v[k] = i0 + k < nb ? by[i0 + k] : 1u;       // 1: part of no pattern
  bool is[4];
  int32_t c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    bool ok = v[k] == 0u && v[k + 11] == 0u;
#pragma unroll
    for (int j = 1; j <= 10; j++) ok = ok && v[k + j] == 255u;
    is[k] = ok;
    c += ok ? 1 : 0;
  }
  int32_t total;
  const int32_t rank = wg_scan<int32_t, 256>(c, sh, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) ccnt[blockIdx.x] = total;
    return;
  }
  int64_t o = coffs[blockIdx.x] + rank;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (is[k]) cand[o++] = pos0 + i0 + k;
}

__device__ __forceinline__ bool has(const int64_t* __restrict__ v, int64_t n, int64_t x) {
  const int64_t k = lower_bound(v, n, x);
  return k < n && v[k] == x;
}

// a candidate per thread: confirmed when another sits at exactly +-2352
template <bool WRITE>
__global__ __launch_bounds__(256) void ldg_k_efmsec_confirm(const int64_t* __restrict__ cand, int64_t nc,
                                                            int32_t* __restrict__ cnt, const int64_t* __restrict__ offs,
                                                            int64_t* __restrict__ conf) {
  __shared__ int32_t sh[256];
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t c = 0;
  bool ok = false;
  if (j < nc) {
    c = cand[j];
    ok = has(cand, nc, c + SECTOR) || has(cand, nc, c - SECTOR);
  }
  int32_t total;
  const int32_t rank = wg_scan<int32_t, 256>(ok ? 1 : 0, sh, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
  } else if (ok) {
    conf[offs[blockIdx.x] + rank] = c;
  }
}

// a confirmed candidate per thread: its sectors (efmsec_plan.hpp sectors_of)
template <bool WRITE>
__global__ __launch_bounds__(256) void ldg_k_efmsec_sectors(const int64_t* __restrict__ conf, int64_t nconf, Window w,
                                                            int32_t* __restrict__ cnt, const int64_t* __restrict__ offs,
                                                            int64_t* __restrict__ starts,
                                                            unsigned long long* __restrict__ counters) {
  __shared__ int32_t sh[256];
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int brk = 0;
  const int64_t m = k < nconf ? sectors_of(conf, nconf, k, w, &brk) : 0;
  int32_t total;
  const int32_t rank = wg_scan<int32_t, 256>((int32_t)m, sh, &total);     // m <= 75
  if (!WRITE) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    return;
  }
  const int64_t o = offs[blockIdx.x] + rank;
  for (int64_t j = 0; j < m; j++) starts[o + j] = conf[k] + SECTOR * j;
  if (m > 1) atomicAdd(counters + K_COASTED, (unsigned long long)(m - 1));
  if (brk) atomicAdd(counters + K_BREAKS, 1ull);
}

__global__ void ldg_k_efmsec_finish(int64_t pos0, const int64_t* __restrict__ cand, int64_t ncand,
                                    const int64_t* __restrict__ conf, int64_t nconf, Window w, GridOut* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  GridOut g;
  finish(pos0, cand, ncand, conf, nconf, w, &g);
  *out = g;
}

// ---- one sector ----------------------------------------------------------------------------

// a times b modulo the EDC polynomial, both in the reflected form (bit 31 is x^0)
__device__ __forceinline__ uint32_t edc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 4
  for (int k = 31; k >= 0; k--) {
    p ^= (a >> k & 1u) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? EDC_POLY : 0u);
  }
  return p;
}

// The EDC of sec[0 .. 2063] (initial value 0, no final XOR: linear), on every thread: lane i
// of 172 takes twelve bytes and multiplies their CRC by x^(8 * bytes after them) (xp[i]).
__device__ __forceinline__ uint32_t edc_of(const uint8_t* sec, const uint32_t* __restrict__ xp, uint32_t* red) {
  const int t = threadIdx.x;
  uint32_t c = 0;
  if (t < EDC_LANES) {
    for (int k = 0; k < EDC_CHUNK; k++) {
      c ^= sec[t * EDC_CHUNK + k];
#pragma unroll
      for (int b = 0; b < 8; b++) c = (c >> 1) ^ ((c & 1u) ? EDC_POLY : 0u);
    }
    c = edc_mul(xp[t], c);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c ^= __shfl_xor(c, off, 64);
  __syncthreads();                                 // red is free again
  if ((t & 63) == 0) red[t >> 6] = c;
  __syncthreads();
  return red[0] ^ red[1] ^ red[2] ^ red[3];
}

// byte index of symbol i of P word n (0..42) / Q word n (0..25) of plane h
__device__ __forceinline__ int p_index(int h, int n, int i) { return 12 + 2 * (43 * i + n) + h; }
__device__ __forceinline__ int q_index(int h, int n, int i) {
  const int s = i < 43 ? (44 * i + 43 * n) % 1118 : (i == 43 ? 1118 + n : 1144 + n);
  return 12 + 2 * s + h;
}

// One word of N symbols in LDS: S0 = sum c[i], S1 = sum c[i] alpha^(N - 1 - i) (Horner), its
// erased symbols counted and the first two kept; then the rule of DESIGN.md section 7e step 6.
// -> the word was changed (a symbol corrected or a flag cleared).
template <int N, bool Q>
__device__ __forceinline__ bool fix_word(const GF& G, uint8_t* sec, uint8_t* flg, int h, int n) {
  uint32_t S0 = 0, S1 = 0;
  int e = 0, j0 = 0, j1 = 0;
  for (int i = 0; i < N; i++) {
    const int at = Q ? q_index(h, n, i) : p_index(h, n, i);
    const uint32_t c = sec[at];
    S0 ^= c;
    S1 = ldg::efmdec::xt(S1) ^ c;
    if (flg[at]) {
      if (e == 0) j0 = i;
      else if (e == 1) j1 = i;
      e++;
    }
  }
  if (e == 0) {
    if (!S0 || !S1) return false;
    const int p = (G.lg(S1) - G.lg(S0) + 255) % 255;
    if (p >= N) return false;
    const int at = Q ? q_index(h, n, N - 1 - p) : p_index(h, n, N - 1 - p);
    sec[at] = (uint8_t)(sec[at] ^ S0);
    return true;
  }
  if (e == 1) {
    if (G.mul(S0, G.ex(N - 1 - j0)) != S1) return false;
    const int at = Q ? q_index(h, n, j0) : p_index(h, n, j0);
    sec[at] = (uint8_t)(sec[at] ^ S0);
    flg[at] = 0;
    return true;
  }
  if (e == 2) {
    const uint32_t x1 = G.ex(N - 1 - j0), x2 = G.ex(N - 1 - j1);        // distinct: x1 ^ x2 != 0
    const uint32_t y1 = G.div(G.mul(S0, x2) ^ S1, x1 ^ x2), y2 = S0 ^ y1;
    const int a0 = Q ? q_index(h, n, j0) : p_index(h, n, j0);
    const int a1 = Q ? q_index(h, n, j1) : p_index(h, n, j1);
    sec[a0] = (uint8_t)(sec[a0] ^ y1);
    sec[a1] = (uint8_t)(sec[a1] ^ y2);
    flg[a0] = 0;
    flg[a1] = 0;
    return true;
  }
  return false;
}

__device__ __forceinline__ void add_per_wave(unsigned long long* cnt, int which, int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if (v && (threadIdx.x & 63) == 0) atomicAdd(cnt + which, (unsigned long long)v);
}

// Sector blockIdx.x: the 2352 bytes from starts[s] (the buffer holds bytes from pos0 on; the
// grid kernels emit only sectors held whole).  Its sync bytes are set and their flags
// cleared, bytes 12.. descrambled, and that is what is written first.  A sector with no flag
// on bytes 12..2067, mode 1 and a matching EDC is good.  Any other goes through rounds of
// (P pass, Q pass, EDC) in LDS until it verifies -- then the repaired copy replaces the
// output -- or a round changes nothing (at most 8); an unverified repair is never passed on.
__global__ __launch_bounds__(FIX_THREADS) void ldg_k_efmsec_fix(const uint8_t* __restrict__ by, const uint8_t* __restrict__ er,
                                                                int64_t pos0, const int64_t* __restrict__ starts,
                                                                const uint8_t* __restrict__ gf, const uint8_t* __restrict__ scr,
                                                                const uint32_t* __restrict__ xp, uint8_t* __restrict__ sectors,
                                                                uint8_t* __restrict__ data, Rec* __restrict__ recs,
                                                                unsigned long long* __restrict__ counters) {
  __shared__ uint8_t sec[SECTOR];
  __shared__ uint8_t flg[SECTOR];
  __shared__ uint8_t gft[GF_BYTES];
  __shared__ uint32_t red[4];
  __shared__ int32_t s_erased, s_early, s_changed;
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t off = starts[s] - pos0;
  const uint8_t* src = by + off;
  const uint8_t* sfl = er + off;
  uint8_t* out = sectors + s * SECTOR;
  if (t == 0) s_erased = s_early = s_changed = 0;
  for (int i = t; i < GF_BYTES; i += FIX_THREADS) gft[i] = gf[i];
  __syncthreads();
  int my_erased = 0, my_early = 0;
  for (int i = t; i < SECTOR; i += FIX_THREADS) {
    uint8_t v, f = 0;
    if (i < 12) {
      v = (i == 0 || i == 11) ? (uint8_t)0 : (uint8_t)255;
    } else {
      v = (uint8_t)(src[i] ^ scr[i - 12]);
      f = sfl[i] ? 1 : 0;
    }
    sec[i] = v;
    flg[i] = f;
    out[i] = v;
    my_erased += f;
    my_early += (f && i < 2068) ? 1 : 0;
  }
  if (my_erased) atomicAdd(&s_erased, my_erased);
  if (my_early) atomicAdd(&s_early, my_early);
  __syncthreads();
  const GF G{gft};
  const int erased = s_erased;
  const uint32_t mode0 = sec[15];
  const bool head_flagged = (flg[12] | flg[13] | flg[14] | flg[15]) != 0;
  auto verified = [&]() {                          // workgroup-uniform
    const uint32_t c = edc_of(sec, xp, red);
    const uint32_t stored = sec[2064] | (uint32_t)sec[2065] << 8 | (uint32_t)sec[2066] << 16 | (uint32_t)sec[2067] << 24;
    return sec[15] == 1 && c == stored;
  };
  int status = ST_BAD, rounds = 0, pf = 0, qf = 0;
  if (s_early == 0 && verified()) {
    status = ST_GOOD;
  } else {
    while (rounds < MAX_ROUNDS) {
      rounds++;
      __syncthreads();
      if (t == 0) s_changed = 0;
      __syncthreads();
      bool ch = false;
      if (t < 86 && fix_word<26, false>(G, sec, flg, t / 43, t % 43)) {
        pf++;
        ch = true;
      }
      __syncthreads();
      if (t < 52 && fix_word<45, true>(G, sec, flg, t / 26, t % 26)) {
        qf++;
        ch = true;
      }
      if (ch) s_changed = 1;
      __syncthreads();
      if (verified()) {
        status = ST_CORRECTED;
        break;
      }
      if (!s_changed) break;
    }
    if (status == ST_CORRECTED) {
      for (int i = t; i < SECTOR; i += FIX_THREADS) out[i] = sec[i];
    } else {
      status = (mode0 != 1 && !head_flagged) ? ST_OTHER : ST_BAD;
    }
  }
  __syncthreads();
  // the user bytes and the header: of the repaired copy if it verified, else of what was written first
  const bool use = status == ST_CORRECTED || status == ST_GOOD;
  for (int i = t; i < 2048; i += FIX_THREADS)
    data[s * 2048 + i] = use ? sec[16 + i] : (uint8_t)(src[16 + i] ^ scr[4 + i]);
  if (t == 0) {
    Rec r;
    r.status = status;
    r.rounds = rounds;
    r.erased = erased;
    r.minute = use ? sec[12] : (uint8_t)(src[12] ^ scr[0]);
    r.second = use ? sec[13] : (uint8_t)(src[13] ^ scr[1]);
    r.frame = use ? sec[14] : (uint8_t)(src[14] ^ scr[2]);
    r.mode = use ? sec[15] : (uint8_t)mode0;
    recs[s] = r;
    atomicAdd(counters + K_GOOD + status, 1ull);   // K_GOOD, K_CORRECTED, K_BAD, K_OTHER follow the status codes
    if (erased) atomicAdd(counters + K_ERASED, (unsigned long long)erased);
  }
  if (t < 128) {                                   // the P and Q threads lie in the first two waves
    add_per_wave(counters, K_P_FIXED, pf);
    add_per_wave(counters, K_Q_FIXED, qf);
  }
}

}  // namespace efmsec
}  // namespace ldg
