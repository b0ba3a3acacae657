// EFM (digital audio) run-length extraction from the raw RF.  BUILD-DEFINED (DESIGN.md
// section 7c, row F7; tests/efm_ref.py is the numpy restatement): the snapshot this project
// follows has no EFM path.
//
//   ldg_k_efm_fir    low-pass (255 taps) and decimate by 4 from the raw capture, and the sums
//                    of the 64-sample baseline blocks
//   ldg_k_efm_cross  z = y - baseline, the zero crossings' times, compacted in order (a count
//                    pass, ldg_k_efm_scan over the tiles' counts, a write pass)
//   ldg_k_efm_clock  the clock recovery: one wave per 2^20-sample segment, the chain on lane 0
//   ldg_k_efm_pack   the segments' bytes into one contiguous buffer
//
// FP64 throughout.  Every tile is anchored to a global grid (multiples of 1024 decimated
// samples, of 2^20 samples for the segments) and every value is computed in one fixed
// order, so a result does not depend on how the capture is cut into calls.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "efm_plan.hpp"
#include "sample.hpp"

namespace ldg {
namespace efm {

constexpr int FIR_THREADS = 256;             // four consecutive outputs a thread
constexpr int FIR_SAMPLES = DEC * TILE + NTAPS - 1;   // 4350 capture samples a tile reads
constexpr int FIR_ROW = 273;                 // doubles per LDS row (272 used; odd: rows on different banks)
constexpr int CLOCK_CHUNK = 512;             // crossings staged into LDS at a time

struct SegDev {                              // ldg_efm_seg, then the segment's place in the byte buffers
  int64_t emitted, ignored, clamped_low, clamped_high;
  double final_P;
  int64_t own0;                              // index of its first own crossing: where its bytes start in tmp
  int64_t out_off;                           // where they start in the packed output
};

struct ClockArgs {
  double p0, pmin, pmax, alpha, beta;
};

// y[m] for the TILE values of m from tile * TILE, into y[m - y_off]; the sums of its 16
// blocks into B[b - b_off].  Sample s of the file is raw's sample s - first; samples outside
// [first, first + n) read as 0 (they only feed outputs nobody uses: efm_plan.hpp).
//
// Output u = 4 t + r of thread t reads tile samples 4 u + e, e = 0..254, with tap h[254 - e].
// In LDS, tile sample 4 i + p sits in row (p, i & 3) at column i >> 2: with e = 4 q + p the
// thread reads i = 4 t + (r + q), row (p, (r + q) & 3), column t + ((r + q) >> 2) -- one
// value for its four outputs, consecutive columns over the lanes.
__global__ __launch_bounds__(FIR_THREADS, 2) void ldg_k_efm_fir(const uint8_t* __restrict__ raw, int fmt, int64_t first,
                                                             int64_t n, const double* __restrict__ h,
                                                             int64_t tile0, double* __restrict__ y, int64_t y_off,
                                                             double* __restrict__ B, int64_t b_off) {
  __shared__ double Q[16 * FIR_ROW];
  const int t = threadIdx.x;
  const int64_t tile = tile0 + blockIdx.x;
  const int64_t sb = tile * TILE * DEC - HALF_TAPS - first;      // the tile's first sample, relative to raw
  for (int is = t; is < FIR_SAMPLES; is += FIR_THREADS) {
    const int64_t rel = sb + is;
    const double v = (rel >= 0 && rel < n) ? load_sample(raw, fmt, rel) : 0.0;
    const int p = is & 3, i = is >> 2;
    Q[(p * 4 + (i & 3)) * FIR_ROW + (i >> 2)] = v;
  }
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int p = 0; p < 4; p++) {
#pragma unroll
    for (int c = 0; c < 67; c++) {
      if (4 * (c - 3) + p > NTAPS - 1) continue;                  // no output's tap reaches this far
      const double v = Q[(p * 4 + (c & 3)) * FIR_ROW + t + (c >> 2)];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int e = 4 * (c - r) + p;
        if (c - r >= 0 && e <= NTAPS - 1) acc[r] = __builtin_fma(h[NTAPS - 1 - e], v, acc[r]);
      }
    }
  }
  const int64_t m0 = tile * TILE + 4 * t;
  double2* yo = reinterpret_cast<double2*>(y + (m0 - y_off));    // m0 - y_off is a multiple of 4
  yo[0] = make_double2(acc[0], acc[1]);
  yo[1] = make_double2(acc[2], acc[3]);
  double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);              // a block = 16 consecutive threads
  s += __shfl_xor(s, 8, 16);
  s += __shfl_xor(s, 4, 16);
  s += __shfl_xor(s, 2, 16);
  s += __shfl_xor(s, 1, 16);
  if ((t & 15) == 0) B[tile * BLOCKS_PER_TILE + (t >> 4) - b_off] = s;
}

// exclusive scan of one value per thread over a workgroup of NT threads (sh: NT values)
template <class V, int NT>
__device__ __forceinline__ V wg_scan(V v, V* sh, V* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < NT; off <<= 1) {
    const V x = t >= off ? sh[t - off] : (V)0;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const V incl = sh[t];
  *total = sh[NT - 1];
  __syncthreads();
  return incl - v;
}

// the baseline of block b: the mean of the nine blocks around it (summed in index order)
__device__ __forceinline__ double base_of(const double* __restrict__ B, int64_t b) {
  double s = B[b - 4];
#pragma unroll
  for (int k = -3; k <= 4; k++) s = s + B[b + k];
  return s / (double)((2 * BASE_HALF + 1) * BLOCK);
}

// The crossings between m - 1 and m for the TILE values of m from tile * TILE, four
// consecutive m a thread; z exists for m in [z_lo, z_hi].  WRITE == false: the tile's count.
// WRITE == true: the times at offs[tile] + rank in m order, and (z_out != NULL) z itself.
template <bool WRITE>
__global__ __launch_bounds__(256) void ldg_k_efm_cross(const double* __restrict__ y, int64_t y_off,
                                                       const double* __restrict__ B, int64_t b_off, int64_t z_lo,
                                                       int64_t z_hi, int64_t ctile0, int32_t* __restrict__ counts,
                                                       const int64_t* __restrict__ offs, double* __restrict__ t_out,
                                                       double* __restrict__ z_out) {
  __shared__ int32_t sh[256];
  const int t = threadIdx.x;
  const int64_t m0 = (ctile0 + blockIdx.x) * TILE + 4 * t;
  double z[5];
  bool ok[5];
  const bool any = m0 + 3 >= z_lo && m0 - 1 <= z_hi;
  const int64_t b1 = m0 >> 6, b0 = (m0 - 1) >> 6;
  double base1 = 0.0, base0 = 0.0;
  if (any) {
    if (m0 + 3 >= z_lo && m0 <= z_hi) base1 = base_of(B - b_off, b1);
    base0 = base1;
    if (b0 != b1 && m0 - 1 >= z_lo && m0 - 1 <= z_hi) base0 = base_of(B - b_off, b0);
  }
#pragma unroll
  for (int r = 0; r < 5; r++) {
    const int64_t m = m0 - 1 + r;
    ok[r] = m >= z_lo && m <= z_hi;
    z[r] = ok[r] ? y[m - y_off] - (r == 0 ? base0 : base1) : 0.0;
  }
  double tc[4];
  int cnt = 0;
#pragma unroll
  for (int r = 1; r < 5; r++) {
    const bool cr = ok[r - 1] && ok[r] && ((z[r - 1] < 0.0) != (z[r] < 0.0));
    tc[r - 1] = cr ? (double)DEC * ((double)(m0 + r - 2) + z[r - 1] / (z[r - 1] - z[r])) : -1.0;
    cnt += cr ? 1 : 0;
  }
  int32_t total;
  const int32_t rank = wg_scan<int32_t, 256>(cnt, sh, &total);
  if (!WRITE) {
    if (t == 0) counts[blockIdx.x] = total;
    return;
  }
  int64_t o = offs[blockIdx.x] + rank;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (tc[r] >= 0.0) t_out[o++] = tc[r];
    if (z_out && ok[r + 1]) z_out[m0 + r - z_lo] = z[r + 1];
  }
}

// offs[i] = counts[0] + ... + counts[i - 1]; *total = their sum.  One workgroup of 1024.
__global__ __launch_bounds__(1024) void ldg_k_efm_scan(const int32_t* __restrict__ counts, int64_t n,
                                                       int64_t* __restrict__ offs, int64_t* __restrict__ total) {
  __shared__ int64_t sh[1024];
  int64_t carry = 0;
  for (int64_t i0 = 0; i0 < n; i0 += 1024) {
    const int64_t i = i0 + threadIdx.x;
    const int64_t v = i < n ? counts[i] : 0;
    int64_t sum;
    const int64_t ex = wg_scan<int64_t, 1024>(v, sh, &sum);
    if (i < n) offs[i] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

// the first index i in [0, n) with t[i] >= v (n when none): t ascends
__device__ __forceinline__ int64_t lower_bound(const double* __restrict__ t, int64_t n, double v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (t[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Clock recovery of segment seg0 + blockIdx.x: one wave.  Its run starts at the first
// crossing at or after the segment's start less RUNIN (segment 0: the first crossing) and
// ends before the next segment's start; crossings from the segment's start on are its own and
// emit.  Lane 0 runs the chain in the restatement's operation order (IEEE division, no
// contraction); the wave stages CLOCK_CHUNK crossing times into LDS ahead of it and stores
// the chunk's bytes behind it, at tmp[own0 + k] for the segment's k-th byte (a segment emits
// at most one byte per own crossing, so the segments' ranges in tmp do not overlap).
__global__ __launch_bounds__(64) void ldg_k_efm_clock(const double* __restrict__ tx, const int64_t* __restrict__ ncross,
                                                      int64_t seg0, ClockArgs A, uint8_t* __restrict__ tmp,
                                                      SegDev* __restrict__ segs) {
#pragma clang fp contract(off)
  __shared__ double ts[CLOCK_CHUNK];
  __shared__ uint8_t ob[CLOCK_CHUNK];
  __shared__ int s_ne;
  prio_latency();
  const int lane = threadIdx.x;
  const int64_t j = seg0 + blockIdx.x;
  const int64_t n = *ncross;
  const double lo = (double)(j * SEG), hi = (double)((j + 1) * SEG);
  const int64_t i0 = j == 0 ? 0 : lower_bound(tx, n, lo - (double)RUNIN);
  const int64_t i1 = lower_bound(tx, n, hi);
  const int64_t own0 = lower_bound(tx, n, lo);
  double P = A.p0, ref = 0.0;
  int64_t emitted = 0, ignored = 0, cl = 0, ch = 0;
  if (i0 < i1) ref = tx[i0];
  for (int64_t c0 = i0 + 1; c0 < i1; c0 += CLOCK_CHUNK) {
    const int m = (int)(i1 - c0 < CLOCK_CHUNK ? i1 - c0 : CLOCK_CHUNK);
    for (int k = lane; k < m; k += 64) ts[k] = tx[c0 + k];
    __syncthreads();
    if (lane == 0) {
      int ne = 0;
      for (int k = 0; k < m; k++) {
        const double c = ts[k];
        const double d = c - ref;
        const double nd = floor(d / P + 0.5);
        const bool own = c >= lo;
        if (nd < 1.0) {
          ignored += own ? 1 : 0;
          continue;
        }
        const double e = d - nd * P;
        ref = (ref + nd * P) + A.alpha * e;
        P = fmin(fmax(P + (A.beta * e) / nd, A.pmin), A.pmax);
        if (own) {
          cl += nd < 3.0 ? 1 : 0;
          ch += nd > 11.0 ? 1 : 0;
          ob[ne++] = (uint8_t)(nd < 3.0 ? 3.0 : (nd > 11.0 ? 11.0 : nd));
        }
      }
      s_ne = ne;
    }
    __syncthreads();
    const int ne = s_ne;
    for (int k = lane; k < ne; k += 64) tmp[own0 + emitted + k] = ob[k];
    emitted += ne;                           // (every lane keeps the count)
    __syncthreads();
  }
  if (lane == 0) {
    SegDev& s = segs[blockIdx.x];
    s.emitted = emitted;
    s.ignored = ignored;
    s.clamped_low = cl;
    s.clamped_high = ch;
    s.final_P = P;
    s.own0 = own0;
  }
}

// out_off of each segment (the bytes before it) and the total; one thread: a call has a few
// thousand segments at the most
__global__ void ldg_k_efm_offsets(SegDev* __restrict__ segs, int64_t nseg, int64_t* __restrict__ total) {
  if (threadIdx.x || blockIdx.x) return;
  int64_t o = 0;
  for (int64_t i = 0; i < nseg; i++) {
    segs[i].out_off = o;
    o += segs[i].emitted;
  }
  *total = o;
}

// segment blockIdx.x's bytes from tmp to their place in out (cap: out's size; the host reports
// an output that does not fit)
__global__ __launch_bounds__(256) void ldg_k_efm_pack(const SegDev* __restrict__ segs, const uint8_t* __restrict__ tmp,
                                                      uint8_t* __restrict__ out, int64_t cap) {
  const SegDev s = segs[blockIdx.x];
  for (int64_t k = (int64_t)blockIdx.y * 256 + threadIdx.x; k < s.emitted; k += (int64_t)gridDim.y * 256)
    if (s.out_off + k < cap) out[s.out_off + k] = tmp[s.own0 + k];
}

}  // namespace efm
}  // namespace ldg
