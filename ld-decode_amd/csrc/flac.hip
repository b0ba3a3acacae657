// FLAC-compressed captures (.ldf, .flac, .oga): the candidate scan, the frame walk / decode and the
// placement.  BUILD-DEFINED (tests/flac_ref.py is the Python restatement the
// device equals byte for byte).  One lane walks one frame: the bit stream is serial inside a frame and
// frames are independent, so a chunk's thousands of frames are the parallelism.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "flac_plan.hpp"

namespace ldg {
namespace flac {

static_assert(sizeof(ldg_flac_info) == LDG_FLAC_INFO_SIZE, "ldg_flac_info has the size the header states");
static_assert(sizeof(ldg_flac_counters) == LDG_FLAC_COUNTERS_SIZE, "ldg_flac_counters has the size the header states");
static_assert(sizeof(ldg_flac_frame) == LDG_FLAC_FRAME_SIZE, "ldg_flac_frame has the size the header states");
static_assert(sizeof(Frame) == sizeof(ldg_flac_frame), "the keeper's frames are copied out as they are");

// one candidate for the walk: the frame begins at byte off of the staged bytes and may not read at or
// past byte limit; exact: it must end at limit (an Ogg packet)
struct Job {
  int64_t off, limit;
  int32_t bs, hdr, exact, pad_;
};
enum { ST_REJECT = 0, ST_PARSED = 1, ST_RANGE = 2, ST_ACCEPT = 3 };
struct Res {
  int32_t state, nbytes;
};
// where the placement puts the samples of a decode slot
struct PlaceRec {
  int64_t pos;
  int32_t bs, ok;
};

constexpr int SCAN_COUNTS = 2;       // sync matches, valid headers

// (a) One thread tests one byte offset of [lo, hi): the sync, then the header with its CRC-8 (R1, R2).
// The offsets of the valid headers go to `out` (wave-compacted; the host sorts the waves' runs),
// at most cap of them: counts[1] says how many there were.
__global__ void __launch_bounds__(256) ldg_k_flac_scan(const uint8_t* __restrict__ b, int64_t lo, int64_t hi, int64_t end,
                                                       int bps, int max_bs, uint32_t* __restrict__ out, uint32_t cap,
                                                       uint32_t* __restrict__ counts) {
  const int64_t c = lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool sync = false, ok = false;
  if (c < hi && c + 1 < end) {
    sync = b[c] == 0xff && (b[c + 1] & 0xfe) == 0xf8;
    if (sync) {
      Header h;
      ok = parse_header(b, c, end, bps, max_bs, &h);
    }
  }
  const uint64_t ms = __ballot(sync);
  if (ms == 0) return;
  const uint64_t mo = __ballot(ok);
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((unsigned long long)ms) - 1;
  uint32_t base = 0;
  if (lane == leader) {
    atomicAdd(&counts[0], (uint32_t)__popcll(ms));
    if (mo) base = atomicAdd(&counts[1], (uint32_t)__popcll(mo));
  }
  base = __shfl(base, leader);
  if (ok) {
    const uint32_t i = base + (uint32_t)__popcll(mo & ((1ull << lane) - 1));
    if (i < cap) out[i] = (uint32_t)c;
  }
}

namespace {

// A lane's view of the staged bytes as a big-endian bit stream: two 64-bit words in registers, one
// aligned load for every 64 bits consumed.  No read reaches bit `lim` or the words past nw.
struct Bits {
  const uint64_t* w;
  int64_t nw, p, lim, wi;
  uint64_t cur, nxt;
  __device__ __forceinline__ uint64_t ld(int64_t i) const { return (i >= 0 && i < nw) ? __builtin_bswap64(w[i]) : 0; }
  __device__ __forceinline__ void init(const uint64_t* w_, int64_t nw_, int64_t p0, int64_t lim_) {
    w = w_;
    nw = nw_;
    p = p0;
    lim = lim_;
    wi = p >> 6;
    cur = ld(wi);
    nxt = ld(wi + 1);
  }
  __device__ __forceinline__ uint64_t window() const {
    const int o = (int)(p & 63);
    return o ? (cur << o) | (nxt >> (64 - o)) : cur;
  }
  __device__ __forceinline__ void advance(int n) {      // n <= 64
    p += n;
    if ((p >> 6) != wi) {
      wi++;
      cur = nxt;
      nxt = ld(wi + 1);
    }
  }
  __device__ __forceinline__ bool read(int n, uint32_t* v) {      // n <= 32
    if (p + n > lim) return false;
    *v = n ? (uint32_t)(window() >> (64 - n)) : 0u;
    advance(n);
    return true;
  }
  __device__ __forceinline__ bool sread(int n, int64_t* v) {
    uint32_t u;
    if (!read(n, &u)) return false;
    *v = n ? (int64_t)((int32_t)(u << (32 - n)) >> (32 - n)) : 0;
    return true;
  }
  // zeros, then a one
  __device__ __forceinline__ bool unary(uint32_t* q) {
    uint32_t z = 0;
    for (;;) {
      if (p >= lim) return false;
      const uint64_t x = window();
      if (x) {
        const int k = __clzll((long long)x);
        if (p + k + 1 > lim) return false;
        advance(k + 1);
        *q = z + (uint32_t)k;
        return true;
      }
      if (p + 64 >= lim) return false;      // nothing but zeros up to the bound
      advance(64);
      z += 64;
    }
  }
};

}  // namespace

// (b) One lane walks one candidate: the subframe (R3), the arithmetic (R4), the padding and the
// CRC-16.  EMIT: the samples go to scratch[i * nslots + job] (int32: lanes of a wave store side by
// side), for the placement; without it nothing but the verdict leaves the lane.
template <bool EMIT>
__global__ void __launch_bounds__(64) ldg_k_flac_walk(const uint64_t* __restrict__ words, int64_t nw,
                                                      const Job* __restrict__ jobs, int njobs, int bps,
                                                      Res* __restrict__ res, int32_t* __restrict__ scratch, int nslots) {
  __shared__ uint16_t T[256];
  for (int i = threadIdx.x; i < 256; i += 64) {
    uint32_t c = (uint32_t)i << 8;
    for (int k = 0; k < 8; k++) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xffff : (c << 1) & 0xffff;
    T[i] = (uint16_t)c;
  }
  __syncthreads();
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= njobs) return;
  const Job J = jobs[j];
  Res R{ST_REJECT, 0};
  const int bs = J.bs;
  const int64_t lo = -(1ll << (bps - 1)), hi = (1ll << (bps - 1)) - 1;
  bool range = false;
  int wasted = 0;
  Bits B;
  B.init(words, nw, 8 * (J.off + J.hdr), 8 * J.limit);

  auto put = [&](int i, int64_t v) {
    const int64_t s = (int64_t)((uint64_t)v << wasted);
    range |= s < lo || s > hi;
    if (EMIT) scratch[(size_t)i * nslots + j] = (int32_t)s;
  };

  do {
    uint32_t u;
    if (!B.read(8, &u) || (u & 0x80)) break;
    const int typ = (u >> 1) & 63;
    if (u & 1) {
      uint32_t q;
      if (!B.unary(&q)) break;
      if (q + 1 >= (uint32_t)bps) break;
      wasted = (int)q + 1;
    }
    const int eff = bps - wasted;
    bool ok = true;
    if (typ == 0) {
      int64_t v;
      if (!B.sread(eff, &v)) break;
      for (int i = 0; i < bs; i++) put(i, v);
    } else if (typ == 1) {
      for (int i = 0; i < bs; i++) {
        int64_t v;
        if (!B.sread(eff, &v)) { ok = false; break; }
        put(i, v);
      }
      if (!ok) break;
    } else {
      int order;
      if (typ >= 8 && typ <= 12) order = typ - 8;
      else if (typ >= 32) order = typ - 31;
      else break;
      if (order > bs) break;
      int64_t hist[32];
      int32_t coef[32];
      for (int i = 0; i < order; i++) {
        int64_t v;
        if (!B.sread(eff, &v)) { ok = false; break; }
        hist[i & 31] = v;
        put(i, v);
      }
      if (!ok) break;
      int shift = 0;
      if (typ >= 32) {
        uint32_t pr;
        int64_t sh;
        if (!B.read(4, &pr) || pr == 15 || !B.sread(5, &sh) || sh < 0) break;
        shift = (int)sh;
        for (int i = 0; i < order; i++) {
          int64_t cf;
          if (!B.sread((int)pr + 1, &cf)) { ok = false; break; }
          coef[i] = (int32_t)cf;
        }
        if (!ok) break;
      } else {
        const int32_t fx[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
        for (int i = 0; i < 4; i++) coef[i] = fx[order][i];
      }
      uint32_t method, po;
      if (!B.read(2, &method) || method > 1 || !B.read(4, &po)) break;
      if (!((po == 0 || (bs & ((1 << po) - 1)) == 0) && (bs >> po) >= order)) break;
      const int kb = method ? 5 : 4;
      const uint32_t esc = method ? 31u : 15u;
      int i = order;
      for (uint32_t p = 0; p < (1u << po) && ok; p++) {
        const int cnt = (bs >> po) - (p == 0 ? order : 0);
        uint32_t k, n = 0;
        if (!B.read(kb, &k)) { ok = false; break; }
        const bool raw = k == esc;
        if (raw && !B.read(5, &n)) { ok = false; break; }
        for (int t = 0; t < cnt; t++, i++) {
          int64_t r;
          if (raw) {
            if (!B.sread((int)n, &r)) { ok = false; break; }
          } else {
            uint32_t q, low;
            if (!B.unary(&q) || !B.read((int)k, &low)) { ok = false; break; }
            const uint64_t uu = ((uint64_t)q << k) | low;
            r = (int64_t)(uu >> 1) ^ -(int64_t)(uu & 1);
          }
          uint64_t sum = 0;
          for (int jj = 0; jj < order; jj++) sum += (uint64_t)(int64_t)coef[jj] * (uint64_t)hist[(i - 1 - jj) & 31];
          const int64_t s = (int64_t)((uint64_t)r + (uint64_t)((int64_t)sum >> shift));
          hist[i & 31] = s;
          put(i, s);
        }
      }
      if (!ok) break;
    }
    const int64_t end = (B.p + 7) >> 3;
    if (end + 2 > J.limit) break;
    if (J.exact && end + 2 != J.limit) break;
    R.nbytes = (int32_t)(end + 2 - J.off);
    // the CRC-16 of [off, end)
    uint32_t crc = 0;
    for (int64_t a = J.off; a < end;) {
      const uint64_t wd = B.ld(a >> 3);
      const int b0 = (int)(a & 7);
      const int nb = (int)((end - a) < (8 - b0) ? (end - a) : (8 - b0));
      for (int t = 0; t < nb; t++) {
        const uint32_t x = (uint32_t)(wd >> (56 - 8 * (b0 + t))) & 0xff;
        crc = ((crc << 8) & 0xffff) ^ T[(crc >> 8) ^ x];
      }
      a += nb;
    }
    const uint32_t s0 = (uint32_t)(B.ld(end >> 3) >> (56 - 8 * (end & 7))) & 0xff;
    const uint32_t s1 = (uint32_t)(B.ld((end + 1) >> 3) >> (56 - 8 * ((end + 1) & 7))) & 0xff;
    R.state = crc != (s0 << 8 | s1) ? ST_PARSED : range ? ST_RANGE : ST_ACCEPT;
  } while (false);
  res[j] = R;
}

// (c) The decode slots' samples into the output at their positions, clipped to the window
// [first, first + n), in the stream's sample format.  A 64 x 64 tile through LDS turns the walk's
// slot-major stores into sample-major ones.
__global__ void __launch_bounds__(256) ldg_k_flac_place(const int32_t* __restrict__ scratch, int nslots,
                                                        const PlaceRec* __restrict__ recs, int nrec, int64_t first,
                                                        int64_t n, int bps, void* __restrict__ dst) {
  __shared__ int32_t tile[64][65];
  const int i0 = blockIdx.x * 64, s0 = blockIdx.y * 64, t = threadIdx.x;
  for (int r = 0; r < 16; r++) {
    const int i = r * 4 + (t >> 6), s = t & 63;
    if (s0 + s < nrec && i0 + i < recs[s0 + s].bs) tile[i][s] = scratch[(size_t)(i0 + i) * nslots + s0 + s];
  }
  __syncthreads();
  for (int r = 0; r < 16; r++) {
    const int s = r * 4 + (t >> 6), i = t & 63;
    if (s0 + s >= nrec) continue;
    const PlaceRec rec = recs[s0 + s];
    if (!rec.ok || i0 + i >= rec.bs) continue;
    const int64_t g = rec.pos + i0 + i - first;
    if (g < 0 || g >= n) continue;
    const int32_t v = tile[i][s];
    if (bps == 16) ((int16_t*)dst)[g] = (int16_t)v;
    else ((uint8_t*)dst)[g] = (uint8_t)(v + 128);
  }
}

}  // namespace flac
}  // namespace ldg
