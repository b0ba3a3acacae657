// NTSC line services: the white flag (field row 10), the video ID (row 19) and the closed
// captions (row 20) of a field, from the uint16 pixels of the one row.
// BUILD-DEFINED (tests/lines_ref.py is the numpy restatement): the
// snapshot this project follows decodes none of them.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "field_rec.hpp"

namespace ldg {

using LineRec = ldg_line_services;
static_assert(sizeof(LineRec) == LDG_LINE_SERVICES_SIZE, "ldg_line_services has the size the header states");

constexpr int LS_W = 910;                      // pixels of an NTSC .tbc row
constexpr int LS_ROWS = 21;                    // field rows the services need (0..20)
constexpr int LS_ROW_WHITE = 10, LS_ROW_VID = 19, LS_ROW_CC = 20;
// u16 = 1024 + (IRE + 40) * 358.4
constexpr int LS_T25 = 24320, LS_T35 = 27904, LS_T50 = 33280;
enum LineService { LS_WHITE = 0, LS_CC = 1, LS_VID = 2, LS_SERVICES = 3 };

namespace {

__device__ __forceinline__ int ls_wave_min(int v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const int w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}

__device__ __forceinline__ int ls_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The smallest x in [lo, hi) with p[x] > T and p[x - q .. x - 1] all <= T, or -1: each lane
// tests the candidates lo + lane, lo + lane + 64, ... (lo - q >= 2 at every call).
__device__ __forceinline__ int ls_first_rise(const uint16_t* p, int T, int lo, int hi, int q, int lane) {
  int best = LS_W;
  for (int x = lo + lane; x < hi && best == LS_W; x += 64) {
    if (p[x] <= T) continue;
    bool quiet = true;
    for (int k = 1; k <= q; k++) quiet &= p[x - k] <= T;
    if (quiet) best = x;
  }
  best = ls_wave_min(best);
  return best < LS_W ? best : -1;
}

// A cell at centre c (4 <= c < LS_W - 4) reads 1 iff the nine pixels about it sum above 9 T.
__device__ __forceinline__ bool ls_cell(const uint16_t* p, int c, int T) {
  int s = 0;
#pragma unroll
  for (int k = -4; k <= 4; k++) s += p[c + k];
  return s > 9 * T;
}

}  // namespace

// grid: (LS_SERVICES, n fields) x 64 threads, one wave per (field, service); the wave stages
// its row in LDS.  Field e's row r lies at
//   smap != NULL (read slots):   base + smap[e] * entry_stride + r * LS_W, valid as recs[smap[e]] says;
//   smap == NULL (packed frames): base + (e >> 1) * entry_stride + (2 r + (e & 1)) * LS_W, always valid.
// Lane 0 writes the service's members of out[e]; the three waves of a field write disjoint members.
extern "C" __global__ __launch_bounds__(64) void ldg_k_line_services(const uint16_t* __restrict__ base,
                                                                      int64_t entry_stride,
                                                                      const int32_t* __restrict__ smap,
                                                                      const FieldRec* __restrict__ recs,
                                                                      LineRec* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint16_t p[LS_W + 2];
  const int lane = threadIdx.x;
  const int svc = blockIdx.x, e = blockIdx.y;
  LineRec* o = out + e;
  bool valid = true;
  const uint16_t* field;
  int row_stride;
  if (smap) {
    const int slot = smap[e];
    valid = recs[slot].status == FS_VALID && recs[slot].linecount >= LS_ROWS;
    field = base + (int64_t)slot * entry_stride;
    row_stride = LS_W;
  } else {
    field = base + (int64_t)(e >> 1) * entry_stride + (e & 1) * LS_W;
    row_stride = 2 * LS_W;
  }
  if (!valid) {
    if (lane == 0) {
      if (svc == LS_WHITE) {
        o->white_count = -1;
        o->white_flag = 0;
      } else if (svc == LS_CC) {
        o->cc_state = LDG_LINE_ABSENT;
        o->cc_runin = 0;
        o->cc_x = -1;
        o->cc[0] = o->cc[1] = o->pad_[0] = o->pad_[1] = 0;
      } else {
        o->vid_state = LDG_LINE_ABSENT;
        o->vid_x = -1;
        o->vid_bits = 0;
      }
    }
    return;
  }
  const int r = svc == LS_WHITE ? LS_ROW_WHITE : (svc == LS_CC ? LS_ROW_CC : LS_ROW_VID);
  const uint16_t* src = field + (int64_t)r * row_stride;
  if (((uintptr_t)src & 3) == 0) {
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* p32 = reinterpret_cast<uint32_t*>(p);
    for (int x = lane; x < LS_W / 2; x += 64) p32[x] = s32[x];
  } else {
    for (int x = lane; x < LS_W; x += 64) p[x] = src[x];
  }
  __syncthreads();

  if (svc == LS_WHITE) {
    int c = 0;
    for (int x = 100 + lane; x < 780; x += 64) c += p[x] > LS_T50;
    c = ls_wave_sum(c);
    if (lane == 0) {
      o->white_count = c;
      o->white_flag = 2 * c > 680;
    }
  } else if (svc == LS_CC) {
    const int xs = ls_first_rise(p, LS_T25, 270, 410, 40, lane);
    int state = LDG_LINE_ABSENT, runin = 0;
    unsigned bits = 0;
    if (xs >= 0) {
      const int lo = xs - 279 > 3 ? xs - 279 : 3;
      for (int x = lo + lane; x < xs - 40; x += 64) runin += p[x] > LS_T25 && p[x - 1] <= LS_T25;
      runin = ls_wave_sum(runin);
      // bit i at centre (32 xs + (3 + 2 i) 455) >> 5 <= 409 + 469 (lanes past 15 read bit 15's cell)
      const int i = lane < 16 ? lane : 15;
      const bool b = ls_cell(p, (32 * xs + (3 + 2 * i) * 455) >> 5, LS_T25);
      bits = (unsigned)(__ballot(b && lane < 16) & 0xffffu);
      const bool odd = (__popc(bits & 0xffu) & 1) && (__popc(bits >> 8) & 1);
      state = (runin < 6 || runin > 8) ? LDG_LINE_FRAME : (odd ? LDG_LINE_OK : LDG_LINE_CHECK);
    }
    if (lane == 0) {
      o->cc_state = state;
      o->cc_runin = runin;
      o->cc_x = xs;
      o->cc[0] = (uint8_t)(bits & 0xffu);
      o->cc[1] = (uint8_t)(bits >> 8);
      o->pad_[0] = o->pad_[1] = 0;
    }
  } else {
    const int xr = ls_first_rise(p, LS_T35, 60, 160, 20, lane);
    int state = LDG_LINE_ABSENT, vbits = 0;
    if (xr >= 0) {
      // cell j at centre xr + 16 + 32 j <= 159 + 688
      const int j = lane < 22 ? lane : 21;
      const bool b = ls_cell(p, xr + 16 + 32 * j, LS_T35);
      const unsigned m = (unsigned)(__ballot(b && lane < 22) & 0x3fffffu);
      int reg = 0x3f;
      for (int k = 2; k < 22; k++) {                 // cell 2 first: bit 19
        const int bit = (m >> k) & 1;
        vbits = (vbits << 1) | bit;
        const int fb = ((reg >> 5) & 1) ^ bit;
        reg = ((reg << 1) & 0x3f) ^ (fb ? 3 : 0);
      }
      state = (m & 3u) != 1u ? LDG_LINE_FRAME : (reg == 0 ? LDG_LINE_OK : LDG_LINE_CHECK);
    }
    if (lane == 0) {
      o->vid_state = state;
      o->vid_x = xr;
      o->vid_bits = vbits;
    }
  }
}

}  // namespace ldg
