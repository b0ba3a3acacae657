// RF dropout detection per field row and concealment on the assembled frame.
// BUILD-DEFINED (tests/dropout_ref.py is the numpy restatement):
// the snapshot this project follows has no dropout handling.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "field_rec.hpp"
#include "pyops.hpp"

namespace ldg {

constexpr int MAX_DROPOUTS = LDG_MAX_DROPOUTS_PER_LINE;
// per entry (a read slot, or a field of a frame being assembled):
//   runs   int16 [MAX_LINES][MAX_DROPOUTS][2]  (startx, endx) of each row's runs
//   counts int32 [MAX_LINES]                   runs of each row
//   nrows  int32                               the field's linecount, -1: field not valid
constexpr int DROP_RUNS_STRIDE = MAX_LINES * MAX_DROPOUTS * 2;

struct DropParams {
  double lo_hz, hi_hz;
  int32_t merge_gap, min_flagged, pad, pad_;
};

// The wave-uniform state of one row's walk: the open raw run, the last padded run (a
// later one may still merge into it), and the pixel runs so far (run k lives in lane k).
struct DropWalk {
  int64_t a = 0, b = 0;       // open raw run [a, b], absolute sample indices
  int cnt = 0;                // its flagged samples (0: none open)
  int64_t pa = 0, pb = -1;    // pending padded run (pb < pa: none)
  int n = 0;                  // pixel runs
  int last_ex = 0;            // endx of run n - 1
  int sx = 0, ex = 0;         // this lane's run (lane < n)
};

// grid: (frame_lines / 2 + 1 rows, n entries) x 64 threads, one wave per (entry, row) as
// ldg_k_final_lines sizes its grid.  Reads demod[ib .. ie) of the slot's CH_DEMOD channel
// 64 samples a step (four steps' loads in flight), one ballot per step; runs are formed
// by bit scans over the masks.  by_slot: the output entry is the slot (ldg_field_dropouts)
// instead of the position in smap (frame assembly: entry 2 f + parity).
extern "C" __global__ __launch_bounds__(64) void ldg_k_dropout_lines(
    const int32_t* __restrict__ smap, int by_slot, const double* __restrict__ video, int64_t vread_stride,
    int64_t vchan_stride, SysConst C, const FieldRec* __restrict__ recs, const double* __restrict__ lines,
    DropParams P, int16_t* __restrict__ runs, int32_t* __restrict__ counts, int32_t* __restrict__ nrows) {
  const int lane = threadIdx.x;
  const int slot = smap[blockIdx.y];
  const int entry = by_slot ? slot : (int)blockIdx.y;
  const int row = blockIdx.x;
  const FieldRec* R = recs + slot;
  const bool valid = R->status == FS_VALID;
  const int lc = valid ? R->linecount : -1;
  if (row == 0 && lane == 0) nrows[entry] = lc;
  if (row >= lc) return;
  const int l = row + ((C.system == 1) ? 3 : 1);
  int32_t* cnt_out = counts + (int64_t)entry * MAX_LINES + row;
  if (l + 1 >= MAX_LINES) {
    if (lane == 0) *cnt_out = 0;
    return;
  }
  const double* lf = lines + (int64_t)slot * LINES_STRIDE + LLF * MAX_LINES;
  const double begin = lf[l], end = lf[l + 1];
  const int64_t ib = py_int(begin), ie = py_int(end);
  // (a valid field's rows passed these checks in the final resample)
  if (!(ib >= 0 && ie > ib && ie <= R->n_out && ie - ib < (1 << 20))) {
    if (lane == 0) *cnt_out = 0;
    return;
  }
  const double* dm = video + (int64_t)slot * vread_stride + (int64_t)CH_DEMOD * vchan_stride;
  const int W = C.outlinelen;
  const double sc = (double)W / (end - begin);
  DropWalk S;

  auto flush_pending = [&]() {
    if (S.pb < S.pa) return;
    const double fs = floor(((double)S.pa - begin) * sc);
    const double fe = ceil(((double)(S.pb + 1) - begin) * sc);
    const int sx = fs > 0.0 ? (int)fs : 0;
    const int ex = fe < (double)W ? (int)fe : W;
    if (S.n > 0 && sx <= S.last_ex) {
      if (ex > S.last_ex) S.last_ex = ex;
    } else if (S.n < MAX_DROPOUTS) {
      if (lane == S.n) S.sx = sx;
      S.n++;
      S.last_ex = ex;
    } else if (ex > S.last_ex) {
      S.last_ex = ex;           // a ninth or later run extends the eighth
    }
    if (lane == S.n - 1) S.ex = S.last_ex;
    S.pb = S.pa - 1;
  };
  auto close_raw = [&]() {
    if (S.cnt >= P.min_flagged) {
      int64_t a = S.a - P.pad, b = S.b + P.pad;
      if (a < ib) a = ib;
      if (b > ie - 1) b = ie - 1;
      if (S.pb >= S.pa && a <= S.pb + 1) {
        if (b > S.pb) S.pb = b;
      } else {
        flush_pending();
        S.pa = a;
        S.pb = b;
      }
    }
    S.cnt = 0;
  };

  constexpr int UN = 4;
  for (int64_t j0 = ib; j0 < ie; j0 += 64 * UN) {
    double v[UN];
#pragma unroll
    for (int u = 0; u < UN; u++) {
      const int64_t j = j0 + 64 * u + lane;
      v[u] = j < ie ? dm[j] : P.lo_hz;
    }
#pragma unroll
    for (int u = 0; u < UN; u++) {
      const int64_t base = j0 + 64 * u;
      const bool flag = (base + lane < ie) && !(P.lo_hz <= v[u] && v[u] <= P.hi_hz);
      uint64_t m = __ballot(flag);
      while (m) {
        const int first = __ffsll((unsigned long long)m) - 1;
        const uint64_t rest = ~(m >> first);               // zeros where the ones continue
        const int len = rest ? __ffsll((unsigned long long)rest) - 1 : 64 - first;
        const int64_t j = base + first;
        if (S.cnt > 0 && j - S.b > P.merge_gap) close_raw();
        if (S.cnt == 0) S.a = j;
        S.b = j + len - 1;
        S.cnt += len;
        m = (first + len >= 64) ? 0 : (m >> (first + len)) << (first + len);
      }
    }
  }
  close_raw();
  flush_pending();
  if (lane == 0) *cnt_out = S.n;
  if (lane < S.n) {
    int16_t* o = runs + (int64_t)entry * DROP_RUNS_STRIDE + ((int64_t)row * MAX_DROPOUTS + lane) * 2;
    o[0] = (int16_t)S.sx;
    o[1] = (int16_t)S.ex;
  }
}

// Concealment of the assembled frames in place.  grid: (frame_lines, n frames) x 64
// threads, one wave per frame row.  Entry 2 f + p holds the runs of frame f's field of
// parity p (0 top, 1 bottom).  A run [startx, endx) of field row r is copied from the first
// of the rows r - d, r + d, r - 2 d, r + 2 d of the same field that is a picture row of
// the frame (below 2 min(lt, lb) and below frame_lines) and has no run of its own over the
// range: a source is never written, so the copy in place has no read-after-write hazard
// between workgroups.
extern "C" __global__ __launch_bounds__(64) void ldg_k_conceal(const int16_t* __restrict__ runs,
                                                                const int32_t* __restrict__ counts,
                                                                const int32_t* __restrict__ nrows, SysConst C,
                                                                uint16_t* frames) {
  const int lane = threadIdx.x;
  const int f = blockIdx.y, frow = blockIdx.x;
  const int p = frow & 1, r = frow >> 1;
  const int lt = nrows[2 * f], lb = nrows[2 * f + 1];
  const int m = lt < lb ? lt : lb;                       // picture rows per field of this frame
  const bool pal = C.system == 1;
  const int first_row = pal ? LDG_CONCEAL_FIRST_ROW_PAL : LDG_CONCEAL_FIRST_ROW_NTSC;
  if (r < first_row || r >= m) return;
  const int entry = 2 * f + p;
  const int32_t* cnt = counts + (int64_t)entry * MAX_LINES;
  const int16_t* rr = runs + (int64_t)entry * DROP_RUNS_STRIDE;
  int n = cnt[r];
  if (n <= 0) return;
  if (n > MAX_DROPOUTS) n = MAX_DROPOUTS;
  const int W = C.outlinelen;
  const int d = pal ? 4 : 2;
  uint16_t* fr = frames + (int64_t)f * C.frame_lines * W;
  for (int k = 0; k < n; k++) {
    const int sx = rr[(r * MAX_DROPOUTS + k) * 2], ex = rr[(r * MAX_DROPOUTS + k) * 2 + 1];
    int src = -1;
    for (int q = 0; q < 4 && src < 0; q++) {
      const int c = r + ((q & 1) ? d : -d) * (1 + (q >> 1));
      if (c < first_row || c >= m || 2 * c + p >= C.frame_lines) continue;
      int nc = cnt[c];
      if (nc > MAX_DROPOUTS) nc = MAX_DROPOUTS;
      bool hit = false;
      for (int t = 0; t < nc; t++) {
        const int cs = rr[(c * MAX_DROPOUTS + t) * 2], ce = rr[(c * MAX_DROPOUTS + t) * 2 + 1];
        hit |= cs < ex && sx < ce;
      }
      if (!hit) src = c;
    }
    if (src < 0) continue;
    int x0 = sx, x1 = ex;
    if (!pal && x0 < 2) x0 = 2;                          // pixels 0, 1: the burst flag pixels
    if (x0 < 0) x0 = 0;
    if (x1 > W) x1 = W;
    if (x0 >= x1) continue;
    uint16_t* dst = fr + (int64_t)(2 * r + p) * W;
    const uint16_t* s = fr + (int64_t)(2 * src + p) * W;
    // the two rows lie an even number of rows apart: the same 32-bit alignment
    const bool same = (((uintptr_t)(dst + x0) ^ (uintptr_t)(s + x0)) & 2) == 0;
    if (same) {
      int xa = x0 + (int)(((uintptr_t)(dst + x0) >> 1) & 1);        // first 32-bit aligned pixel
      if (xa > x1) xa = x1;
      const int nw = (x1 - xa) / 2;
      if (lane == 0 && xa > x0) dst[x0] = s[x0];
      uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + xa);
      const uint32_t* s32 = reinterpret_cast<const uint32_t*>(s + xa);
      for (int x = lane; x < nw; x += 64) d32[x] = s32[x];
      if (lane == 0 && xa + 2 * nw < x1) dst[x1 - 1] = s[x1 - 1];
    } else {
      for (int x = x0 + lane; x < x1; x += 64) dst[x] = s[x];
    }
  }
}

}  // namespace ldg
