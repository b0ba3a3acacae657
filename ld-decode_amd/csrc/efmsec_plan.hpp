// EFM data sectors: what a call may emit from the bytes it holds and
// what the next call has to see again, so that the result does not depend on how the stream
// is cut into calls.  Plain C++ (no device, no HIP): efmsec.hip calls sectors_of / finish from
// its kernels, efmsec.inc carries the state between calls with them, and
// tests/san/efmsec_san.cpp runs all of it under the sanitizers.  The shape is
// efmdec_plan.hpp's, over byte indices instead of channel bits.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define LDG_EFMSEC_HD __host__ __device__
#else
#define LDG_EFMSEC_HD
#endif

namespace ldg {
namespace efmsec {

constexpr int64_t SECTOR = 2352;
constexpr int64_t SYNC_BYTES = 12;               // 00 FF x 10 00
constexpr int64_t MAX_COAST = 75;                // sectors between two confirmed headers, at the most
// a candidate at c is settled once a candidate at c + 2352 would be held whole
constexpr int64_t SETTLE = SECTOR + SYNC_BYTES;
// floor(d / 2352 + 0.5) > 75 from this d on
constexpr int64_t BREAK_BYTES = (2 * MAX_COAST + 1) * SECTOR / 2;
constexpr int64_t NEVER = INT64_MAX;

// What a call's header search may decide.  Positions are byte indices from the stream's
// first byte.  Candidates above `lim` are not settled (final call: all are); candidates below
// `emit_from` were dealt with by an earlier call and are held only to confirm others.
struct Window {
  int64_t emit_from;
  int64_t lim;       // E - SETTLE, or NEVER in the final call
  int64_t end;       // E: the index one past the last byte held
  int32_t final_;
};

// Sectors confirmed candidate k of conf[0 .. nconf) starts in this call; *brk: a break was
// counted.  Every sector returned lies wholly below w.end.
LDG_EFMSEC_HD inline int64_t sectors_of(const int64_t* conf, int64_t nconf, int64_t k, const Window& w, int* brk) {
  *brk = 0;
  const int64_t a = conf[k];
  if (a < w.emit_from) return 0;
  int64_t n;
  if (k + 1 < nconf && (w.final_ || conf[k + 1] <= w.lim)) {
    n = (2 * (conf[k + 1] - a) + SECTOR) / (2 * SECTOR);
    if (n > MAX_COAST) {
      n = 1;
      *brk = 1;
    }
  } else if (w.final_) {
    n = 1;                                        // the last confirmed candidate
  } else if (a <= w.lim && w.lim - a >= BREAK_BYTES) {
    n = 1;                                        // whatever follows is a break: finish() moves on
  } else {
    n = 0;                                        // the next call's
  }
  const int64_t room = w.end - SECTOR - a;        // sectors a + 2352 j held whole
  const int64_t fit = room < 0 ? 0 : room / SECTOR + 1;
  return n < fit ? n : fit;
}

struct GridOut {      // one call's header search, read back by the host
  int64_t restart;    // R: the next call emits from here (NEVER after the final call)
  int64_t tail_pos;   // the byte the next call's buffer starts at
  int64_t candidates, confirmed;   // those in [emit_from, R)
  int64_t forced;     // a candidate's sector was emitted ahead of a break that is certain
};

// first index in [0, n) with v[i] >= x (n when none); v ascends
LDG_EFMSEC_HD inline int64_t lower_bound(const int64_t* v, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The restart point: the last settled confirmed candidate (its sectors are the next call's),
// else just past the settled range.  The buffer holds bytes [pos0, w.end).
LDG_EFMSEC_HD inline void finish(int64_t pos0, const int64_t* cand, int64_t ncand, const int64_t* conf, int64_t nconf,
                                 const Window& w, GridOut* o) {
  o->forced = 0;
  if (w.final_) {
    o->restart = NEVER;
    o->tail_pos = w.end;
  } else {
    const int64_t kl = lower_bound(conf, nconf, w.lim + 1) - 1;
    int64_t r = w.lim + 1 > w.emit_from ? w.lim + 1 : w.emit_from;
    if (kl >= 0 && conf[kl] >= w.emit_from) {
      if (w.lim - conf[kl] >= BREAK_BYTES) o->forced = 1;
      else r = conf[kl];
    }
    o->restart = r;
    // a candidate at r - 2352 can still confirm one at r
    int64_t t = r - SECTOR;
    if (t < pos0) t = pos0;
    if (t > w.end) t = w.end;
    o->tail_pos = t;
  }
  o->candidates = lower_bound(cand, ncand, o->restart) - lower_bound(cand, ncand, w.emit_from);
  o->confirmed = lower_bound(conf, nconf, o->restart) - lower_bound(conf, nconf, w.emit_from);
}

// The header search's state between calls.
struct Carry {
  int64_t pos0 = 0;            // index of the first byte the next buffer holds
  int64_t emit_from = 0;
  bool pending_break = false;  // a break counts once another confirmed candidate turns up
};

inline Window window_of(const Carry& c, int64_t end, bool final_) {
  return Window{c.emit_from, final_ ? NEVER : end - SETTLE, end, final_ ? 1 : 0};
}

// Applies a call's result; returns the breaks to add for a pending break that came true.
inline int64_t advance(Carry* c, const GridOut& g) {
  int64_t add = 0;
  if (c->pending_break && g.confirmed > 0) {
    add = 1;
    c->pending_break = false;
  }
  if (g.forced) c->pending_break = true;
  c->emit_from = g.restart;
  c->pos0 = g.tail_pos;
  return add;
}

}  // namespace efmsec
}  // namespace ldg
