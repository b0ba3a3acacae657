// EFM decode: what a chunk of run lengths may emit and what the next
// chunk has to see again, so that the result does not depend on how the stream is cut into
// calls.  Plain C++ (no device, no HIP): efmdec.hip calls frames_of / finish from its
// kernels, efmdec.inc carries the state between calls with them, and tests/san/efmdec_san.cpp
// runs all of it under the sanitizers.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define LDG_EFMDEC_HD __host__ __device__
#else
#define LDG_EFMDEC_HD
#endif

namespace ldg {
namespace efmdec {

constexpr int64_t FRAME_BITS = 588;
constexpr int64_t MAX_COAST = 7350;              // frames between two confirmed syncs, at the most
constexpr int64_t LAST_BIT = 27 + 17 * 32 + 13;  // a frame's last symbol bit, from its start
// a candidate at c is settled once a candidate at c + 588 would be held whole (11 + 11 bits)
constexpr int64_t SETTLE = FRAME_BITS + 22;
// floor(d / 588 + 0.5) > 7350 from this d on
constexpr int64_t BREAK_BITS = (2 * MAX_COAST + 1) * FRAME_BITS / 2;
constexpr int64_t NEVER = INT64_MAX;
constexpr int LATENCY = 111;                     // F3 frames before the first sample
constexpr int C2_FIRST = 109;                    // first frame with a C2 word

// What a call's sync search may decide.  Positions are channel bits from the stream's first
// transition.  Candidates above `lim` are not settled (final call: all are); candidates
// below `emit_from` were dealt with by an earlier call and are held only to confirm others.
struct Window {
  int64_t emit_from;
  int64_t lim;       // E - SETTLE, or NEVER in the final call
  int64_t end;       // E: the position of the last transition held
  int32_t final_;
};

// Frames confirmed candidate k of conf[0 .. nconf) starts in this call (after truncation);
// *brk: a break was counted.
LDG_EFMDEC_HD inline int64_t frames_of(const int64_t* conf, int64_t nconf, int64_t k, const Window& w, int* brk) {
  *brk = 0;
  const int64_t a = conf[k];
  if (a < w.emit_from) return 0;
  int64_t n;
  if (k + 1 < nconf && (w.final_ || conf[k + 1] <= w.lim)) {
    n = (2 * (conf[k + 1] - a) + FRAME_BITS) / (2 * FRAME_BITS);
    if (n > MAX_COAST) {
      n = 1;
      *brk = 1;
    }
  } else if (w.final_) {
    n = 1;                                        // the last confirmed candidate
  } else if (a <= w.lim && w.lim - a >= BREAK_BITS) {
    n = 1;                                        // whatever follows is a break: finish() moves on
  } else {
    n = 0;                                        // the next call's
  }
  const int64_t room = w.end - LAST_BIT - a;      // frames a + 588 j whose bits are all held
  const int64_t fit = room < 0 ? 0 : room / FRAME_BITS + 1;
  return n < fit ? n : fit;
}

struct GridOut {      // one call's sync search, read back by the host
  int64_t end;        // E
  int64_t restart;    // R: the next call emits from here (NEVER after the final call)
  int64_t tail_idx;   // the run index the next call's buffer starts at,
  int64_t tail_pos;   // and its position
  int64_t candidates, confirmed;   // those in [emit_from, R)
  int64_t forced;     // a candidate's frame was emitted ahead of a break that is certain
};

// first index in [0, n) with v[i] >= x (n when none); v ascends
LDG_EFMDEC_HD inline int64_t lower_bound(const int64_t* v, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The restart point: the last settled confirmed candidate (its frames are the next call's),
// else just past the settled range.  pos[0 .. nrun] are the held transitions.
LDG_EFMDEC_HD inline void finish(const int64_t* pos, int64_t nrun, const int64_t* cand, int64_t ncand,
                                 const int64_t* conf, int64_t nconf, const Window& w, GridOut* o) {
  o->end = w.end;
  o->forced = 0;
  if (w.final_) {
    o->restart = NEVER;
    o->tail_idx = nrun;
    o->tail_pos = w.end;
  } else {
    const int64_t kl = lower_bound(conf, nconf, w.lim + 1) - 1;
    int64_t r = w.lim + 1 > w.emit_from ? w.lim + 1 : w.emit_from;
    if (kl >= 0 && conf[kl] >= w.emit_from) {
      if (w.lim - conf[kl] >= BREAK_BITS) o->forced = 1;
      else r = conf[kl];
    }
    o->restart = r;
    // the last transition at or before r - 588: a candidate there can still confirm one at r
    int64_t i = lower_bound(pos, nrun + 1, r - FRAME_BITS + 1) - 1;
    if (i < 0) i = 0;
    o->tail_idx = i;
    o->tail_pos = pos[i];
  }
  o->candidates = lower_bound(cand, ncand, o->restart) - lower_bound(cand, ncand, w.emit_from);
  o->confirmed = lower_bound(conf, nconf, o->restart) - lower_bound(conf, nconf, w.emit_from);
}

// The sync search's state between calls.
struct SyncCarry {
  int64_t pos0 = 0;            // position of the first transition the next buffer holds
  int64_t emit_from = 0;
  bool pending_break = false;  // a break counts once another confirmed candidate turns up
};

inline Window window_of(const SyncCarry& c, int64_t end, bool final_) {
  return Window{c.emit_from, final_ ? NEVER : end - SETTLE, end, final_ ? 1 : 0};
}

// Applies a call's result; returns the breaks to add for a pending break that came true.
inline int64_t advance(SyncCarry* c, const GridOut& g) {
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

// The CIRC and PCM stages see F3 frames [g0, g0 + held + fresh): C1 exists from local index
// 1, C2 from 109, samples from 111.  A call emits the concealed samples of frames [e0, e1):
// all whose right-hand neighbour it holds (final call: all), and keeps what frame e1 - 1
// needs, so that e1's left-hand neighbour can be computed again.
struct CircCarry {
  int64_t g0 = 0;        // global index of the first frame held
  int64_t held = 0;      // frames held from earlier calls
  int64_t e0 = LATENCY;  // first frame whose samples are not emitted yet
};

struct CircPlan {
  int64_t total;         // frames in the buffer
  int64_t e1;
  int64_t keep_from;     // local index the next call's buffer starts at
};

inline CircPlan circ_plan(const CircCarry& c, int64_t fresh, bool final_) {
  CircPlan p;
  p.total = c.held + fresh;
  const int64_t g1 = c.g0 + p.total;
  p.e1 = final_ ? g1 : g1 - 1;
  if (p.e1 < c.e0) p.e1 = c.e0;
  int64_t keep = p.e1 - 1 - LATENCY - c.g0;       // frame e1 - 1 is local 111 of the next buffer
  if (keep < 0) keep = 0;
  p.keep_from = final_ ? p.total : keep;
  return p;
}

inline void circ_advance(CircCarry* c, const CircPlan& p) {
  c->g0 += p.keep_from;
  c->held = p.total - p.keep_from;
  c->e0 = p.e1;
}

}  // namespace efmdec
}  // namespace ldg
