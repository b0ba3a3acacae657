// The EFM decode's chunk planning (csrc/efmdec_plan.hpp: which frames a call may emit, where
// the next call restarts, what the CIRC stage carries) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no device and no library.  A serial model
// of the sync-search kernels (positions, candidates, confirmation; frames_of and finish are
// the header's own, as the kernels call them) runs streams with lost syncs, bit slips, chance
// sync patterns, long gaps and no sync at all, whole and cut into calls of many sizes; the
// frame starts and counters must not depend on the cut, and must equal the rule stated
// directly over the whole stream.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ld-decode_amd/csrc/efmdec_plan.hpp"

using namespace ldg::efmdec;

static int fails = 0;
static const char* g_case = "";
static long long g_chunk = 0;
#define CHECK(c)                                                                                            \
  do {                                                                                                      \
    if (!(c)) {                                                                                             \
      std::printf("FAIL %s:%d: %s (%s, chunk %lld)\n", __FILE__, __LINE__, #c, g_case, g_chunk);            \
      if (++fails > 20) std::exit(1);                                                                       \
    }                                                                                                       \
  } while (0)

struct Result {
  std::vector<int64_t> starts;
  int64_t candidates = 0, confirmed = 0, coasted = 0, breaks = 0, max_held = 0;
  bool operator==(const Result& o) const {
    return starts == o.starts && candidates == o.candidates && confirmed == o.confirmed && coasted == o.coasted &&
           breaks == o.breaks;
  }
};

static bool has(const std::vector<int64_t>& v, int64_t x) {
  const int64_t k = lower_bound(v.data(), (int64_t)v.size(), x);
  return k < (int64_t)v.size() && v[k] == x;
}

// the rule, directly
static Result direct(const std::vector<uint8_t>& rl) {
  Result r;
  std::vector<int64_t> pos(rl.size() + 1, 0), cand, conf;
  for (size_t i = 0; i < rl.size(); i++) pos[i + 1] = pos[i] + rl[i];
  for (size_t i = 0; i + 1 < rl.size(); i++)
    if (rl[i] == 11 && rl[i + 1] == 11) cand.push_back(pos[i]);
  for (int64_t c : cand)
    if (has(cand, c + 588) || has(cand, c - 588)) conf.push_back(c);
  r.candidates = (int64_t)cand.size();
  r.confirmed = (int64_t)conf.size();
  for (size_t k = 0; k < conf.size(); k++) {
    int64_t n = 1;
    if (k + 1 < conf.size()) {
      n = (2 * (conf[k + 1] - conf[k]) + 588) / 1176;
      if (n > 7350) {
        n = 1;
        r.breaks++;
      }
    }
    int64_t m = 0;
    for (int64_t j = 0; j < n; j++)
      if (conf[k] + 588 * j + 584 <= pos.back()) {
        r.starts.push_back(conf[k] + 588 * j);
        m++;
      }
    if (m > 1) r.coasted += m - 1;
  }
  return r;
}

// the calls, as efmdec.inc makes them
static Result chunked(const std::vector<uint8_t>& rl, size_t chunk) {
  Result r;
  SyncCarry carry;
  std::vector<uint8_t> tail;
  size_t at = 0;
  while (true) {
    const size_t b = at + chunk < rl.size() ? at + chunk : rl.size();
    const bool fin = b >= rl.size();
    tail.insert(tail.end(), rl.begin() + (long)at, rl.begin() + (long)b);
    const int64_t nrun = (int64_t)tail.size();
    if ((int64_t)tail.size() > r.max_held) r.max_held = (int64_t)tail.size();
    std::vector<int64_t> pos((size_t)nrun + 1, carry.pos0), cand, conf;
    for (int64_t i = 0; i < nrun; i++) pos[(size_t)i + 1] = pos[(size_t)i] + tail[(size_t)i];
    for (int64_t i = 0; i + 1 < nrun; i++)
      if (tail[(size_t)i] == 11 && tail[(size_t)i + 1] == 11) cand.push_back(pos[(size_t)i]);
    for (int64_t c : cand)
      if (has(cand, c + 588) || has(cand, c - 588)) conf.push_back(c);
    const Window w = window_of(carry, pos.back(), fin);
    for (int64_t k = 0; k < (int64_t)conf.size(); k++) {
      int brk = 0;
      const int64_t m = frames_of(conf.data(), (int64_t)conf.size(), k, w, &brk);
      for (int64_t j = 0; j < m; j++) r.starts.push_back(conf[(size_t)k] + FRAME_BITS * j);
      if (m > 1) r.coasted += m - 1;
      r.breaks += brk;
    }
    GridOut g;
    finish(pos.data(), nrun, cand.data(), (int64_t)cand.size(), conf.data(), (int64_t)conf.size(), w, &g);
    CHECK(g.tail_idx >= 0 && g.tail_idx <= nrun && g.tail_pos == pos[(size_t)g.tail_idx]);
    CHECK(fin || g.restart >= carry.emit_from);
    CHECK(fin || g.tail_pos <= g.restart);
    CHECK(fin || g.tail_idx == 0 || g.restart - g.tail_pos >= FRAME_BITS);
    r.candidates += g.candidates;
    r.confirmed += g.confirmed;
    r.breaks += advance(&carry, g);
    tail.erase(tail.begin(), tail.begin() + (long)g.tail_idx);
    at = b;
    if (fin) break;
  }
  return r;
}

static uint32_t rng_state = 12345;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

// a frame: 11, 11, then runs of 3..10 filling 588 bits
static void frame(std::vector<uint8_t>* rl, bool sync = true) {
  int left = 588;
  if (sync) {
    rl->push_back(11);
    rl->push_back(11);
    left -= 22;
  }
  while (left) {
    int r = 3 + (int)(rnd() % 8);
    if (left - r != 0 && left - r < 3) r = left <= 10 ? left : 3;
    if (r > left) r = left;
    rl->push_back((uint8_t)r);
    left -= r;
  }
}

static void noise(std::vector<uint8_t>* rl, int64_t bits) {
  while (bits > 0) {
    const int r = 3 + (int)(rnd() % 8);
    rl->push_back((uint8_t)r);
    bits -= r;
  }
}

static void run_case(const char* name, const std::vector<uint8_t>& rl, bool big = false) {
  g_case = name;
  g_chunk = 0;
  const Result want = direct(rl);
  std::vector<size_t> chunks = {rl.size() + 1, 4096, 1000, 333, 64, 7, 1};
  if (big) chunks = {rl.size() + 1, 1 << 20, 65536, 4096};
  for (size_t c : chunks) {
    g_chunk = (long long)c;
    const Result got = chunked(rl, c);
    CHECK(got == want);
    if (!(got == want))
      std::printf("  frames %zu / %zu, candidates %lld / %lld, confirmed %lld / %lld, coasted %lld / %lld, breaks %lld / %lld\n",
                  got.starts.size(), want.starts.size(), (long long)got.candidates, (long long)want.candidates,
                  (long long)got.confirmed, (long long)want.confirmed, (long long)got.coasted, (long long)want.coasted,
                  (long long)got.breaks, (long long)want.breaks);
  }
}

// the CIRC stage's carry: the calls' sample ranges tile [111, F), and a call holds what it reads
static void circ_walk(const std::vector<int64_t>& fresh) {
  CircCarry c;
  int64_t frames = 0, next = LATENCY;
  for (size_t i = 0; i < fresh.size(); i++) {
    const bool fin = i + 1 == fresh.size();
    const CircPlan p = circ_plan(c, fresh[i], fin);
    frames += fresh[i];
    CHECK(p.total == c.held + fresh[i] && c.g0 + p.total == frames);
    CHECK(c.e0 == next && p.e1 >= c.e0 && p.e1 <= (frames > LATENCY ? frames : LATENCY));
    if (p.e1 > c.e0) {
      CHECK(c.e0 - c.g0 >= LATENCY);                                 // the first emitted frame has its 111 before it
      CHECK(c.e0 == LATENCY || c.e0 - 1 - c.g0 >= LATENCY);          // and its left-hand neighbour's samples exist
      CHECK(fin || p.e1 < frames);                                   // the right-hand neighbour is held
    }
    CHECK(fin ? p.e1 == (frames > LATENCY ? frames : LATENCY) : true);
    CHECK(p.keep_from >= 0 && p.keep_from <= p.total);
    next = p.e1;
    circ_advance(&c, p);
    CHECK(c.held <= LATENCY + 2 || c.g0 == 0);
  }
}

int main() {
  std::vector<uint8_t> rl;
  // clean frames, a closing sync
  for (int i = 0; i < 40; i++) frame(&rl);
  rl.push_back(11);
  rl.push_back(11);
  rl.push_back(5);
  run_case("clean", rl);
  // lost syncs (coasting), a bit slip, a chance pair, leading and trailing noise
  rl.clear();
  noise(&rl, 2000);
  for (int i = 0; i < 60; i++) {
    const size_t at = rl.size();
    frame(&rl, !(i == 20 || i == 21 || i == 33));
    if (i == 40) rl[at + 10] += 1;
    if (i == 45) {
      rl[at + 30] = 11;
      rl[at + 31] = 11;
    }
  }
  noise(&rl, 3000);
  run_case("damaged", rl);
  // no sync at all; one candidate only; empty; a single run
  rl.clear();
  noise(&rl, 30000);
  run_case("no sync", rl);
  rl[100] = rl[101] = 11;
  run_case("one candidate", rl);
  run_case("empty", std::vector<uint8_t>());
  run_case("one run", std::vector<uint8_t>(1, 11));
  // every run 11: every transition a candidate, confirmed only where 588 apart (never: 588 = 53.45 x 11)
  run_case("all eleven", std::vector<uint8_t>(3000, 11));
  // zeros and long runs among the bytes
  rl.clear();
  for (int i = 0; i < 20; i++) frame(&rl);
  rl[50] = 0;
  rl[51] = 255;
  for (int i = 0; i < 20; i++) frame(&rl);
  run_case("odd bytes", rl);
  // a gap longer than 7350 frames between syncs (a break), then the stream ends without another
  rl.clear();
  for (int i = 0; i < 5; i++) frame(&rl);
  noise(&rl, 7400 * 588);
  for (int i = 0; i < 5; i++) frame(&rl);
  noise(&rl, 7400 * 588);
  run_case("breaks", rl, true);
  const Result br = direct(rl);
  CHECK(br.breaks == 1 && br.starts.size() >= 8);
  // the held run lengths stay bounded across a long gap (the forced break)
  g_case = "held";
  CHECK(chunked(rl, 65536).max_held < 2 * BREAK_BITS / 3);

  circ_walk({0});
  circ_walk({50, 0});
  circ_walk({111, 0});
  circ_walk({112});
  circ_walk({300});
  circ_walk({1, 1, 1, 0});
  circ_walk({100, 11, 1, 1, 200, 0, 3, 1000, 5});
  circ_walk({0, 0, 110, 1, 1, 1, 1});
  std::vector<int64_t> ones(400, 1);
  circ_walk(ones);
  if (fails) return 1;
  std::printf("efmdec_san ok\n");
  return 0;
}
