// The EFM data sectors' chunk planning (csrc/efmsec_plan.hpp: which sectors a call may emit,
// where the next call restarts, which bytes it keeps) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no device and no library.  A serial model
// of the grid kernels (candidates, confirmation; sectors_of and finish are the header's own, as
// the kernels call them) runs byte streams with lost headers, chance patterns, two interleaved
// grids, long gaps and no header at all, whole and cut into calls of 1 to 2^16 bytes; the
// sector starts and counters must not depend on the cut, must equal the rule stated directly
// over the whole stream, and every sector emitted must lie inside the bytes the call holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ld-decode_amd/csrc/efmsec_plan.hpp"

using namespace ldg::efmsec;

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
  return k < (int64_t)v.size() && v[(size_t)k] == x;
}

static bool pattern(const uint8_t* p) {
  if (p[0] != 0 || p[11] != 0) return false;
  for (int j = 1; j <= 10; j++)
    if (p[j] != 255) return false;
  return true;
}

// candidates of the buffer b (its first byte is stream byte pos0), confirmed ones
static void search(const std::vector<uint8_t>& b, int64_t pos0, std::vector<int64_t>* cand, std::vector<int64_t>* conf) {
  for (size_t i = 0; i + 12 <= b.size(); i++)
    if (pattern(b.data() + i)) cand->push_back(pos0 + (int64_t)i);
  for (int64_t c : *cand)
    if (has(*cand, c + 2352) || has(*cand, c - 2352)) conf->push_back(c);
}

// the rule, directly
static Result direct(const std::vector<uint8_t>& by) {
  Result r;
  std::vector<int64_t> cand, conf;
  search(by, 0, &cand, &conf);
  r.candidates = (int64_t)cand.size();
  r.confirmed = (int64_t)conf.size();
  const int64_t n = (int64_t)by.size();
  for (size_t k = 0; k < conf.size(); k++) {
    int64_t m = 1;
    if (k + 1 < conf.size()) {
      m = (2 * (conf[k + 1] - conf[k]) + 2352) / 4704;
      if (m > 75) {
        m = 1;
        r.breaks++;
      }
    }
    int64_t got = 0;
    for (int64_t j = 0; j < m; j++)
      if (conf[k] + 2352 * j + 2352 <= n) {
        r.starts.push_back(conf[k] + 2352 * j);
        got++;
      }
    if (got > 1) r.coasted += got - 1;
  }
  return r;
}

// the calls, as efmsec.inc makes them
static Result chunked(const std::vector<uint8_t>& by, size_t chunk) {
  Result r;
  Carry carry;
  std::vector<uint8_t> held;
  size_t at = 0;
  while (true) {
    const size_t b = at + chunk < by.size() ? at + chunk : by.size();
    const bool fin = b >= by.size();
    held.insert(held.end(), by.begin() + (long)at, by.begin() + (long)b);
    const int64_t nb = (int64_t)held.size(), pos0 = carry.pos0;
    if (nb > r.max_held) r.max_held = nb;
    CHECK(pos0 + nb == (int64_t)b);
    std::vector<int64_t> cand, conf;
    search(held, pos0, &cand, &conf);
    const Window w = window_of(carry, pos0 + nb, fin);
    for (int64_t k = 0; k < (int64_t)conf.size(); k++) {
      int brk = 0;
      const int64_t m = sectors_of(conf.data(), (int64_t)conf.size(), k, w, &brk);
      CHECK(m >= 0 && m <= MAX_COAST);
      for (int64_t j = 0; j < m; j++) {
        const int64_t s = conf[(size_t)k] + SECTOR * j;
        CHECK(s >= pos0 && s + SECTOR <= pos0 + nb);                     // what the fix kernel reads is held
        r.starts.push_back(s);
      }
      if (m > 1) r.coasted += m - 1;
      r.breaks += brk;
    }
    GridOut g;
    finish(pos0, cand.data(), (int64_t)cand.size(), conf.data(), (int64_t)conf.size(), w, &g);
    CHECK(g.tail_pos >= pos0 && g.tail_pos <= pos0 + nb);
    CHECK(fin || g.restart >= carry.emit_from);
    CHECK(fin || g.tail_pos <= g.restart);
    CHECK(fin || g.tail_pos == pos0 || g.restart - g.tail_pos >= SECTOR);
    r.candidates += g.candidates;
    r.confirmed += g.confirmed;
    r.breaks += advance(&carry, g);
    held.erase(held.begin(), held.begin() + (long)(g.tail_pos - pos0));
    at = b;
    if (fin) break;
  }
  return r;
}

static uint32_t rng_state = 4711;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static void noise(std::vector<uint8_t>* by, int64_t n) {
  for (int64_t i = 0; i < n; i++) by->push_back((uint8_t)(1 + rnd() % 254));   // 1..254: part of no pattern
}

static void sync_at(std::vector<uint8_t>* by, size_t at) {
  (*by)[at] = (*by)[at + 11] = 0;
  for (int j = 1; j <= 10; j++) (*by)[at + (size_t)j] = 255;
}

static void sector(std::vector<uint8_t>* by, bool sync = true) {
  const size_t at = by->size();
  noise(by, 2352);
  if (sync) sync_at(by, at);
}

static void run_case(const char* name, const std::vector<uint8_t>& by, bool big = false) {
  g_case = name;
  g_chunk = 0;
  const Result want = direct(by);
  std::vector<size_t> chunks = {by.size() + 1, 65536, 5000, 2364, 2352, 2351, 777, 64, 12, 11, 1};
  if (big) chunks = {by.size() + 1, 65536, 5000, 777};
  for (size_t c : chunks) {
    g_chunk = (long long)c;
    const Result got = chunked(by, c);
    CHECK(got == want);
    if (!(got == want))
      std::printf("  sectors %zu / %zu, candidates %lld / %lld, confirmed %lld / %lld, coasted %lld / %lld, breaks %lld / %lld\n",
                  got.starts.size(), want.starts.size(), (long long)got.candidates, (long long)want.candidates,
                  (long long)got.confirmed, (long long)want.confirmed, (long long)got.coasted, (long long)want.coasted,
                  (long long)got.breaks, (long long)want.breaks);
  }
}

int main() {
  std::vector<uint8_t> by;
  // clean sectors from byte 40, a partial one at the end
  noise(&by, 40);
  for (int i = 0; i < 6; i++) sector(&by);
  noise(&by, 56);
  run_case("clean", by);
  CHECK(direct(by).starts.size() == 6);
  // the stream ends inside the last sector: it is dropped
  by.resize(by.size() - 100);
  run_case("cut short", by);
  CHECK(direct(by).starts.size() == 5);
  // lost headers (coasting), a chance pattern, a second grid 1000 bytes off, leading and trailing noise
  by.clear();
  noise(&by, 3000);
  for (int i = 0; i < 14; i++) sector(&by, !(i == 4 || i == 5 || i == 9));
  sync_at(&by, 3000 + 2352 * 7 + 700);
  sync_at(&by, 3000 + 2352 * 11 + 1000);
  sync_at(&by, 3000 + 2352 * 12 + 1000);
  noise(&by, 5000);
  run_case("damaged", by);
  CHECK(direct(by).coasted == 3);
  // a slip: the grid moves by 5 bytes half way
  by.clear();
  for (int i = 0; i < 5; i++) sector(&by);
  noise(&by, 5);
  for (int i = 0; i < 5; i++) sector(&by);
  run_case("slip", by);
  // no header at all; one candidate; two candidates not 2352 apart; empty; short inputs
  by.clear();
  noise(&by, 20000);
  run_case("no sync", by);
  sync_at(&by, 100);
  run_case("one candidate", by);
  sync_at(&by, 100 + 2351);
  run_case("not apart", by);
  run_case("empty", std::vector<uint8_t>());
  run_case("one byte", std::vector<uint8_t>(1, 0));
  by.assign(12, 255);
  by[0] = by[11] = 0;
  run_case("a pattern alone", by);
  // patterns back to back (the closing 00 opens the next), confirmed where 2352 apart: never (2352 = 213.8 x 11)
  by.clear();
  for (int i = 0; i < 500; i++) {
    by.push_back(0);
    for (int j = 0; j < 10; j++) by.push_back(255);
  }
  by.push_back(0);
  run_case("back to back", by);
  // a gap longer than 75 sectors between headers (a break), then the stream ends without another
  by.clear();
  for (int i = 0; i < 3; i++) sector(&by);
  noise(&by, 80 * 2352);
  for (int i = 0; i < 3; i++) sector(&by);
  noise(&by, 80 * 2352 + 17);
  run_case("breaks", by, true);
  const Result br = direct(by);
  CHECK(br.breaks == 1 && br.starts.size() == 6);
  // the held bytes stay bounded across a long gap (the forced break)
  g_case = "held";
  CHECK(chunked(by, 5000).max_held < BREAK_BYTES + 2 * 5000 + SETTLE);
  // a gap of exactly 75 sectors coasts, 76 breaks
  for (int gap : {75, 76}) {
    by.clear();
    for (int i = 0; i < 2; i++) sector(&by);
    noise(&by, (int64_t)(gap - 1) * 2352);
    for (int i = 0; i < 2; i++) sector(&by);
    run_case(gap == 75 ? "gap 75" : "gap 76", by, true);
    CHECK(direct(by).breaks == (gap == 76 ? 1 : 0));
  }
  if (fails) return 1;
  std::printf("efmsec_san ok\n");
  return 0;
}
