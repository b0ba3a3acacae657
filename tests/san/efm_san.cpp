// The EFM extraction's host planning (csrc/efm_plan.hpp: which samples, decimated samples,
// baseline blocks and kernel tiles a segment range needs) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no device and no library.  It walks
// file lengths and segment ranges around every edge (files shorter than the filter, than one
// baseline span, ends just before and after a block, a tile, a segment; ranges past the
// file; extreme indices) and checks each plan against the definition stated level by level.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ld-decode_amd/csrc/efm_plan.hpp"

#ifndef PROG
#define PROG "efm_san"
#endif

using namespace ldg::efm;

static int fails = 0;
#define CHECK(c)                                                                              \
  do {                                                                                        \
    if (!(c)) {                                                                               \
      std::printf("FAIL %s:%d: %s (n %lld, segments %lld..%lld)\n", __FILE__, __LINE__, #c,   \
                  (long long)g_n, (long long)g_a, (long long)g_b);                            \
      if (++fails > 20) std::exit(1);                                                         \
    }                                                                                         \
  } while (0)
static int64_t g_n, g_a, g_b;

// z[m] is defined: blocks (m >> 6) - 4 .. + 4 have all 64 of their y, whose taps lie in the file
static bool z_defined(int64_t m, int64_t n) {
  if (m < 0) return false;
  const int64_t lo = ((m >> 6) - BASE_HALF) * BLOCK, hi = ((m >> 6) + BASE_HALF) * BLOCK + BLOCK - 1;
  return lo * DEC - HALF_TAPS >= 0 && hi * DEC + HALF_TAPS <= n - 1;
}

static void check(int64_t a, int64_t b, int64_t n) {
  g_n = n;
  g_a = a;
  g_b = b;
  Plan p;
  const int rc = plan(a, b, n, &p);
  if (a < 0 || b < a || n < 0 || b > MAX_SEG_INDEX) {
    CHECK(rc == -1);
    return;
  }
  CHECK(rc == 0);
  CHECK(0 <= p.win_lo && p.win_lo <= p.win_hi && p.win_hi <= n && p.win_lo % 12 == 0);
  if (b == a) {
    CHECK(p.win_hi == 0 && p.z_hi < p.z_lo);
    return;
  }
  // the z the range's crossings touch, by the definition
  const int64_t t0 = a * SEG - RUNIN, t1 = b * SEG;
  int64_t mz_lo = floor_div(t0, DEC) - 1, mz_hi = t1 / DEC;
  if (mz_lo < 0) mz_lo = 0;
  if (p.z_hi >= p.z_lo) {
    CHECK(p.z_lo >= mz_lo && p.z_hi <= mz_hi);
    CHECK(z_defined(p.z_lo, n) && z_defined(p.z_hi, n));
    CHECK(p.z_lo == mz_lo || !z_defined(p.z_lo - 1, n));
    CHECK(p.z_hi == mz_hi || !z_defined(p.z_hi + 1, n));
    CHECK(p.b_lo == (p.z_lo >> 6) - BASE_HALF && p.b_hi == (p.z_hi >> 6) + BASE_HALF);
    CHECK(p.tile_lo * BLOCKS_PER_TILE <= p.b_lo && p.b_hi < p.tile_hi * BLOCKS_PER_TILE);
    CHECK(p.tile_hi - p.tile_lo <= (p.b_hi - p.b_lo) / BLOCKS_PER_TILE + 2);
    CHECK(p.ctile_lo * TILE <= p.z_lo && p.z_hi < p.ctile_hi * TILE);
    CHECK(p.need_lo == p.b_lo * BLOCK * DEC - HALF_TAPS);
    CHECK(p.need_hi == (p.b_hi * BLOCK + BLOCK - 1) * DEC + HALF_TAPS + 1);
    CHECK(p.win_lo <= p.need_lo && p.need_hi <= p.win_hi && p.need_lo >= 0 && p.need_hi <= n);
  } else {
    // no z: nothing in the touched range is defined (sampled: both ends and the file's reach)
    CHECK(!z_defined(mz_lo, n) || mz_lo > mz_hi);
    CHECK(p.need_lo == p.need_hi);
    for (int64_t m = mz_lo; m <= mz_hi && m < mz_lo + 4096; m++) CHECK(!z_defined(m, n));
    if (n >= 4 * (int64_t)BLOCK * DEC) {
      const int64_t m = (n / DEC) - 5 * BLOCK;     // around the last defined z of the file
      for (int64_t k = m - 2 * BLOCK; k <= m + 2 * BLOCK; k++)
        if (k >= mz_lo && k <= mz_hi) CHECK(!z_defined(k, n));
    }
  }
}

int main() {
  std::vector<int64_t> lens = {0, 1, 126, 127, 128, 254, 255, 256, 2683, 2684, 2685, 2939, 2940, 4096, 65536};
  for (int64_t base : {SEG - RUNIN, SEG, SEG + RUNIN, 2 * SEG, 5 * SEG / 2, 3 * SEG, 64 * SEG, ((int64_t)1 << 33) + 12345})
    for (int64_t d : {-4097, -2685, -1300, -257, -256, -255, -129, -128, -127, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 127, 128,
                      255, 256, 257, 1023, 1024, 4095, 4096, 4350})
      lens.push_back(base + d);
  int64_t plans = 0;
  for (int64_t n : lens) {
    const int64_t nseg = (n + SEG - 1) / SEG;
    std::vector<int64_t> idx = {0, 1, 2, 3, nseg - 2, nseg - 1, nseg, nseg + 1, nseg + 70};
    for (int64_t a : idx)
      for (int64_t b : idx) {
        check(a, b, n);
        plans++;
      }
  }
  check(-1, 1, 1000);
  check(0, MAX_SEG_INDEX, ((int64_t)1 << 50));
  check(MAX_SEG_INDEX - 1, MAX_SEG_INDEX, ((int64_t)1 << 61));
  check(0, MAX_SEG_INDEX + 1, 1000);
  check(0, 1, -5);
  // the first file that defines any z, and the last that does not
  Plan p;
  plan(0, 1, 2684, &p);
  g_n = 2684;
  CHECK(p.z_lo == 320 && p.z_hi == 383);
  plan(0, 1, 2683, &p);
  CHECK(p.z_hi < p.z_lo);
  if (fails) return 1;
  std::printf("%s ok (%lld plans)\n", PROG, (long long)plans);
  return 0;
}
