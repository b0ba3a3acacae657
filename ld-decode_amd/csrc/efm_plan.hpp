// EFM run-length extraction: the geometry of a segment range --
// which capture samples, decimated samples, baseline blocks and kernel tiles it needs.
// Plain host C++ (no device, no HIP): efm.inc plans its launches with it, and
// tests/san/efm_san.cpp runs it under the sanitizers.
#pragma once
#include <stdint.h>

namespace ldg {
namespace efm {

constexpr int NTAPS = 255;                 // firwin(255, 1.75 MHz)
constexpr int HALF_TAPS = NTAPS / 2;       // y[m] reads x[4m - 127 .. 4m + 127]
constexpr int DEC = 4;
constexpr int BLOCK = 64;                  // decimated samples per baseline block
constexpr int BASE_HALF = 4;               // the baseline: blocks b - 4 .. b + 4
constexpr int64_t SEG = (int64_t)1 << 20;  // L: RF samples per segment
constexpr int64_t RUNIN = (int64_t)1 << 16;// R: a segment's run starts this far before it
constexpr int TILE = 1024;                 // decimated samples per workgroup tile (16 blocks)
constexpr int BLOCKS_PER_TILE = TILE / BLOCK;
constexpr double CHANNEL_HZ = 4321800.0;
constexpr int64_t MAX_SEG_INDEX = (int64_t)1 << 40;   // (segment times stay inside int64)

inline int64_t floor_div(int64_t a, int64_t b) {     // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// Everything below is in global indices (file sample 0 = 0).  Ranges [lo, hi] are
// inclusive and empty when hi < lo.
struct Plan {
  int64_t win_lo, win_hi;    // file samples [win_lo, win_hi) the range's definition may touch, clipped to the
                             // file; win_lo a multiple of 12 (whole .r30 and .lds groups); 0, 0: none
  int64_t need_lo, need_hi;  // samples [need_lo, need_hi) the kernels read (inside the window; equal: none)
  int64_t z_lo, z_hi;        // z[m] this range reads, clipped to where z is defined in the file
  int64_t b_lo, b_hi;        // baseline blocks whose sums z needs
  int64_t tile_lo, tile_hi;  // FIR tiles [tile_lo, tile_hi) of TILE outputs: y and the block sums they hold
  int64_t ctile_lo, ctile_hi;// crossing tiles [ctile_lo, ctile_hi) of TILE values of m
};

// The plan of segments [seg_lo, seg_hi) of a file of nsamples samples.  Returns 0, or -1 for
// an invalid range (negative, reversed or absurd indices, a negative file length).
inline int plan(int64_t seg_lo, int64_t seg_hi, int64_t nsamples, Plan* p) {
  *p = Plan{0, 0, 0, 0, 0, -1, 0, -1, 0, 0, 0, 0};
  if (seg_lo < 0 || seg_hi < seg_lo || seg_hi > MAX_SEG_INDEX || nsamples < 0) return -1;
  if (seg_hi == seg_lo || nsamples == 0) return 0;
  // a crossing between m - 1 and m lies in [4 (m - 1), 4 m]: the range's crossings have
  // times in [t0, t1), so it reads z[t0 / 4 - 1 .. t1 / 4]
  const int64_t t0 = seg_lo * SEG - RUNIN, t1 = seg_hi * SEG;
  int64_t mz_lo = floor_div(t0, DEC) - 1, mz_hi = t1 / DEC;
  if (mz_lo < 0) mz_lo = 0;
  // the window: those z's blocks, four more either side, their y's taps; clipped to the file
  {
    const int64_t lo = ((mz_lo >> 6) - BASE_HALF) * BLOCK * DEC - HALF_TAPS;
    const int64_t hi = (((mz_hi >> 6) + BASE_HALF) * BLOCK + BLOCK - 1) * DEC + HALF_TAPS + 1;
    const int64_t cl = lo < 0 ? 0 : lo, ch = hi > nsamples ? nsamples : hi;
    if (ch > cl) {
      p->win_lo = cl / 12 * 12;
      p->win_hi = ch;
    }
  }
  // where the file defines y, the block sums, the baseline and z
  if (nsamples < NTAPS) return 0;
  const int64_t y_lo = (HALF_TAPS + DEC - 1) / DEC, y_hi = (nsamples - 1 - HALF_TAPS) / DEC;
  const int64_t yb_lo = (y_lo + BLOCK - 1) / BLOCK, yb_hi = (y_hi + 1) / BLOCK - 1;
  const int64_t zb_lo = yb_lo + BASE_HALF, zb_hi = yb_hi - BASE_HALF;
  if (zb_hi < zb_lo) return 0;
  const int64_t zd_lo = zb_lo * BLOCK, zd_hi = zb_hi * BLOCK + BLOCK - 1;
  const int64_t z_lo = mz_lo > zd_lo ? mz_lo : zd_lo, z_hi = mz_hi < zd_hi ? mz_hi : zd_hi;
  if (z_hi < z_lo) return 0;
  p->z_lo = z_lo;
  p->z_hi = z_hi;
  p->b_lo = (z_lo >> 6) - BASE_HALF;
  p->b_hi = (z_hi >> 6) + BASE_HALF;
  p->tile_lo = p->b_lo / BLOCKS_PER_TILE;
  p->tile_hi = p->b_hi / BLOCKS_PER_TILE + 1;
  p->ctile_lo = z_lo / TILE;
  p->ctile_hi = z_hi / TILE + 1;
  p->need_lo = p->b_lo * BLOCK * DEC - HALF_TAPS;
  p->need_hi = (p->b_hi * BLOCK + BLOCK - 1) * DEC + HALF_TAPS + 1;
  return 0;
}

}  // namespace efm
}  // namespace ldg
