// The tail plan of a read: which of its audio work lies past
// its video cut and is read by nothing.  One copy of the arithmetic for the host's
// read set-up (abi.inc), ldg_k_probe_pick (demod.hip), the kernels that skip by it and
// the geometry test hook (ldg_tail_plan).
#pragma once
#include <stdint.h>

#include "common.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDG_HD __host__ __device__
#else
#define LDG_HD
#endif

namespace ldg {

constexpr int32_t ACUT_NONE = INT32_MAX;                      // acut1 / acut2: nothing is trimmed
constexpr int A2_SKIP = 64;                                   // audio phase 2's overlap (lddecode_core.py:335-371)
constexpr int A2_JUMP = BLOCKLEN - A2_SKIP * AUDIO_DIV2;      // 16128: phase-2 blocks step by this many 2.5 MHz samples
constexpr int A2_KEEP = AUDIO2_BLOCK - A2_SKIP;               // 4032 outputs per block after the first
constexpr int A1_STEP = BLOCKSTEP / AUDIO_DIV1;               // 958 audio-1 samples kept per demod block
static_assert(BLOCKSTEP % AUDIO_DIV1 == 0, "a demod block keeps whole audio-1 samples");

// Audio phase 2's block layout over a read's n_in 2.5 MHz samples: a first block,
// n_mid middle blocks at A2_JUMP, and a last block placed from the read's end, which
// alone produces the outputs from last_start on.
LDG_HD inline int a2_n_mid(int n_in) {
  const int span = n_in - A2_JUMP - A2_JUMP;
  return span > 0 ? (span + A2_JUMP - 1) / A2_JUMP : 0;
}
LDG_HD inline int a2_block_start(int j, int n_mid, int n_in) {
  return j == 0 ? 0 : (j <= n_mid ? A2_JUMP * j : n_in - BLOCKLEN - 1);
}
LDG_HD inline int a2_last_start(int n_out2) { return n_out2 - A2_KEEP; }

struct TailPlan {
  int32_t acut1;      // first audio-1 (2.5 MHz) sample no live phase-2 block reads
  int32_t acut2;      // first audio-2 (625 kHz) output that is not produced
};

// Audio trimming engages only when everything the read's video can need, in audio-2
// units (ceil(vcut / 64): a line location below vcut indexes audio-2 below that), lies
// at or below the first output only the last phase-2 block serves.  Then that block is
// dead, and with it every audio-1 sample from the live blocks' reach on.
LDG_HD inline TailPlan tail_plan(int n_audio, int n_audio2, int64_t vcut) {
  TailPlan p{ACUT_NONE, ACUT_NONE};
  if (vcut <= 0 || vcut == INT64_MAX) return p;
  const int last_start = a2_last_start(n_audio2);
  if (last_start <= 0 || n_audio - BLOCKLEN - 1 < 0) return p;     // a short read: the last block serves it all
  const int64_t vcut2 = (vcut + AUDIO_DIV1 * AUDIO_DIV2 - 1) / (AUDIO_DIV1 * AUDIO_DIV2);
  if (vcut2 > last_start) return p;
  p.acut2 = last_start;
  p.acut1 = a2_n_mid(n_audio) * A2_JUMP + BLOCKLEN;
  return p;
}

// Demod block b keeps the audio-1 samples [b * A1_STEP, ...): dead when they all lie at or past acut1.
LDG_HD inline bool a1_block_dead(int b, int32_t acut1) { return (int64_t)b * A1_STEP >= acut1; }
// Phase-2 block j is dead when all its outputs are >= acut2: the last block of a trimmed read.
LDG_HD inline bool a2_block_dead(int j, int n_mid, int32_t acut2) { return acut2 != ACUT_NONE && j == n_mid + 1; }

// downscale_audio (lddecode_core.py:431-484; ldg_k_audio_ds) takes audio-2 sample
// int(pos / 64), pos between lf[il] and lf[il + 1] (lf[il] + linelen past the array's
// end), for the line il = int(ln) of each 48 kHz tick.  Its ticks run from the
// carried-in offset (above -1/48000 s: ln > 0.67, il >= 0) to below frametime + 1/48000 s
// (ln < linecount + 1.33, il <= linecount + 1).  The span of positions line il can give:
LDG_HD inline void audio_line_span(const double* lf, int nl, int il, double linelen, double& lo, double& hi) {
  const double cur = lf[il];
  const double nxt = (il + 1 < nl) ? lf[il + 1] : cur + linelen;
  lo = cur < nxt ? cur : nxt;
  hi = cur < nxt ? nxt : cur;
  if (!(cur == cur) || !(nxt == nxt)) lo = hi = cur + nxt;       // NaN fails every test below
}
LDG_HD inline int audio_last_line(int nl, int linecount) { return linecount + 1 < nl - 1 ? linecount + 1 : nl - 1; }
// every index of the span lies in [0, acut2) (a negative one would wrap to the tail)
LDG_HD inline bool audio_span_ok(double lo, double hi, int32_t acut2) {
  return lo >= 0.0 && hi < (double)(AUDIO_DIV1 * AUDIO_DIV2) * (double)acut2;
}

}  // namespace ldg
