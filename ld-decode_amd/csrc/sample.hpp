// The loader: sample `rel` of a raw capture window as a double, for the four container
// formats (shared by the demod and the EFM extraction).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldg {

__device__ __forceinline__ double load_sample(const uint8_t* __restrict__ cap, int fmt, int64_t rel) {
  if (fmt == 0) return (double)cap[rel];
  if (fmt == 1) return (double)reinterpret_cast<const int16_t*>(cap)[rel];
  if (fmt == 2) {   // .r30: 3 x 10 bit per LE uint32, low bits first (lddutils.py:150-173)
    const int64_t w = rel / 3;
    const int sh = 10 * (int)(rel - 3 * w);
    return (double)((reinterpret_cast<const uint32_t*>(cap)[w] >> sh) & 0x3ffu);
  }
  // .lds: 4 x 10 bit in 5 bytes, MSB first (lddutils.py:195-229)
  const int64_t g = rel >> 2;
  const int k = (int)(rel & 3);
  const uint8_t* b = cap + 5 * g;
  uint32_t v;
  if (k == 0) v = ((uint32_t)b[0] << 2) | (b[1] >> 6);
  else if (k == 1) v = ((uint32_t)(b[1] & 0x3f) << 4) | (b[2] >> 4);
  else if (k == 2) v = ((uint32_t)(b[2] & 0x0f) << 6) | (b[3] >> 2);
  else v = ((uint32_t)(b[3] & 0x03) << 8) | b[4];
  return (double)v;
}

}  // namespace ldg
