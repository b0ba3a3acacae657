// Correctly rounded FP64 division by a constant without the divider: a product, one FMA for
// the residual and one FMA for the correction, in place of the ~12 VALU instructions (one
// of them a quarter-rate v_rcp_f64) of an IEEE division.
//
//   r = RN(1 / c);   q = RN(x r);   e = RN(x - c q) (exact);   x / c = RN(q + e r)
//
// Markstein's theorem (P. Markstein, "Computation of elementary functions on the IBM RISC
// System/6000 processor", IBM J. Res. Dev. 34, 1990; Muller et al., Handbook of
// Floating-Point Arithmetic, section 4.7): with r the correctly rounded reciprocal, q is a
// faithful quotient and the corrected one is RN(x / c), provided c's significand is not all
// ones (divconst_ok) and nothing under- or overflows: |x / c| and |x| 2^-53 stay normal
// numbers.  Every operand set in use is compared with `/` bit for bit by
// tests/test_divconst_host.py.
//
// Where the sequence and the division part ways: -0 / c is -0 but q + e r is +0 (e = +0), and
// inf / c is inf but e is NaN.  div_const returns q itself in both cases (and for a NaN x);
// div_const_nz is for operands that are finite and never -0, or whose zero's sign cannot
// reach a result (each call site says which).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDG_DIV_HD __host__ __device__ __forceinline__
#else
#define LDG_DIV_HD inline
#endif

namespace ldg {

// x / c for finite x that is not -0 (or whose sign of zero does not matter); r = 1 / c
LDG_DIV_HD double div_const_nz(double x, double c, double r) {
  const double q = x * r;
  const double e = __builtin_fma(-c, q, x);
  return __builtin_fma(e, r, q);
}

// x / c for any x: +-0, +-inf and NaN as the division gives them
LDG_DIV_HD double div_const(double x, double c, double r) {
  const double q = x * r;
  const double e = __builtin_fma(-c, q, x);
  // e is +-0 for an exact q (and for x = +-0: q carries the sign), NaN for x = +-inf or NaN
  return __builtin_islessgreater(e, 0.0) ? __builtin_fma(e, r, q) : q;
}

// The theorem's condition on the divisor: finite, normal, and a significand that is not all
// ones.  The host checks it for a divisor it prepares a reciprocal for (a context that fails
// it keeps the division).
inline bool divconst_ok(double c) {
  uint64_t u;
  memcpy(&u, &c, sizeof u);
  const uint64_t ex = (u >> 52) & 0x7ff, man = u & ((1ull << 52) - 1);
  return ex != 0 && ex != 0x7ff && man != ((1ull << 52) - 1);
}

}  // namespace ldg

#undef LDG_DIV_HD
