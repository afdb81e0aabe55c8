// The running log-sum-exp state (max, sum of exp(x - max)) that the held-out scores keep per entry (ysum.hip,
// ycond.hip).
#pragma once
#include <math.h>

namespace nmgp {

// (m, r) <- log-sum-exp state of two states: M = max, r = r1 exp(m1 - M) + r2 exp(m2 - M).  Two empty states
// (-inf, 0) stay empty (exp(-inf - -inf) would be NaN); a NaN in either makes both words NaN.
__device__ inline void y_lse_combine(double m1, double r1, double m2, double r2, double* m, double* r) {
  if (m1 != m1 || m2 != m2 || r1 != r1 || r2 != r2) {
    *m = *r = __builtin_nan("");
    return;
  }
  const double M = fmax(m1, m2);
  if (M == -INFINITY) {
    *m = -INFINITY;
    *r = 0.0;
    return;
  }
  *m = M;
  *r = r1 * exp(m1 - M) + r2 * exp(m2 - M);
}

}  // namespace nmgp
