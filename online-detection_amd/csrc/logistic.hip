// The per-row terms of the weighted logistic loss (odx/logistic.py):  l(y, t) = c(y) log(1 + exp(-y t)),  c(+1) = 1,
// c(-1) = neg_weight, with its first and second derivatives in t.  One thread per row, all f64, no workspace.
//
// With z = y t and u = exp(-|z|) (one exponential, never above 1, so nothing overflows for any finite t):
//     sigma(-|z|) = u / (1 + u),   sigma(|z|) = 1 / (1 + u)
// are s = 1 / (1 + exp(z)) and 1 - s, the one or the other way round by the sign of z — each a quotient, neither a
// difference, so both keep their relative accuracy where the other is 1 to the last bit (and into the subnormals, where
// 1 / (1 + exp(z)) itself has already divided by infinity).  Then
//     l' = -c y s,   l'' = c s (1 - s),   l = c (max(-z, 0) + log1p(u)).
#include <math.h>

#include "odx_internal.h"

namespace odx {

__global__ __launch_bounds__(256) void logistic_rows_kernel(const double* __restrict__ t, const double* __restrict__ y, int64_t n,
                                                            double neg_weight, double* __restrict__ g, double* __restrict__ w,
                                                            double* __restrict__ l) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double yi = y[i];
  const double c = yi > 0.0 ? 1.0 : neg_weight;
  const double z = yi * t[i];
  const double u = exp(-fabs(z));
  const double den = 1.0 + u;
  const double lo = u / den, hi = 1.0 / den;      // sigma(-|z|), sigma(|z|)
  const double s = z > 0.0 ? lo : hi;             // 1 / (1 + exp(z))
  const double s1 = z > 0.0 ? hi : lo;            // 1 - s
  if (g != nullptr) g[i] = -(c * yi) * s;
  if (w != nullptr) w[i] = c * (s * s1);
  if (l != nullptr) l[i] = c * (fmax(-z, 0.0) + log1p(u));
}

}  // namespace odx

using namespace odx;

extern "C" int odx_logistic_rows_f64(const double* t, const double* y, int64_t n, double neg_weight, double* g, double* w,
                                     double* l, odx_stream_t stream) {
  ODX_REQUIRE(neg_weight > 0.0 && neg_weight < INFINITY, "odx_logistic_rows_f64: neg_weight must be positive and finite");
  if (n <= 0) return ODX_OK;
  ODX_REQUIRE(t && y, "odx_logistic_rows_f64: null t or y");
  ODX_REQUIRE(ceil_div(n, 256) <= 0x7fffffffLL, "odx_logistic_rows_f64: n = %lld is more than one launch takes", (long long)n);
  hipLaunchKernelGGL(logistic_rows_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, as_stream(stream), t, y, n, neg_weight,
                     g, w, l);
  ODX_CHECK_LAUNCH("odx_logistic_rows_f64");
  return ODX_OK;
}
