// Device special functions shared by the elementwise functors
// (elementwise.hip) and the GLM reducers (glm.hip): one copy, included where
// it is called.  Internal linkage: every including file compiles its own.
#pragma once
#include <cmath>

#include <hip/hip_runtime.h>

namespace {

// ------------------------------------------------------ special functions
// digamma: boost::math::digamma, 53-bit path, policy errno_on_error -> NaN
// at poles (boost/math/special_functions/digamma.hpp:108-128, 300-347, 381-449;
// stan/math/prim/scal/fun/digamma.hpp:46-48, boost_policy.hpp)
__device__ double dev_digamma_large(double x) {
  const double P0 = 0.083333333333333333333333333333333333333333333333333,
               P1 = -0.0083333333333333333333333333333333333333333333333333,
               P2 = 0.003968253968253968253968253968253968253968253968254,
               P3 = -0.0041666666666666666666666666666666666666666666666667,
               P4 = 0.0075757575757575757575757575757575757575757575757576,
               P5 = -0.021092796092796092796092796092796092796092796092796,
               P6 = 0.083333333333333333333333333333333333333333333333333,
               P7 = -0.44325980392156862745098039215686274509803921568627;
  x -= 1;
  double result = log(x);
  result += 1 / (2 * x);
  const double z = 1 / (x * x);
  const double p = P0 + z * (P1 + z * (P2 + z * (P3 + z * (P4 + z * (P5 + z * (P6 + z * P7))))));
  result -= z * p;
  return result;
}

__device__ double dev_digamma_1_2(double x) {
  const double Y = (double)0.99558162689208984F;
  const double root1 = 1569415565.0 / 1073741824.0;
  const double root2 = (381566830.0 / 1073741824.0) / 1073741824.0;
  const double root3 = 0.9016312093258695918615325266959189453125e-19;
  double g = x - root1;
  g -= root2;
  g -= root3;
  const double t = x - 1;
  const double p = 0.25479851061131551 +
                   t * (-0.32555031186804491 +
                        t * (-0.65031853770896507 +
                             t * (-0.28919126444774784 +
                                  t * (-0.045251321448739056 + t * -0.0020713321167745952))));
  const double q =
      1.0 + t * (2.0767117023730469 +
                 t * (1.4606242909763515 +
                      t * (0.43593529692665969 +
                           t * (0.054151797245674225 +
                                t * (0.0021284987017821144 + t * -0.55789841321675513e-6)))));
  return g * Y + g * (p / q);
}

__device__ double dev_digamma(double x) {
  double result = 0;
  if (x <= -1) {
    // pi cot(pi (1 - x)) = -pi cot(pi r) with r = x - round(x) taken from x
    // itself (exact): 1 - x is rounded where it crosses a binade, and the
    // reference, which reduces after that, is off by |1 - x| 2^-53 pi^2 /
    // sin^2(pi x) near the poles
    const double r = x - round(x);
    if (r == 0) return __longlong_as_double(0x7ff8000000000000LL);
    result = -M_PI / tan(M_PI * r);
    x = 1 - x;
  }
  if (x == 0) return __longlong_as_double(0x7ff8000000000000LL);
  if (isnan(x)) return x;
  if (x >= 10) {
    result += dev_digamma_large(x);
  } else {
    while (x > 2) {
      x -= 1;
      result += 1 / x;
    }
    while (x < 1) {
      result -= 1 / x;
      x += 1;
    }
    result += dev_digamma_1_2(x);
  }
  return result;
}

// lgamma: the reference calls glibc lgamma_r (prim/scal/fun/lgamma.hpp:62-71);
// the device uses the ROCm libm lgamma (same function, <= a few ulp apart).
__device__ double dev_lgamma(double x) { return lgamma(x); }

}  // namespace
