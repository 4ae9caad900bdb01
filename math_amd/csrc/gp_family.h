// The covariance families of the GP path (smg_gp_family in smg_hip.h): what
// k_gp_* (gp.hip) and k_gp_inv_reduce / k_gp_inv_final (chol_mvn.hip) know
// about the kernel function.  With q the family's distance argument and c its
// length-scale coefficient (a = c q below):
//
//   family        q     c          K_ij (i != j)                 dK_ij/dl
//   exp_quad      d^2   1/(2 l^2)  s2 exp(-q c)                  K q / l^3
//   exponential   d     1/l        s2 exp(-a)                    K a / l
//   matern32      d     sqrt(3)/l  s2 (1 + a) exp(-a)            s2 a^2 exp(-a) / l
//   matern52      d     sqrt(5)/l  s2 (1 + a + a^2/3) exp(-a)    s2 a^2 (1 + a) exp(-a) / (3 l)
//
// d = |x_i - x_j| for D == 1 (no square root), sqrt of the squared distance
// otherwise.  No derivative divides by d: coincident points give K = s2 and a
// zero l-derivative.  exp_quad's members are the expressions the kernels had
// before they were templated (the same bits).
//
// One length scale per dimension (ARD, gp_ard.hip): the points are scaled
// first, z = x / l, and the kernels above run on z with c = coef(1).  With
// t_d = z_id - z_jd and a = c q:  dK_ij/dl_d = s2 h(a) t_d^2 / l_d,
//   h = exp(-q / 2) | exp(-a) / a (0 at a = 0) | 3 exp(-a) | (5/3)(1 + a) exp(-a).
#ifndef SMG_GP_FAMILY_H
#define SMG_GP_FAMILY_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "smg_hip.h"

template <int F>
struct gp_fam;

inline bool gp_family_ok(int family) { return family >= SMG_GP_EXP_QUAD && family <= SMG_GP_MATERN52; }

// fn(F) with the family as a compile-time constant (gp_fam<F()>); exp_quad for any other value
template <class Fn>
auto gp_with_family(int family, Fn&& fn) {
  switch (family) {
    case SMG_GP_EXPONENTIAL: return fn(std::integral_constant<int, SMG_GP_EXPONENTIAL>());
    case SMG_GP_MATERN32: return fn(std::integral_constant<int, SMG_GP_MATERN32>());
    case SMG_GP_MATERN52: return fn(std::integral_constant<int, SMG_GP_MATERN52>());
    default: return fn(std::integral_constant<int, SMG_GP_EXP_QUAD>());
  }
}

// The grid of the rectangular walks over an n1 x n2 K (gp.hip's k_gp_rect_*,
// gp_ard.hip's cross reverse): one workgroup per column up to GP_BLOCKS (the
// column loop wraps beyond), times as many row parts as bring the grid to about
// GP_BLOCKS workgroups, none of them without rows; rows: what a workgroup
// covers in one pass.
constexpr int GP_BLOCKS = 2048;
inline dim3 cross_grid(int n1, int n2, int rows) {
  const int gx = n2 < GP_BLOCKS ? n2 : GP_BLOCKS;
  int gy = (int)(((long long)n1 + rows - 1) / rows);
  if (gy > GP_BLOCKS / gx) gy = GP_BLOCKS / gx;
  return dim3(gx, gy < 1 ? 1 : gy);
}

template <>
struct gp_fam<SMG_GP_EXP_QUAD> {
  static double coef(double l) { return 0.5 / (l * l); }
  static __device__ __forceinline__ double from_diff(double d) { return d * d; }
  static __device__ __forceinline__ double from_sq(double d2) { return d2; }
  static __device__ __forceinline__ double k(double q, double s2, double c) { return s2 * exp(-q * c); }
  // the reverse's terms of one position with adjoint a: as += a K, al += (l-scaled) a dK/dl
  static __device__ __forceinline__ void acc(double a, double q, double s2, double c, double& as, double& al) {
    const double prod = a * (s2 * exp(-q * c));
    al += prod * q;
    as += prod;
  }
  // dK/dl = K w(q) scaled by lscale: the fused reducer's weight (it reads K)
  static __device__ __forceinline__ double w(double q, double c) { return q; }
  static __device__ __forceinline__ double lscale(double sl, double l) { return sl / (l * l * l); }
  // ARD (q from z = x / l, c = coef(1)): dK/dl_d = s2 h t_d^2 / l_d
  static __device__ __forceinline__ double h(double q, double c) { return exp(-q * c); }
};

template <>
struct gp_fam<SMG_GP_EXPONENTIAL> {
  static double coef(double l) { return 1.0 / l; }
  static __device__ __forceinline__ double from_diff(double d) { return fabs(d); }
  static __device__ __forceinline__ double from_sq(double d2) { return sqrt(d2); }
  static __device__ __forceinline__ double k(double q, double s2, double c) { return s2 * exp(-(q * c)); }
  static __device__ __forceinline__ void acc(double a, double q, double s2, double c, double& as, double& al) {
    const double t = q * c;
    const double prod = a * (s2 * exp(-t));
    al += prod * t;
    as += prod;
  }
  static __device__ __forceinline__ double w(double q, double c) { return q * c; }
  static __device__ __forceinline__ double lscale(double sl, double l) { return sl / l; }
  // (the one h that divides by a: t_d^2 / a -> 0 with the distance, 0 at a coincident pair)
  static __device__ __forceinline__ double h(double q, double c) {
    const double t = q * c;
    return t > 0.0 ? exp(-t) / t : 0.0;
  }
};

template <>
struct gp_fam<SMG_GP_MATERN32> {
  static double coef(double l) { return sqrt(3.0) / l; }
  static __device__ __forceinline__ double from_diff(double d) { return fabs(d); }
  static __device__ __forceinline__ double from_sq(double d2) { return sqrt(d2); }
  static __device__ __forceinline__ double k(double q, double s2, double c) {
    const double t = q * c;
    return s2 * ((1.0 + t) * exp(-t));
  }
  static __device__ __forceinline__ void acc(double a, double q, double s2, double c, double& as, double& al) {
    const double t = q * c;
    const double e = a * (s2 * exp(-t));
    al += e * (t * t);
    as += e * (1.0 + t);
  }
  static __device__ __forceinline__ double w(double q, double c) {
    const double t = q * c;
    return t * t / (1.0 + t);
  }
  static __device__ __forceinline__ double lscale(double sl, double l) { return sl / l; }
  static __device__ __forceinline__ double h(double q, double c) { return 3.0 * exp(-(q * c)); }
};

template <>
struct gp_fam<SMG_GP_MATERN52> {
  static double coef(double l) { return sqrt(5.0) / l; }
  static __device__ __forceinline__ double from_diff(double d) { return fabs(d); }
  static __device__ __forceinline__ double from_sq(double d2) { return sqrt(d2); }
  static __device__ __forceinline__ double k(double q, double s2, double c) {
    const double t = q * c;
    return s2 * ((1.0 + t + t * t * (1.0 / 3.0)) * exp(-t));
  }
  static __device__ __forceinline__ void acc(double a, double q, double s2, double c, double& as, double& al) {
    const double t = q * c;
    const double e = a * (s2 * exp(-t));
    al += e * (t * t * (1.0 + t));
    as += e * (1.0 + t + t * t * (1.0 / 3.0));
  }
  static __device__ __forceinline__ double w(double q, double c) {
    const double t = q * c;
    return t * t * (1.0 + t) / (1.0 + t + t * t * (1.0 / 3.0));
  }
  static __device__ __forceinline__ double lscale(double sl, double l) { return sl / (3.0 * l); }
  static __device__ __forceinline__ double h(double q, double c) {
    const double t = q * c;
    return (5.0 / 3.0) * ((1.0 + t) * exp(-t));
  }
};

#endif
