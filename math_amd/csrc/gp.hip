// gp_exp_quad_cov and add_diag, forward and reverse.
//
// gp_exp_quad_cov(std::vector<double> x, var sigma, var l)
//   rev/mat/fun/gp_exp_quad_cov.hpp:64-94 (forward), :96-112 (chain)
// The reference stores the N(N-1)/2 lower entries once and aliases the upper
// triangle to them (:233-238), so the adjoint of each lower vari is the sum of
// the adjoints of positions (i,j) and (j,i).  Here the node keeps the full
// N x N adjoint and the reverse kernel sweeps every position once (coalesced),
// which sums exactly those pairs:
//   d/dl     = sum_{i != j} Kadj_ij K_ij d_ij^2 / l^3
//   d/dsigma = 2/sigma (sum_{i != j} Kadj_ij K_ij + sum_i Kadj_ii sigma^2)
// K_ij is recomputed from x instead of re-read (HBM: one read of Kadj).
// Reductions are fixed-order (per-block partials + one ordered pass).
//
// The forward and reverse kernels are templated on the covariance family
// (gp_family.h: exp_quad, exponential, Matern 3/2 and 5/2); their argument
// inv_half_sq_l is the family's length-scale coefficient, 1 / (2 l^2) for
// exp_quad.  The tangent kernels are exp_quad's alone.
//
// Everything rectangular -- the cross-covariance K(x1, x2) of the four families
// (smg_gp_cross_cov_fwd / _rev), gp_periodic_cov and gp_dot_prod_cov, square and
// cross -- is one walk over an n1 x n2 rectangle, without the diagonal
// (k_gp_rect_*), instantiated with three pair laws (gp_stat_law<F>, gp_per_law,
// gp_dot_law) and launched by rect_fwd / rect_rev.  Its final pass
// k_gp_rect_final is the square reverse's too.
//
// add_diag: prim/mat/fun/add_diag.hpp:20-55.
#include "smg_internal.h"
#include "gp_family.h"

namespace {

template <int F>
__global__ __launch_bounds__(256) void k_gp_fwd(const double* __restrict__ x, int n, double s2,
                                                double inv_half_sq_l, double* __restrict__ K,
                                                int ldk) {
  // 2D: blockIdx.y over columns j, x-dim over rows i (coalesced stores)
  const int j = blockIdx.y;
  const double xj = x[j];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double v;
    if (i == j) {
      v = s2;
    } else {
      const double d = (i > j) ? x[i] - xj : xj - x[i];
      v = gp_fam<F>::k(gp_fam<F>::from_diff(d), s2, inv_half_sq_l);
    }
    K[i + (size_t)j * ldk] = v;
  }
}

template <int F>
__global__ __launch_bounds__(256) void k_gp_rev_partials(const double* __restrict__ x, int n,
                                                         double s2, double inv_half_sq_l,
                                                         const double* __restrict__ Ka, int lda,
                                                         double* __restrict__ part) {
  __shared__ double lds[16];
  double al = 0.0, as = 0.0;
  for (smg_mn it(n, n); it.ok(); it.next()) {
    const long long e = it.e;
    const int i = it.i, j = it.j;
    const double a = Ka[i + (size_t)j * lda];
    if (i == j) {
      as += a * s2;
    } else {
      const double d = (i > j) ? x[i] - x[j] : x[j] - x[i];
      gp_fam<F>::acc(a, gp_fam<F>::from_diff(d), s2, inv_half_sq_l, as, al);
    }
  }
  const double sl = block_sum(al, lds);
  __syncthreads();
  const double ss = block_sum(as, lds);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x + 0] = ss;
    part[2 * blockIdx.x + 1] = sl;
  }
}

// k_gp_rev_partials in the column form (16-byte reads of Kadj and x; a
// workgroup walks whole columns); the same per-element terms, fixed order.
template <int F>
__global__ __launch_bounds__(256) void k_gp_rev_partials_col2(const double* __restrict__ x, int n,
                                                              double s2, double inv_half_sq_l,
                                                              const double* __restrict__ Ka,
                                                              int lda, double* __restrict__ part) {
  __shared__ double lds[16];
  const int np = n >> 1;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  double al = 0.0, as = 0.0;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    const double xj = x[j];
    const double2* col = reinterpret_cast<const double2*>(Ka + (size_t)j * lda);
    for (int p0 = threadIdx.x; p0 < np; p0 += 4 * 256) {
      double2 a[4], xi[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          a[k] = col[p];
          xi[k] = x2[p];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          const int i = 2 * p;
          const double av[2] = {a[k].x, a[k].y}, xv[2] = {xi[k].x, xi[k].y};
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (i + h == j) {
              as += av[h] * s2;
            } else {
              const double d = (i + h > j) ? xv[h] - xj : xj - xv[h];
              gp_fam<F>::acc(av[h], gp_fam<F>::from_diff(d), s2, inv_half_sq_l, as, al);
            }
          }
        }
      }
    }
  }
  const double sl = block_sum(al, lds);
  __syncthreads();
  const double ss = block_sum(as, lds);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x + 0] = ss;
    part[2 * blockIdx.x + 1] = sl;
  }
}

__global__ void k_add_diag_fwd(const double* __restrict__ A, int lda, int n, double d,
                               const double* __restrict__ dv, double* __restrict__ B, int ldb) {
  for (smg_mn it(n, n); it.ok(); it.next()) {
    const long long e = it.e;
    const int i = it.i, j = it.j;
    double v = A[i + (size_t)j * lda];
    if (i == j) v += dv ? dv[i] : d;
    B[i + (size_t)j * ldb] = v;
  }
}

// Column forms of k_gp_fwd / k_add_diag_fwd for 16-byte aligned operands with
// even n and leading dimensions (the N=4096 GP): a workgroup walks whole
// columns, each lane moves two rows with one 16-byte access, four accesses in
// flight per lane.  Same per-element expressions as above (the same bits).
template <int F>
__global__ __launch_bounds__(256) void k_gp_fwd_col2(const double* __restrict__ x, int n, double s2,
                                                     double inv_half_sq_l, double* __restrict__ K,
                                                     int ldk) {
  const int np = n >> 1;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    const double xj = x[j];
    double2* col = reinterpret_cast<double2*>(K + (size_t)j * ldk);
    for (int p0 = threadIdx.x; p0 < np; p0 += 4 * 256) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          const double2 xi = x2[p];
          const int i = 2 * p;
          double2 v;
          if (i == j) {
            v.x = s2;
          } else {
            const double d = (i > j) ? xi.x - xj : xj - xi.x;
            v.x = gp_fam<F>::k(gp_fam<F>::from_diff(d), s2, inv_half_sq_l);
          }
          if (i + 1 == j) {
            v.y = s2;
          } else {
            const double d = (i + 1 > j) ? xi.y - xj : xj - xi.y;
            v.y = gp_fam<F>::k(gp_fam<F>::from_diff(d), s2, inv_half_sq_l);
          }
          col[p] = v;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_add_diag_fwd_col2(const double* __restrict__ A, int lda,
                                                           int n, double d,
                                                           const double* __restrict__ dv,
                                                           double* __restrict__ B, int ldb) {
  const int np = n >> 1;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    const double2* a = reinterpret_cast<const double2*>(A + (size_t)j * lda);
    double2* b = reinterpret_cast<double2*>(B + (size_t)j * ldb);
    const double dj = dv ? dv[j] : d;
    for (int p0 = threadIdx.x; p0 < np; p0 += 4 * 256) {
      double2 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) v[k] = a[p];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          if (2 * p == j) v[k].x += dj;
          if (2 * p + 1 == j) v[k].y += dj;
          b[p] = v[k];
        }
      }
    }
  }
}

// Both column forms need 16-byte aligned columns.
inline bool col2_ok(const void* p, int ld, int n) {
  return ((reinterpret_cast<uintptr_t>(p) & 15) == 0) && (ld % 2 == 0) && (n % 2 == 0);
}

// Y += X over whole columns, 16-byte accesses (add_diag's reverse, A's adjoint)
__global__ __launch_bounds__(256) void k_add_full_col2(const double* __restrict__ X, int ldx, int n,
                                                       double* __restrict__ Y, int ldy) {
  const int np = n >> 1;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    const double2* x = reinterpret_cast<const double2*>(X + (size_t)j * ldx);
    double2* y = reinterpret_cast<double2*>(Y + (size_t)j * ldy);
    for (int p0 = threadIdx.x; p0 < np; p0 += 4 * 256) {
      double2 a[4], b[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          a[k] = x[p];
          b[k] = y[p];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          b[k].x += a[k].x;
          b[k].y += a[k].y;
          y[p] = b[k];
        }
      }
    }
  }
}

__global__ void k_add_full(const double* __restrict__ X, int ldx, int n, double* __restrict__ Y,
                           int ldy) {
  for (smg_mn it(n, n); it.ok(); it.next()) {
    const long long e = it.e;
    const int i = it.i, j = it.j;
    Y[i + (size_t)j * ldy] += X[i + (size_t)j * ldx];
  }
}

__global__ void k_diag_adj(const double* __restrict__ Ba, int ldb, int n, double* dadj, int vec) {
  __shared__ double lds[16];
  if (vec) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dadj[i] += Ba[i + (size_t)i * ldb];
    return;
  }
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += Ba[i + (size_t)i * ldb];
  s = block_sum(s, lds);
  if (threadIdx.x == 0) dadj[0] += s;
}

// Tangent of K along (sigma', l') -- the fvar<var> instantiation of the same
// covariance (prim/mat/fun/gp_exp_quad_cov.hpp:40-59 over fvar, used by
// hessian_times_vector):  Kd_ij = 2 sigma sigma' e + sigma^2 l' d^2 e / l^3,
// e = exp(-d^2 / (2 l^2)); Kd_ii = 2 sigma sigma'.
__global__ __launch_bounds__(256) void k_gp_tan_fwd(const double* __restrict__ x, int n, double a,
                                                    double b, double inv_half_sq_l,
                                                    double* __restrict__ K, int ldk) {
  // a = 2 sigma sigma', b = sigma^2 l' / l^3
  const int j = blockIdx.y;
  const double xj = x[j];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double v;
    if (i == j) {
      v = a;
    } else {
      const double d = (i > j) ? x[i] - xj : xj - x[i];
      const double d2 = d * d;
      const double e = exp(-d2 * inv_half_sq_l);
      v = a * e + b * d2 * e;
    }
    K[i + (size_t)j * ldk] = v;
  }
}

// per-block partials of S_e = sum A e, S_2 = sum A e d^2, S_4 = sum A e d^4 (all positions)
__global__ __launch_bounds__(256) void k_gp_tan_partials(const double* __restrict__ x, int n,
                                                         double inv_half_sq_l,
                                                         const double* __restrict__ Ka, int lda,
                                                         double* __restrict__ part) {
  __shared__ double lds[16];
  double se = 0.0, s2 = 0.0, s4 = 0.0;
  const long long tot = (long long)n * n;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < tot;
       q += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(q / n), i = (int)(q % n);
    const double a = Ka[i + (size_t)j * lda];
    if (i == j) {
      se += a;
    } else {
      const double d = (i > j) ? x[i] - x[j] : x[j] - x[i];
      const double d2 = d * d;
      const double ae = a * exp(-d2 * inv_half_sq_l);
      se += ae;
      s2 += ae * d2;
      s4 += ae * d2 * d2;
    }
  }
  se = block_sum(se, lds);
  __syncthreads();
  s2 = block_sum(s2, lds);
  __syncthreads();
  s4 = block_sum(s4, lds);
  if (threadIdx.x == 0) {
    part[3 * blockIdx.x + 0] = se;
    part[3 * blockIdx.x + 1] = s2;
    part[3 * blockIdx.x + 2] = s4;
  }
}

__global__ void k_gp_tan_final(const double* __restrict__ part, int nparts, double sigma, double l,
                               double ds, double dl, double* out4) {
  __shared__ double lds[16];
  double se = 0.0, s2 = 0.0, s4 = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    se += part[3 * i];
    s2 += part[3 * i + 1];
    s4 += part[3 * i + 2];
  }
  se = block_sum(se, lds);
  __syncthreads();
  s2 = block_sum(s2, lds);
  __syncthreads();
  s4 = block_sum(s4, lds);
  if (threadIdx.x == 0) {
    const double l3 = l * l * l, l4 = l3 * l, l6 = l3 * l3;
    out4[0] += 2 * ds * se + 2 * sigma * dl * s2 / l3;                                  // d/dsigma
    out4[1] += 2 * sigma * ds * s2 / l3 + sigma * sigma * dl * (s4 / l6 - 3 * s2 / l4);  // d/dl
    out4[2] += 2 * sigma * se;                                                          // d/dsigma'
    out4[3] += sigma * sigma * s2 / l3;                                                 // d/dl'
  }
}


// D-dimensional inputs (gp_exp_quad_cov(std::vector<T_x> x, ...) with T_x an
// Eigen vector, rev/mat/fun/gp_exp_quad_cov.hpp:158-184,211-242): x is D x n
// column-major (point i at x + i D), d_ij^2 = squared_distance(x_i, x_j)
// summed over the D coordinates in order.  A workgroup walks whole columns j;
// x_j is staged in LDS, the row points are read from L2 (x is n D doubles).
template <int F>
__global__ __launch_bounds__(256) void k_gp_nd_fwd(const double* __restrict__ x, int D, int n, double s2,
                                                   double inv_half_sq_l, double* __restrict__ K, int ldk) {
  extern __shared__ double xj[];
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += blockDim.x) xj[d] = x[(size_t)j * D + d];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      double v = s2;
      if (i != j) {
        const double* xi = x + (size_t)i * D;
        double d2 = 0.0;
        for (int d = 0; d < D; ++d) {
          const double t = xi[d] - xj[d];
          d2 += t * t;
        }
        v = gp_fam<F>::k(gp_fam<F>::from_sq(d2), s2, inv_half_sq_l);
      }
      K[i + (size_t)j * ldk] = v;
    }
  }
}

template <int F>
__global__ __launch_bounds__(256) void k_gp_nd_rev_partials(const double* __restrict__ x, int D, int n, double s2,
                                                            double inv_half_sq_l, const double* __restrict__ Ka,
                                                            int lda, double* __restrict__ part) {
  extern __shared__ double xj[];
  __shared__ double lds[16];
  double al = 0.0, as = 0.0;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += blockDim.x) xj[d] = x[(size_t)j * D + d];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const double a = Ka[i + (size_t)j * lda];
      if (i == j) {
        as += a * s2;
      } else {
        const double* xi = x + (size_t)i * D;
        double d2 = 0.0;
        for (int d = 0; d < D; ++d) {
          const double t = xi[d] - xj[d];
          d2 += t * t;
        }
        gp_fam<F>::acc(a, gp_fam<F>::from_sq(d2), s2, inv_half_sq_l, as, al);
      }
    }
  }
  const double sl = block_sum(al, lds);
  __syncthreads();
  const double ss = block_sum(as, lds);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x + 0] = ss;
    part[2 * blockIdx.x + 1] = sl;
  }
}

// The rectangular walk: K(x1, x2), n1 x n2, and its reverse, for every
// covariance with rectangular entries (smg_gp_cross_cov_*, the four stationary
// families; smg_gp_periodic_cov_* and smg_gp_dot_prod_cov_*, whose square
// K(x, x) is x1 == x2).  It is written once, over a pair law passed by value
// that carries its own scalars and provides what the walk cannot know:
//   q1(xi, xj)      the law's argument q of a pair of scalar points (D == 1)
//   step(acc, a, b) one coordinate's term of the D > 1 sum, in coordinate order
//   qn(acc)         q from that sum
//   k(q)            the element
//   NS, acc(a, q, sum)   the reverse's NS sums, and one adjoint entry's terms
//   finish(sum, out)     the last line of the final pass
// Every position alike, no diagonal branch: a coincident pair gives the
// diagonal's value exactly, and the sign of a difference drops out of q (the
// products of the dot law commute), so x1 == x2 gives a bitwise symmetric K.

// (both distance laws: the squared distance, coordinate by coordinate)
struct gp_sq_dist {
  static __device__ __forceinline__ void step(double& acc, double a, double b) {
    const double t = a - b;
    acc += t * t;
  }
};

// Stationary (gp_fam<F>): q and the terms of gp_family.h; the bits of k_gp_fwd*
// when x1 == x2.
template <int F>
struct gp_stat_law : gp_sq_dist {
  static constexpr int NS = 2;             // [sum Kadj K, l-scaled sum Kadj dK/dl]
  static constexpr bool RED_DESC = true;   // (the block reduction takes the l sum first)
  double s2, c, sigma, l;
  gp_stat_law(double sigma_, double l_) : s2(sigma_ * sigma_), c(gp_fam<F>::coef(l_)), sigma(sigma_), l(l_) {}
  __device__ __forceinline__ double q1(double xi, double xj) const { return gp_fam<F>::from_diff(xi - xj); }
  __device__ __forceinline__ double qn(double d2) const { return gp_fam<F>::from_sq(d2); }
  __device__ __forceinline__ double k(double q) const { return gp_fam<F>::k(q, s2, c); }
  __device__ __forceinline__ void acc(double a, double q, double* sum) const {
    gp_fam<F>::acc(a, q, s2, c, sum[0], sum[1]);
  }
  __device__ __forceinline__ void finish(const double* sum, double* out) const {
    out[0] += sum[0] * 2 / sigma;              // :110
    out[1] += gp_fam<F>::lscale(sum[1], l);    // exp_quad: sl / l^3 (:109)
  }
};

// Periodic (gp_periodic_cov, Stan Math 3.0.0 prim/mat/fun/), q = d, a = pi d / p:
//   K = s2 exp(-2 sin^2(a) / l^2),  dK/dsigma = 2 K / sigma,
//   dK/dl = K 4 sin^2(a) / l^3,  dK/dp = K (2 pi d / (l^2 p^2)) sin(2a).
// sin(a) and cos(a) come from one sincospi(d / p) (the forward needs sinpi
// alone), d / p as d times the host's 1 / p: exact argument reduction, so a
// pair a whole number of periods apart gives s2 when d / p is exact, and
// sin(2a) = 2 sin cos.
struct gp_per_law : gp_sq_dist {
  static constexpr int NS = 3;  // sums of a K, a K sin^2, a K d sin cos
  static constexpr bool RED_DESC = false;
  double s2, inv_p, cn, sigma, l, p;  // cn = -2 / l^2
  gp_per_law(double sigma_, double l_, double p_)
      : s2(sigma_ * sigma_), inv_p(1.0 / p_), cn(-2.0 / (l_ * l_)), sigma(sigma_), l(l_), p(p_) {}
  __device__ __forceinline__ double q1(double xi, double xj) const { return fabs(xi - xj); }
  __device__ __forceinline__ double qn(double d2) const { return sqrt(d2); }
  __device__ __forceinline__ double k(double d) const {
    const double s = sinpi(d * inv_p);
    return s2 * exp(cn * (s * s));
  }
  __device__ __forceinline__ void acc(double a, double d, double* sum) const {
    double s, c;
    sincospi(d * inv_p, &s, &c);
    const double ss = s * s;
    const double ak = a * (s2 * exp(cn * ss));
    sum[0] += ak;
    sum[1] += ak * ss;
    sum[2] += ak * (d * (s * c));
  }
  // out3 += [2 ss / sigma, 4 sl / l^3, 4 pi sp / (l^2 p^2)] (sp carries sin cos = sin(2a) / 2)
  __device__ __forceinline__ void finish(const double* sum, double* out) const {
    out[0] += sum[0] * 2 / sigma;
    out[1] += 4 * sum[1] / (l * l * l);
    out[2] += 4 * 3.14159265358979323846 * sum[2] / (l * l * p * p);
  }
};

// Dot product (gp_dot_prod_cov): K_ij = sigma^2 + sum_d x1_id x2_jd, q the sum
// of products; dK/dsigma = 2 sigma, so the reverse is the sum of the adjoint
// and reads no points (k_gp_dot_rev_partials* below, not the walk's acc).
struct gp_dot_law {
  static constexpr int NS = 1;
  static constexpr bool RED_DESC = false;
  double s2, sigma;
  explicit gp_dot_law(double sigma_) : s2(sigma_ * sigma_), sigma(sigma_) {}
  __device__ __forceinline__ double q1(double xi, double xj) const { return xi * xj; }
  static __device__ __forceinline__ void step(double& acc, double a, double b) { acc += a * b; }
  __device__ __forceinline__ double qn(double dot) const { return dot; }
  __device__ __forceinline__ double k(double dot) const { return s2 + dot; }
  __device__ __forceinline__ void finish(const double* sum, double* out) const { out[0] += 2 * sigma * sum[0]; }
};

// The walk of k_gp_fwd_col2 / k_gp_nd_fwd over the rectangle: a workgroup walks
// whole columns j (x2_j in a register for D == 1, staged in LDS otherwise), its
// lanes consecutive rows i of x1.  The grid's y dimension splits the rows
// (blockIdx.y takes every gridDim.y-th pass of a workgroup's rows), so that a
// tall K with few columns still fills the chip; it is 1 once the columns alone
// give GP_BLOCKS workgroups (cross_grid, gp_family.h).
//
// Column form: 16-byte aligned x1 and columns, even n1 and ldk (col2_ok)
template <class Law>
__global__ __launch_bounds__(256) void k_gp_rect_fwd_col2(Law law, const double* __restrict__ x1, int n1,
                                                          const double* __restrict__ x2, int n2,
                                                          double* __restrict__ K, int ldk) {
  const int np = n1 >> 1;
  const double2* xr = reinterpret_cast<const double2*>(x1);
  for (int j = blockIdx.x; j < n2; j += gridDim.x) {
    const double xj = x2[j];
    double2* col = reinterpret_cast<double2*>(K + (size_t)j * ldk);
    for (int p0 = blockIdx.y * (4 * 256) + threadIdx.x; p0 < np; p0 += gridDim.y * (4 * 256)) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          const double2 xi = xr[p];
          double2 v;
          v.x = law.k(law.q1(xi.x, xj));
          v.y = law.k(law.q1(xi.y, xj));
          col[p] = v;
        }
      }
    }
  }
}

// Generic form: any n1 and ldk (rows n1 .. ldk - 1 are not written)
template <class Law>
__global__ __launch_bounds__(256) void k_gp_rect_fwd(Law law, const double* __restrict__ x1, int n1,
                                                     const double* __restrict__ x2, int n2, double* __restrict__ K,
                                                     int ldk) {
  for (int j = blockIdx.x; j < n2; j += gridDim.x) {
    const double xj = x2[j];
    double* col = K + (size_t)j * ldk;
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n1; i += gridDim.y * 256) col[i] = law.k(law.q1(x1[i], xj));
  }
}

template <class Law>
__global__ __launch_bounds__(256) void k_gp_rect_nd_fwd(Law law, const double* __restrict__ x1, int n1,
                                                        const double* __restrict__ x2, int n2, int D,
                                                        double* __restrict__ K, int ldk) {
  extern __shared__ double xj[];
  for (int j = blockIdx.x; j < n2; j += gridDim.x) {
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += blockDim.x) xj[d] = x2[(size_t)j * D + d];
    __syncthreads();
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n1; i += gridDim.y * 256) {
      const double* xi = x1 + (size_t)i * D;
      double acc = 0.0;
      for (int d = 0; d < D; ++d) Law::step(acc, xi[d], xj[d]);
      K[i + (size_t)j * ldk] = law.k(law.qn(acc));
    }
  }
}

// A workgroup's NS sums -> part[NS b ..], b its place in the grid
template <int NS, bool RED_DESC>
__device__ __forceinline__ void rect_store_partials(const double* sum, double* lds, double* __restrict__ part) {
  double tot[NS];
#pragma unroll
  for (int r = 0; r < NS; ++r) {
    const int s = RED_DESC ? NS - 1 - r : r;
    if (r) __syncthreads();
    tot[s] = block_sum(sum[s], lds);
  }
  if (threadIdx.x == 0) {
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
    for (int s = 0; s < NS; ++s) part[NS * b + s] = tot[s];
  }
}

// The reverse's per-workgroup partials over the same walks (one read of Kadj,
// K recomputed); k_gp_rect_final sums them.
template <class Law>
__global__ __launch_bounds__(256) void k_gp_rect_rev_partials_col2(Law law, const double* __restrict__ x1, int n1,
                                                                   const double* __restrict__ x2, int n2,
                                                                   const double* __restrict__ Ka, int lda,
                                                                   double* __restrict__ part) {
  __shared__ double lds[16];
  const int np = n1 >> 1;
  const double2* xr = reinterpret_cast<const double2*>(x1);
  double sum[Law::NS];
#pragma unroll
  for (int s = 0; s < Law::NS; ++s) sum[s] = 0.0;
  for (int j = blockIdx.x; j < n2; j += gridDim.x) {
    const double xj = x2[j];
    const double2* col = reinterpret_cast<const double2*>(Ka + (size_t)j * lda);
    for (int p0 = blockIdx.y * (4 * 256) + threadIdx.x; p0 < np; p0 += gridDim.y * (4 * 256)) {
      double2 a[4], xi[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          a[k] = col[p];
          xi[k] = xr[p];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          law.acc(a[k].x, law.q1(xi[k].x, xj), sum);
          law.acc(a[k].y, law.q1(xi[k].y, xj), sum);
        }
      }
    }
  }
  rect_store_partials<Law::NS, Law::RED_DESC>(sum, lds, part);
}

// Generic form, D >= 1 (x2_j staged in LDS as k_gp_rect_nd_fwd does; D == 1 from the two scalars)
template <class Law>
__global__ __launch_bounds__(256) void k_gp_rect_rev_partials(Law law, const double* __restrict__ x1, int n1,
                                                              const double* __restrict__ x2, int n2, int D,
                                                              const double* __restrict__ Ka, int lda,
                                                              double* __restrict__ part) {
  extern __shared__ double xj[];
  __shared__ double lds[16];
  double sum[Law::NS];
#pragma unroll
  for (int s = 0; s < Law::NS; ++s) sum[s] = 0.0;
  for (int j = blockIdx.x; j < n2; j += gridDim.x) {
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += blockDim.x) xj[d] = x2[(size_t)j * D + d];
    __syncthreads();
    const double* col = Ka + (size_t)j * lda;
    const double xj0 = xj[0];
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n1; i += gridDim.y * 256) {
      const double a = col[i];
      if (D == 1) {
        law.acc(a, law.q1(x1[i], xj0), sum);
      } else {
        const double* xi = x1 + (size_t)i * D;
        double acc = 0.0;
        for (int d = 0; d < D; ++d) Law::step(acc, xi[d], xj[d]);
        law.acc(a, law.qn(acc), sum);
      }
    }
  }
  rect_store_partials<Law::NS, Law::RED_DESC>(sum, lds, part);
}

// The dot product's reverse partials: per-workgroup sums of the n1 x n2 adjoint over the same walks
__global__ __launch_bounds__(256) void k_gp_dot_rev_partials_col2(int n1, int n2, const double* __restrict__ Ka,
                                                                  int lda, double* __restrict__ part) {
  __shared__ double lds[16];
  const int np = n1 >> 1;
  double as = 0.0;
  for (int j = blockIdx.x; j < n2; j += gridDim.x) {
    const double2* col = reinterpret_cast<const double2*>(Ka + (size_t)j * lda);
    for (int p0 = blockIdx.y * (4 * 256) + threadIdx.x; p0 < np; p0 += gridDim.y * (4 * 256)) {
      double2 a[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        a[k] = p < np ? col[p] : make_double2(0.0, 0.0);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) as += a[k].x + a[k].y;
    }
  }
  rect_store_partials<1, false>(&as, lds, part);
}

__global__ __launch_bounds__(256) void k_gp_dot_rev_partials(int n1, int n2, const double* __restrict__ Ka, int lda,
                                                             double* __restrict__ part) {
  __shared__ double lds[16];
  double as = 0.0;
  for (int j = blockIdx.x; j < n2; j += gridDim.x) {
    const double* col = Ka + (size_t)j * lda;
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n1; i += gridDim.y * 256) as += col[i];
  }
  rect_store_partials<1, false>(&as, lds, part);
}

// The one ordered pass over the partials (the square reverse's too): out += law.finish(sums)
template <class Law>
__global__ void k_gp_rect_final(Law law, const double* __restrict__ part, int nparts, double* out) {
  __shared__ double lds[16];
  double sum[Law::NS];
#pragma unroll
  for (int s = 0; s < Law::NS; ++s) sum[s] = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
#pragma unroll
    for (int s = 0; s < Law::NS; ++s) sum[s] += part[Law::NS * i + s];
  }
#pragma unroll
  for (int s = 0; s < Law::NS; ++s) {
    if (s) __syncthreads();
    sum[s] = block_sum(sum[s], lds);
  }
  if (threadIdx.x == 0) law.finish(sum, out);
}

// K(x1, x2) of a law for checked arguments, n1, n2 > 0: the LDS-staged form for
// D > 1, the column form for aligned scalar points, the generic form otherwise
template <class Law>
int rect_fwd(smg_ctx* ctx, const Law& law, const double* x1, int n1, const double* x2, int n2, int D, double* K,
             int ldk) {
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  if (D > 1)
    hipLaunchKernelGGL(k_gp_rect_nd_fwd<Law>, cross_grid(n1, n2, 256), dim3(256), D * sizeof(double), ctx->stream, law,
                       x1, n1, x2, n2, D, K, ldk);
  else if (col2_ok(x1, 2, n1) && col2_ok(K, ldk, n1))
    hipLaunchKernelGGL(k_gp_rect_fwd_col2<Law>, cross_grid(n1, n2, 8 * 256), dim3(256), 0, ctx->stream, law, x1, n1, x2,
                       n2, K, ldk);
  else
    hipLaunchKernelGGL(k_gp_rect_fwd<Law>, cross_grid(n1, n2, 256), dim3(256), 0, ctx->stream, law, x1, n1, x2, n2, K,
                       ldk);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

// out += the law's hyperparameter derivatives of K(x1, x2) from its adjoint (same forms)
template <class Law>
int rect_rev(smg_ctx* ctx, const Law& law, const double* x1, int n1, const double* x2, int n2, int D,
             const double* Kadj, int ldka, double* out) {
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  const bool col2 = D == 1 && col2_ok(x1, 2, n1) && col2_ok(Kadj, ldka, n1);
  const dim3 grid = cross_grid(n1, n2, col2 ? 8 * 256 : 256);
  const int nb = (int)(grid.x * grid.y);
  double* part = smg_ws(ctx, SMG_WS_RED, Law::NS * (size_t)nb);
  if (!part) return SMG_ERR_OOM;
  if (col2)
    hipLaunchKernelGGL(k_gp_rect_rev_partials_col2<Law>, grid, dim3(256), 0, ctx->stream, law, x1, n1, x2, n2, Kadj,
                       ldka, part);
  else
    hipLaunchKernelGGL(k_gp_rect_rev_partials<Law>, grid, dim3(256), D * sizeof(double), ctx->stream, law, x1, n1, x2,
                       n2, D, Kadj, ldka, part);
  hipLaunchKernelGGL(k_gp_rect_final<Law>, dim3(1), dim3(1024), 0, ctx->stream, law, part, nb, out);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

inline int grid_for(long long tot) {
  long long g = (tot + 255) / 256;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (int)g;
}

// K of family F for checked arguments, n > 0: the column form for aligned
// scalar x, the 2-D grid otherwise, the LDS-staged form for D > 1.
template <int F>
int gp_fwd(smg_ctx* ctx, const double* x, int D, int n, double sigma, double l, double* K, int ldk) {
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  const double s2 = sigma * sigma;
  const double c = gp_fam<F>::coef(l);
  if (D > 1) {
    hipLaunchKernelGGL(k_gp_nd_fwd<F>, dim3(n < 2048 ? n : 2048), dim3(256), D * sizeof(double), ctx->stream, x, D, n,
                       s2, c, K, ldk);
    SMG_LAUNCH_CHECK();
    return SMG_OK;
  }
  if (col2_ok(x, 2, n) && col2_ok(K, ldk, n)) {
    hipLaunchKernelGGL(k_gp_fwd_col2<F>, dim3(n < 2048 ? n : 2048), dim3(256), 0, ctx->stream, x, n, s2, c, K, ldk);
    SMG_LAUNCH_CHECK();
    return SMG_OK;
  }
  dim3 grid(smg_ceil_div(n, 256) > 16 ? 16 : smg_ceil_div(n, 256), n);
  hipLaunchKernelGGL(k_gp_fwd<F>, grid, dim3(256), 0, ctx->stream, x, n, s2, c, K, ldk);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

// out2 += [d/dsigma, d/dl] of family F from the full adjoint (same forms)
template <int F>
int gp_rev(smg_ctx* ctx, const double* x, int D, int n, double sigma, double l, const double* Kadj, int ldka,
           double* out2) {
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  const double s2 = sigma * sigma;
  const double c = gp_fam<F>::coef(l);
  const bool col2 = D == 1 && col2_ok(x, 2, n) && col2_ok(Kadj, ldka, n);
  int nb = (D > 1 || col2) ? n : grid_for((long long)n * n);
  if (nb > GP_BLOCKS) nb = GP_BLOCKS;
  double* part = smg_ws(ctx, SMG_WS_RED, 2 * (size_t)nb);
  if (!part) return SMG_ERR_OOM;
  if (D > 1)
    hipLaunchKernelGGL(k_gp_nd_rev_partials<F>, dim3(nb), dim3(256), D * sizeof(double), ctx->stream, x, D, n, s2, c,
                       Kadj, ldka, part);
  else if (col2)
    hipLaunchKernelGGL(k_gp_rev_partials_col2<F>, dim3(nb), dim3(256), 0, ctx->stream, x, n, s2, c, Kadj, ldka, part);
  else
    hipLaunchKernelGGL(k_gp_rev_partials<F>, dim3(nb), dim3(256), 0, ctx->stream, x, n, s2, c, Kadj, ldka, part);
  hipLaunchKernelGGL(k_gp_rect_final<gp_stat_law<F>>, dim3(1), dim3(1024), 0, ctx->stream, gp_stat_law<F>(sigma, l), part, nb,
                     out2);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

// The factorisation's input generated in one pass (smg_gp_chol_source_fill):
// L = tril(K + d I), zeros above, for K of family F -- what k_gp_fwd*,
// k_add_diag_fwd* and the factorisation's checked copy left in L's buffer in
// three passes.  A workgroup walks whole columns in order (the first panel's
// land first), so a lane's stores of one instruction are contiguous.  The
// strictly lower elements are k_gp_fwd* / k_gp_nd_fwd's expressions, the
// diagonal k_add_diag_fwd*'s s2 + d (diag); a generated NaN / Inf is what the
// copy's !(|a - a^T| <= 1e-8) flagged.
//
// Column form (D == 1, n % 64 == 0, 16-byte aligned x and columns): two rows
// per 16-byte store, four stores in flight per lane; the pairs above the
// diagonal's are zeros without a load of x.
template <int F>
__global__ __launch_bounds__(256) void k_gp_chol_src_col2(const double* __restrict__ x, int n, double s2,
                                                          double inv_half_sq_l, double diag,
                                                          double* __restrict__ L, int ldl, int* status) {
  const int np = n >> 1;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  bool bad = false;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    const double xj = x[j];
    double2* col = reinterpret_cast<double2*>(L + (size_t)j * ldl);
    const int pd = j >> 1;  // the pair holding the diagonal
    for (int p0 = threadIdx.x; p0 < np; p0 += 4 * 256) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = p0 + 256 * k;
        if (p < np) {
          double2 v = make_double2(0.0, 0.0);
          if (p >= pd) {
            const double2 xi = x2[p];
            const int i = 2 * p;
            if (i > j) {
              v.x = gp_fam<F>::k(gp_fam<F>::from_diff(xi.x - xj), s2, inv_half_sq_l);
              bad |= !(fabs(v.x - v.x) <= 1e-8);
            } else if (i == j) {
              v.x = diag;
            }
            if (i + 1 > j) {
              v.y = gp_fam<F>::k(gp_fam<F>::from_diff(xi.y - xj), s2, inv_half_sq_l);
              bad |= !(fabs(v.y - v.y) <= 1e-8);
            } else {  // i + 1 == j
              v.y = diag;
            }
          }
          col[p] = v;
        }
      }
    }
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, (int)SMG_ERR_NOT_SYMMETRIC);
}

// Generic form: any n, ldl and D (x_j staged in LDS as k_gp_nd_fwd does)
template <int F>
__global__ __launch_bounds__(256) void k_gp_chol_src(const double* __restrict__ x, int D, int n, double s2,
                                                     double inv_half_sq_l, double diag, double* __restrict__ L,
                                                     int ldl, int* status) {
  extern __shared__ double xj[];
  bool bad = false;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += blockDim.x) xj[d] = x[(size_t)j * D + d];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      double v = 0.0;
      if (i == j) {
        v = diag;
      } else if (i > j) {
        if (D == 1) {
          v = gp_fam<F>::k(gp_fam<F>::from_diff(x[i] - xj[0]), s2, inv_half_sq_l);
        } else {
          const double* xi = x + (size_t)i * D;
          double d2 = 0.0;
          for (int d = 0; d < D; ++d) {
            const double t = xi[d] - xj[d];
            d2 += t * t;
          }
          v = gp_fam<F>::k(gp_fam<F>::from_sq(d2), s2, inv_half_sq_l);
        }
        bad |= !(fabs(v - v) <= 1e-8);
      }
      L[i + (size_t)j * ldl] = v;
    }
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, (int)SMG_ERR_NOT_SYMMETRIC);
}

template <int F>
int gp_chol_src(smg_ctx* ctx, const smg_gp_source* s, double* L, int ldl) {
  const int n = s->n;
  const double s2 = s->sigma * s->sigma;
  const double c = gp_fam<F>::coef(s->l);
  const double diag = s2 + s->d;
  const int nb = n < 2048 ? n : 2048;
  if (s->D == 1 && n % 64 == 0 && col2_ok(s->x, 2, n) && col2_ok(L, ldl, n))
    hipLaunchKernelGGL(k_gp_chol_src_col2<F>, dim3(nb), dim3(256), 0, ctx->stream, s->x, n, s2, c, diag, L, ldl,
                       ctx->status_d);
  else
    hipLaunchKernelGGL(k_gp_chol_src<F>, dim3(nb), dim3(256), s->D * sizeof(double), ctx->stream, s->x, s->D, n, s2, c,
                       diag, L, ldl, ctx->status_d);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

}  // namespace

bool smg_gp_source_ok(const smg_gp_source* s) {
  return s && s->n >= 0 && s->D >= 1 && s->D <= 8192 && gp_family_ok(s->family) && (s->n == 0 || s->x) &&
         s->sigma > 0 && s->l > 0 && std::isfinite(s->sigma) && std::isfinite(s->l) && std::isfinite(s->d);
}

// checked arguments (smg_gp_source_ok, n > 0, L n x n with ldl >= n)
int smg_gp_chol_source_launch(smg_ctx* ctx, const smg_gp_source* s, double* L, int ldl) {
  return gp_with_family(s->family, [&](auto F) { return gp_chol_src<F()>(ctx, s, L, ldl); });
}

extern "C" {

int smg_gp_chol_source_fill(smg_ctx* ctx, const smg_gp_source* src, double* L, int ldl) {
  if (!ctx || !smg_gp_source_ok(src) || (src->n > 0 && (!L || ldl < src->n))) return SMG_ERR_ARG;
  if (src->n == 0) return SMG_OK;
  return smg_gp_chol_source_launch(ctx, src, L, ldl);
}

int smg_gp_exp_quad_cov_fwd(smg_ctx* ctx, const double* x, int n, double sigma, double l,
                            double* K, int ldk) {
  if (!ctx || n < 0 || (n > 0 && (!x || !K || ldk < n))) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  return gp_fwd<SMG_GP_EXP_QUAD>(ctx, x, 1, n, sigma, l, K, ldk);
}

int smg_gp_exp_quad_cov_rev(smg_ctx* ctx, const double* x, int n, double sigma, double l,
                            const double* Kadj, int ldka, double* out2) {
  if (!ctx || n < 0 || (n > 0 && (!x || !Kadj || !out2 || ldka < n))) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  return gp_rev<SMG_GP_EXP_QUAD>(ctx, x, 1, n, sigma, l, Kadj, ldka, out2);
}

int smg_gp_exp_quad_cov_nd_fwd(smg_ctx* ctx, const double* x, int D, int n, double sigma, double l, double* K,
                               int ldk) {
  return smg_gp_cov_fwd(ctx, SMG_GP_EXP_QUAD, x, D, n, sigma, l, K, ldk);
}

int smg_gp_exp_quad_cov_nd_rev(smg_ctx* ctx, const double* x, int D, int n, double sigma, double l,
                               const double* Kadj, int ldka, double* out2) {
  return smg_gp_cov_rev(ctx, SMG_GP_EXP_QUAD, x, D, n, sigma, l, Kadj, ldka, out2);
}

int smg_gp_cov_fwd(smg_ctx* ctx, int family, const double* x, int D, int n, double sigma, double l, double* K,
                   int ldk) {
  if (!ctx || n < 0 || D < 1 || D > 8192 || (n > 0 && (!x || !K || ldk < n))) return SMG_ERR_ARG;
  if (!gp_family_ok(family)) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  return gp_with_family(family, [&](auto F) { return gp_fwd<F()>(ctx, x, D, n, sigma, l, K, ldk); });
}

int smg_gp_cov_rev(smg_ctx* ctx, int family, const double* x, int D, int n, double sigma, double l,
                   const double* Kadj, int ldka, double* out2) {
  if (!ctx || n < 0 || D < 1 || D > 8192 || (n > 0 && (!x || !Kadj || !out2 || ldka < n))) return SMG_ERR_ARG;
  if (!gp_family_ok(family)) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  return gp_with_family(family, [&](auto F) { return gp_rev<F()>(ctx, x, D, n, sigma, l, Kadj, ldka, out2); });
}

int smg_gp_cross_cov_fwd(smg_ctx* ctx, int family, const double* x1, int n1, const double* x2, int n2, int D,
                         double sigma, double l, double* K, int ldk) {
  if (!ctx || n1 < 0 || n2 < 0 || D < 1 || D > 8192) return SMG_ERR_ARG;
  if (!gp_family_ok(family)) return SMG_ERR_ARG;
  if (n1 == 0 || n2 == 0) return SMG_OK;
  if (!x1 || !x2 || !K || ldk < n1) return SMG_ERR_ARG;
  return gp_with_family(
      family, [&](auto F) { return rect_fwd(ctx, gp_stat_law<F()>(sigma, l), x1, n1, x2, n2, D, K, ldk); });
}

int smg_gp_cross_cov_rev(smg_ctx* ctx, int family, const double* x1, int n1, const double* x2, int n2, int D,
                         double sigma, double l, const double* Kadj, int ldka, double* out2) {
  if (!ctx || n1 < 0 || n2 < 0 || D < 1 || D > 8192) return SMG_ERR_ARG;
  if (!gp_family_ok(family)) return SMG_ERR_ARG;
  if (n1 == 0 || n2 == 0) return SMG_OK;
  if (!x1 || !x2 || !Kadj || !out2 || ldka < n1) return SMG_ERR_ARG;
  return gp_with_family(family, [&](auto F) {
    return rect_rev(ctx, gp_stat_law<F()>(sigma, l), x1, n1, x2, n2, D, Kadj, ldka, out2);
  });
}

int smg_gp_exp_quad_cov_tangent_fwd(smg_ctx* ctx, const double* x, int n, double sigma, double l,
                                    double dsigma, double dl, double* Kd, int ldk) {
  if (!ctx || n < 0 || (n > 0 && (!x || !Kd || ldk < n))) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  dim3 grid(smg_ceil_div(n, 256) > 16 ? 16 : smg_ceil_div(n, 256), n);
  hipLaunchKernelGGL(k_gp_tan_fwd, grid, dim3(256), 0, ctx->stream, x, n, 2 * sigma * dsigma,
                     sigma * sigma * dl / (l * l * l), 0.5 / (l * l), Kd, ldk);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_gp_exp_quad_cov_tangent_rev(smg_ctx* ctx, const double* x, int n, double sigma, double l,
                                    double dsigma, double dl, const double* Kdadj, int ldka,
                                    double* out4) {
  if (!ctx || n < 0 || (n > 0 && (!x || !Kdadj || !out4 || ldka < n))) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  int nb = grid_for((long long)n * n);
  if (nb > GP_BLOCKS) nb = GP_BLOCKS;
  double* part = smg_ws(ctx, SMG_WS_RED, 3 * (size_t)nb);
  if (!part) return SMG_ERR_OOM;
  hipLaunchKernelGGL(k_gp_tan_partials, dim3(nb), dim3(256), 0, ctx->stream, x, n, 0.5 / (l * l),
                     Kdadj, ldka, part);
  hipLaunchKernelGGL(k_gp_tan_final, dim3(1), dim3(1024), 0, ctx->stream, part, nb, sigma, l,
                     dsigma, dl, out4);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_add_diag_fwd(smg_ctx* ctx, const double* A, int lda, int n, double d, const double* dv,
                     double* B, int ldb) {
  if (!ctx || n < 0 || (n > 0 && (!A || !B || lda < n || ldb < n))) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  if (col2_ok(A, lda, n) && col2_ok(B, ldb, n)) {
    hipLaunchKernelGGL(k_add_diag_fwd_col2, dim3(n < 2048 ? n : 2048), dim3(256), 0, ctx->stream,
                       A, lda, n, d, dv, B, ldb);
    SMG_LAUNCH_CHECK();
    return SMG_OK;
  }
  hipLaunchKernelGGL(k_add_diag_fwd, dim3(grid_for((long long)n * n)), dim3(256), 0, ctx->stream, A,
                     lda, n, d, dv, B, ldb);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_add_diag_rev(smg_ctx* ctx, const double* Ba, int ldb, int n, double* Aa, int ldaa,
                     double* dadj, int vec) {
  if (!ctx || n < 0 || (n > 0 && !Ba)) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  if (Aa && col2_ok(Ba, ldb, n) && col2_ok(Aa, ldaa, n))
    hipLaunchKernelGGL(k_add_full_col2, dim3(n < 2048 ? n : 2048), dim3(256), 0, ctx->stream, Ba,
                       ldb, n, Aa, ldaa);
  else if (Aa)
    hipLaunchKernelGGL(k_add_full, dim3(grid_for((long long)n * n)), dim3(256), 0, ctx->stream, Ba,
                       ldb, n, Aa, ldaa);
  if (dadj)
    hipLaunchKernelGGL(k_diag_adj, dim3(1), dim3(1024), 0, ctx->stream, Ba, ldb, n, dadj, vec);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_gp_periodic_cov_fwd(smg_ctx* ctx, const double* x1, int n1, const double* x2, int n2, int D, double sigma,
                            double l, double p, double* K, int ldk) {
  if (!ctx || n1 < 0 || n2 < 0 || D < 1 || D > 8192) return SMG_ERR_ARG;
  if (n1 == 0 || n2 == 0) return SMG_OK;
  if (!x1 || !x2 || !K || ldk < n1) return SMG_ERR_ARG;
  return rect_fwd(ctx, gp_per_law(sigma, l, p), x1, n1, x2, n2, D, K, ldk);
}

int smg_gp_periodic_cov_rev(smg_ctx* ctx, const double* x1, int n1, const double* x2, int n2, int D, double sigma,
                            double l, double p, const double* Kadj, int ldka, double* out3) {
  if (!ctx || n1 < 0 || n2 < 0 || D < 1 || D > 8192) return SMG_ERR_ARG;
  if (n1 == 0 || n2 == 0) return SMG_OK;
  if (!x1 || !x2 || !Kadj || !out3 || ldka < n1) return SMG_ERR_ARG;
  return rect_rev(ctx, gp_per_law(sigma, l, p), x1, n1, x2, n2, D, Kadj, ldka, out3);
}

int smg_gp_dot_prod_cov_fwd(smg_ctx* ctx, const double* x1, int n1, const double* x2, int n2, int D, double sigma,
                            double* K, int ldk) {
  if (!ctx || n1 < 0 || n2 < 0 || D < 1 || D > 8192) return SMG_ERR_ARG;
  if (n1 == 0 || n2 == 0) return SMG_OK;
  if (!x1 || !x2 || !K || ldk < n1) return SMG_ERR_ARG;
  return rect_fwd(ctx, gp_dot_law(sigma), x1, n1, x2, n2, D, K, ldk);
}

// (no points to read: its own two partials kernels, the walk's grid and final pass)
int smg_gp_dot_prod_cov_rev(smg_ctx* ctx, int n1, int n2, double sigma, const double* Kadj, int ldka, double* out1) {
  if (!ctx || n1 < 0 || n2 < 0) return SMG_ERR_ARG;
  if (n1 == 0 || n2 == 0) return SMG_OK;
  if (!Kadj || !out1 || ldka < n1) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  const bool col2 = col2_ok(Kadj, ldka, n1);
  const dim3 grid = cross_grid(n1, n2, col2 ? 8 * 256 : 256);
  const int nb = (int)(grid.x * grid.y);
  double* part = smg_ws(ctx, SMG_WS_RED, (size_t)nb);
  if (!part) return SMG_ERR_OOM;
  if (col2)
    hipLaunchKernelGGL(k_gp_dot_rev_partials_col2, grid, dim3(256), 0, ctx->stream, n1, n2, Kadj, ldka, part);
  else
    hipLaunchKernelGGL(k_gp_dot_rev_partials, grid, dim3(256), 0, ctx->stream, n1, n2, Kadj, ldka, part);
  hipLaunchKernelGGL(k_gp_rect_final<gp_dot_law>, dim3(1), dim3(1024), 0, ctx->stream, gp_dot_law(sigma), part, nb, out1);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

}  // extern "C"
