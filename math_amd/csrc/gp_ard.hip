// One length scale per input dimension (ARD) for the GP covariances: the
// std::vector<T_l> length_scale overloads of gp_exp_quad_cov,
// gp_exponential_cov, gp_matern32_cov and gp_matern52_cov.  The reference
// computes them as divide_columns(x, l) followed by the kernel of unit length
// scale; here the same split:
//   z = x / l               smg_gp_ard_scale (this file): point-major z for the
//                           two lines below, coordinate-major zt for the reducers
//   K                       smg_gp_cov_fwd(family, z, D, n, sigma, 1.0)          (gp.hip, unchanged)
//   tril(K + d I) -> L      smg_gp_source {x = z, l = 1}                        (gp.hip, unchanged)
//   sigma', l_1' .. l_D'    smg_gp_ard_cov_rev (dense adjoint) and
//                           smg_gp_ard_cov_inverse_adjoint (G from K^{-1})      (this file)
//   the same sums of the    smg_gp_ard_cross_cov_rev (dense adjoint, z1 and z2
//   cross-covariance        scaled by the same l)                               (this file)
// With t_d = z_id - z_jd, r^2 = sum_d t_d^2 in coordinate order and h from
// gp_family.h:  dK_ij/dl_d = sigma^2 h t_d^2 / l_d (i != j), nothing on the
// diagonal.  K_ij is recomputed with the forward's expression
// (gp_fam<F>::k(from_diff(t_0) | from_sq(r^2), s2, coef(1))).
//
// Accumulators: a thread keeps [diag, sigma, l_0 .. l_{DP-1}] in registers,
// DP = 4, 8 or 16 the padded D (coordinates past D contribute t = 0).  For
// D > 16 the sweep is repeated once per 16 coordinates (r^2 still over all D),
// each pass writing its own columns of the partials.  A workgroup's partial is
// a wave reduction per accumulator, then an ordered sum of the four waves
// through LDS ([waves][DP + 2], read along rows: no bank conflict); one
// ordered pass (k_gp_ard_final) sums the workgroups and applies adj, 2 / sigma
// and 1 / l_d.  No floating-point atomics: the same bits run to run.
//
// The reducers read zt, the coordinate-major copy (n x D, coordinate d of
// point i at zt[d n + i]) that the scale kernel writes beside z: a wave's load
// of one coordinate is 512 contiguous bytes at any D.  Against the point-major
// z (lane stride 8 D bytes) it measured 4 % faster at D = 4 and 2.4 to 3.8
// times faster at D = 16 and 64 (N = 4096, DESIGN "ARD length scales").
#include "smg_internal.h"
#include "gp_family.h"

namespace {

constexpr int ARD_PASS = 16;  // coordinates per pass (the widest register form)

struct ard_scales {
  double v[SMG_GP_ARD_MAX_D];
};

__global__ __launch_bounds__(256) void k_gp_ard_scale(const double* __restrict__ x, int D, long long tot,
                                                      int n, ard_scales l, double* __restrict__ z,
                                                      double* __restrict__ zt) {
  __shared__ double ls[SMG_GP_ARD_MAX_D];
  if ((int)threadIdx.x < D) ls[threadIdx.x] = l.v[threadIdx.x];
  __syncthreads();
  const long long st = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += st) {
    const int i = (int)(e / D), d = (int)(e - (long long)i * D);
    const double v = x[e] / ls[d];
    z[e] = v;
    if (zt) zt[(size_t)d * n + i] = v;
  }
}

// The terms of position (i, j), i != j, with adjoint g: sa += g K_ij and
// al[d] += g s2 h t_d^2 for the coordinates d0 .. d0 + DP - 1.  zi = zt + i:
// coordinate d of point i at zi[d n].
template <int F, int DP>
__device__ __forceinline__ void ard_terms(const double* __restrict__ zi, int n, const double* zj, int D, int d0,
                                          double g, double s2, double c, double& sa, double (&al)[DP]) {
  double t[DP];
  double d2 = 0.0;
  if (D <= DP) {  // one pass: r^2 from the same differences
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      t[d] = d < D ? zi[(size_t)d * n] - zj[d] : 0.0;
      d2 += t[d] * t[d];
    }
  } else {
    for (int d = 0; d < D; ++d) {
      const double u = zi[(size_t)d * n] - zj[d];
      d2 += u * u;
    }
#pragma unroll
    for (int d = 0; d < DP; ++d) t[d] = d0 + d < D ? zi[(size_t)(d0 + d) * n] - zj[d0 + d] : 0.0;
  }
  // (the forward's element: k_gp_fwd from the difference for D == 1, k_gp_nd_fwd from r^2)
  const double q = D == 1 ? gp_fam<F>::from_diff(t[0]) : gp_fam<F>::from_sq(d2);
  sa += g * gp_fam<F>::k(q, s2, c);
  const double gh = g * (s2 * gp_fam<F>::h(q, c));
#pragma unroll
  for (int d = 0; d < DP; ++d) al[d] += gh * (t[d] * t[d]);
}

// a workgroup's partial: part[W * blockIdx.x + {0, 1, 2 + d0 + d}] = the sums
// of sd, sa, al[d] over its threads in a fixed order (sd, sa by the first pass only)
template <int DP>
__device__ __forceinline__ void ard_block_partials(double sd, double sa, const double (&al)[DP], int D, int d0,
                                                   double* __restrict__ part) {
  __shared__ double red[4][DP + 2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  sd = wave_sum(sd);
  sa = wave_sum(sa);
  double r[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) r[d] = wave_sum(al[d]);
  __syncthreads();
  if (lane == 0) {
    red[w][0] = sd;
    red[w][1] = sa;
#pragma unroll
    for (int d = 0; d < DP; ++d) red[w][2 + d] = r[d];
  }
  __syncthreads();
  const int q = threadIdx.x;
  if (q < DP + 2) {
    const double v = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    double* p = part + (size_t)(D + 2) * blockIdx.x;
    if (q < 2) {
      if (d0 == 0) p[q] = v;
    } else if (d0 + q - 2 < D) {
      p[2 + d0 + q - 2] = v;
    }
  }
}

// Dense adjoint: a workgroup walks whole columns j (z_j staged in LDS once per
// column), its threads every row; the element is k_gp_nd_rev_partials'.
template <int F, int DP>
__global__ __launch_bounds__(256) void k_gp_ard_rev_partials(const double* __restrict__ zt, int D, int n, double s2,
                                                             double c, int d0, const double* __restrict__ Ka,
                                                             int lda, double* __restrict__ part) {
  __shared__ double zj[SMG_GP_ARD_MAX_D];
  double sa = 0.0, al[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) al[d] = 0.0;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    __syncthreads();
    if ((int)threadIdx.x < D) zj[threadIdx.x] = zt[(size_t)threadIdx.x * n + j];
    __syncthreads();
    const double* col = Ka + (size_t)j * lda;
    for (int i = threadIdx.x; i < n; i += 256) {
      const double a = col[i];
      if (i == j)
        sa += a * s2;
      else
        ard_terms<F, DP>(zt + i, n, zj, D, d0, a, s2, c, sa, al);
    }
  }
  ard_block_partials<DP>(0.0, sa, al, D, d0, part);
}

// G = Phi(sum_o s_o s_o^T - k C) (adj factored out) over C's lower triangle:
// k_gp_inv_reduce's balanced column pairing (j, n - 1 - j), n + 1 rows per
// workgroup; z_j staged once per column.
template <int F, int DP>
__global__ __launch_bounds__(256) void k_gp_ard_inv_reduce(const double* __restrict__ C, int ldc, int n,
                                                           const double* __restrict__ s, int k, long long ss,
                                                           const double* __restrict__ zt, int D, double s2, double c,
                                                           int d0, double* __restrict__ part) {
  __shared__ double zj[SMG_GP_ARD_MAX_D];
  double sd = 0.0, sa = 0.0, al[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) al[d] = 0.0;
  const int half = (n + 1) / 2;
  for (int b = blockIdx.x; b < half; b += gridDim.x) {
    for (int h = 0; h < 2; ++h) {
      const int j = h == 0 ? b : n - 1 - b;
      if (h == 1 && j == b) break;  // (odd n: the unpaired middle column)
      __syncthreads();
      if ((int)threadIdx.x < D) zj[threadIdx.x] = zt[(size_t)threadIdx.x * n + j];
      __syncthreads();
      const double* col = C + (size_t)j * ldc;
      for (int i = j + threadIdx.x; i < n; i += 256) {
        double g = 0.0;
        for (int o = 0; o < k; ++o) g += s[o * ss + i] * s[o * ss + j];
        g -= k * col[i];
        if (i == j) {
          sd += 0.5 * g;
          sa += 0.5 * g * s2;
        } else {
          ard_terms<F, DP>(zt + i, n, zj, D, d0, g, s2, c, sa, al);
        }
      }
    }
  }
  ard_block_partials<DP>(sd, sa, al, D, d0, part);
}

// sum_i Phi(.)_ii alone (dadj without the hyperparameter sums)
__global__ __launch_bounds__(1024) void k_gp_ard_diag(const double* __restrict__ C, int ldc, int n,
                                                      const double* __restrict__ s, int k, long long ss, double adj,
                                                      double* dadj) {
  __shared__ double lds[16];
  double sd = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    double g = 0.0;
    for (int o = 0; o < k; ++o) g += s[o * ss + i] * s[o * ss + i];
    g -= k * C[i + (size_t)i * ldc];
    sd += 0.5 * g;
  }
  sd = block_sum(sd, lds);
  if (threadIdx.x == 0) dadj[0] = adj * sd;
}

// The ordered sum of the workgroups' partials, one wave per quantity q of
// [sd, sa, l_0 ..]: dadj = adj sd, out[0] = 2 adj sa / sigma, out[1 + d] =
// adj sl_d / l_d; acc: added to out (the dense entry) instead of written.
__global__ __launch_bounds__(1024) void k_gp_ard_final(const double* __restrict__ part, int nparts, int D, double adj,
                                                       double sigma, ard_scales l, int acc, double* dadj,
                                                       double* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int W = D + 2;
  for (int q = w; q < W; q += 16) {
    double v = 0.0;
    for (int i = lane; i < nparts; i += 64) v += part[(size_t)W * i + q];
    v = wave_sum(v);
    if (lane != 0) continue;
    if (q == 0) {
      if (dadj) dadj[0] = adj * v;
    } else if (out) {
      const double r = q == 1 ? adj * v * 2 / sigma : adj * v / l.v[q - 2];
      out[q - 1] = acc ? out[q - 1] + r : r;
    }
  }
}

inline ard_scales host_scales(const double* l, int D) {
  ard_scales r;
  for (int d = 0; d < SMG_GP_ARD_MAX_D; ++d) r.v[d] = d < D ? l[d] : 1.0;
  return r;
}

template <int F, int DP>
void launch_rev(smg_ctx* ctx, int nb, const double* zt, int D, int n, double s2, const double* Ka, int lda,
                double* part) {
  const double c = gp_fam<F>::coef(1.0);
  for (int d0 = 0; d0 < D; d0 += DP)
    hipLaunchKernelGGL((k_gp_ard_rev_partials<F, DP>), dim3(nb), dim3(256), 0, ctx->stream, zt, D, n, s2, c, d0, Ka,
                       lda, part);
}

template <int F, int DP>
void launch_inv(smg_ctx* ctx, int nb, const double* C, int ldc, int n, const double* s, int k, long long ss,
                const double* zt, int D, double s2, double* part) {
  const double c = gp_fam<F>::coef(1.0);
  for (int d0 = 0; d0 < D; d0 += DP)
    hipLaunchKernelGGL((k_gp_ard_inv_reduce<F, DP>), dim3(nb), dim3(256), 0, ctx->stream, C, ldc, n, s, k, ss, zt, D,
                       s2, c, d0, part);
}

// k_gp_ard_rev_partials for the cross-covariance K(x1, x2), n1 x n2: the
// column point from z2t, the row points from z1t, no diagonal (a coincident
// pair goes through ard_terms: K = s2, t_d = 0, and exponential's h is 0 there).
// blockIdx.y takes every gridDim.y-th pass of the rows (a tall K with few
// columns); its partials follow those of the row parts before it.
template <int F, int DP>
__global__ __launch_bounds__(256) void k_gp_ard_cross_rev_partials(const double* __restrict__ z1t, int n1,
                                                                   const double* __restrict__ z2t, int n2, int D,
                                                                   double s2, double c, int d0,
                                                                   const double* __restrict__ Ka, int lda,
                                                                   double* __restrict__ part) {
  __shared__ double zj[SMG_GP_ARD_MAX_D];
  double sa = 0.0, al[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) al[d] = 0.0;
  for (int j = blockIdx.x; j < n2; j += gridDim.x) {
    __syncthreads();
    if ((int)threadIdx.x < D) zj[threadIdx.x] = z2t[(size_t)threadIdx.x * n2 + j];
    __syncthreads();
    const double* col = Ka + (size_t)j * lda;
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n1; i += gridDim.y * 256)
      ard_terms<F, DP>(z1t + i, n1, zj, D, d0, col[i], s2, c, sa, al);
  }
  ard_block_partials<DP>(0.0, sa, al, D, d0, part + (size_t)(D + 2) * gridDim.x * blockIdx.y);
}

template <int F, int DP>
void launch_cross_rev(smg_ctx* ctx, dim3 grid, const double* z1t, int n1, const double* z2t, int n2, int D, double s2,
                      const double* Ka, int lda, double* part) {
  const double c = gp_fam<F>::coef(1.0);
  for (int d0 = 0; d0 < D; d0 += DP)
    hipLaunchKernelGGL((k_gp_ard_cross_rev_partials<F, DP>), grid, dim3(256), 0, ctx->stream, z1t, n1, z2t, n2, D,
                       s2, c, d0, Ka, lda, part);
}

// the padded D's register form: 4, 8 or 16 accumulators (16 per pass beyond)
#define ARD_DISPATCH_DP(FN, F, ...)                \
  do {                                             \
    if (D <= 4) FN<F, 4>(__VA_ARGS__);             \
    else if (D <= 8) FN<F, 8>(__VA_ARGS__);        \
    else FN<F, ARD_PASS>(__VA_ARGS__);             \
  } while (0)
#define ARD_DISPATCH(FN, ...) gp_with_family(family, [&](auto F) { ARD_DISPATCH_DP(FN, F(), __VA_ARGS__); })

}  // namespace

extern "C" {

int smg_gp_ard_scale(smg_ctx* ctx, const double* x, int D, int n, const double* l, double* z, double* zt) {
  if (!ctx || n < 0 || D < 1 || D > SMG_GP_ARD_MAX_D || (n > 0 && (!x || !l || !z))) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  const long long tot = (long long)n * D;
  long long g = (tot + 255) / 256;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(k_gp_ard_scale, dim3((unsigned)g), dim3(256), 0, ctx->stream, x, D, tot, n,
                     host_scales(l, D), z, zt);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_gp_ard_cov_rev(smg_ctx* ctx, int family, const double* zt, int D, int n, double sigma, const double* l,
                       const double* Kadj, int ldka, double* out) {
  if (!ctx || n < 0 || D < 1 || D > SMG_GP_ARD_MAX_D || !gp_family_ok(family)) return SMG_ERR_ARG;
  if (n > 0 && (!zt || !l || !Kadj || !out || ldka < n)) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  const int nb = n < 2048 ? n : 2048;
  double* part = smg_ws(ctx, SMG_WS_RED, (size_t)(D + 2) * nb);
  if (!part) return SMG_ERR_OOM;
  ARD_DISPATCH(launch_rev, ctx, nb, zt, D, n, sigma * sigma, Kadj, ldka, part);
  hipLaunchKernelGGL(k_gp_ard_final, dim3(1), dim3(1024), 0, ctx->stream, part, nb, D, 1.0, sigma, host_scales(l, D),
                     1, (double*)nullptr, out);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_gp_ard_cross_cov_rev(smg_ctx* ctx, int family, const double* z1t, int n1, const double* z2t, int n2, int D,
                             double sigma, const double* l, const double* Kadj, int ldka, double* out) {
  if (!ctx || n1 < 0 || n2 < 0 || D < 1 || D > SMG_GP_ARD_MAX_D || !gp_family_ok(family)) return SMG_ERR_ARG;
  if (n1 == 0 || n2 == 0) return SMG_OK;
  if (!z1t || !z2t || !l || !Kadj || !out || ldka < n1) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  const dim3 grid = cross_grid(n1, n2, 256);
  const int nb = (int)(grid.x * grid.y);
  double* part = smg_ws(ctx, SMG_WS_RED, (size_t)(D + 2) * nb);
  if (!part) return SMG_ERR_OOM;
  ARD_DISPATCH(launch_cross_rev, ctx, grid, z1t, n1, z2t, n2, D, sigma * sigma, Kadj, ldka, part);
  hipLaunchKernelGGL(k_gp_ard_final, dim3(1), dim3(1024), 0, ctx->stream, part, nb, D, 1.0, sigma, host_scales(l, D),
                     1, (double*)nullptr, out);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_gp_ard_cov_inverse_adjoint(smg_ctx* ctx, int family, const double* C, int ldc, int n, const double* s, int k,
                                   long long s_stride, double adj, const double* zt, int D, double sigma,
                                   const double* l, double* dadj, double* out) {
  if (!ctx || n < 0 || k < 1 || (k > 1 && s_stride < n) || D < 1 || D > SMG_GP_ARD_MAX_D || !gp_family_ok(family))
    return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  if (!C || !s || ldc < n || (out && (!zt || !l || !(sigma > 0)))) return SMG_ERR_ARG;
  if (!dadj && !out) return SMG_OK;
  smg_prof_scope prof(ctx, SMG_FAM_GP);
  if (!out) {
    hipLaunchKernelGGL(k_gp_ard_diag, dim3(1), dim3(1024), 0, ctx->stream, C, ldc, n, s, k, s_stride, adj, dadj);
    SMG_LAUNCH_CHECK();
    return SMG_OK;
  }
  const int half = (n + 1) / 2;
  const int nb = half < 2048 ? half : 2048;
  double* part = smg_ws(ctx, SMG_WS_RED, (size_t)(D + 2) * nb);
  if (!part) return SMG_ERR_OOM;
  ARD_DISPATCH(launch_inv, ctx, nb, C, ldc, n, s, k, s_stride, zt, D, sigma * sigma, part);
  hipLaunchKernelGGL(k_gp_ard_final, dim3(1), dim3(1024), 0, ctx->stream, part, nb, D, adj, sigma, host_scales(l, D),
                     0, dadj, out);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

}  // extern "C"
