// Heavy-tailed location-scale densities as fused one-launch reducers:
// student_t_lpdf (KIND 0) and cauchy_lpdf (KIND 1).  One kernel template in
// normal_lpdf's pattern (k_normal_fused, elementwise.hip): domain checks, value
// and partials in ONE launch over operands in device memory or in pinned host
// memory (zero-copy), ended by a completion word.  A further density of the
// same shape is one more KIND.
#include <cmath>

#include "smg_internal.h"
#include "special_dev.h"  // dev_lgamma, dev_digamma

namespace {

constexpr int HT_COLS = 9;        // [lp, bad_y, bad_nu, bad_mu, bad_sigma, sum y', sum nu', sum mu', sum sigma']
constexpr int HT_BLOCK = 1024;    // threads of a block
constexpr int HT_PER_BLOCK = 4096;  // elements of a block before the grid grows
constexpr int HT_MAX_BLOCKS = 512;

// flag columns (1..4) hold bit sets and combine by OR, the others by sum
__device__ __forceinline__ double ht_combine(int col, double a, double b) {
  return (col >= 1 && col <= 4) ? (double)((int)a | (int)b) : a + b;
}

// With z = (y - mu) / sigma, and for Student-t q = z^2 / nu, h = nu / 2
// (prim/scal/prob/student_t_lpdf.hpp, cauchy_lpdf.hpp; Cauchy is the t at
// nu = 1 without the nu terms: q = z^2, w = 2):
//   lp    = c0 + [lgamma(h + 1/2) - lgamma(h) - 1/2 log nu] - log sigma - (h + 1/2) log1p(q)
//   y'    = -w z / (sigma (1 + q)),  w = (nu + 1) / nu;   mu' = -y'
//   nu'   = 1/2 [digamma(h + 1/2) - digamma(h) - 1/nu] + 1/2 [w q / (1 + q) - log1p(q)]
//   sigma'= -1/sigma + w z^2 / (sigma (1 + q))
// include bits: 1 = c0, 2 = -log sigma, 4 = the log1p term, 8 = the nu-only
// terms.  A null operand pointer selects the scalar kernel argument; a term
// that depends on scalar operands alone (c0; the nu-only brackets with scalar
// nu; log sigma and -1/sigma with scalar sigma) is evaluated once per launch
// by the thread that writes its column and enters as n times the term, so
// the element loop of vector y, mu with scalar nu, sigma is one division, one
// log1p and multiplies.  Only a vector nu pays lgamma / digamma per element:
// VNU (nu is a vector) is a template parameter beside KIND, so the inlined
// special functions of that loop cost the scalar-nu loop no registers.
//
// Per-block columns HT_COLS; bad_nu / bad_sigma: bit 1 = an element failed
// > 0 (a NaN included), bit 2 = an element is +infinity (check_positive_finite
// reports the first kind over the whole operand before the second).  Vector
// partials are WRITTEN where their pointer is non-null; a scalar operand's
// non-null pointer asks for its partial reduced into the result.  Block
// reduction, self-resetting ticket, block-order final sum, one system-scope
// release and the completion word: k_normal_fused's protocol (its comment has
// the measured reasons).  Bitwise repeatable.
template <int KIND, bool VNU>
__global__ void __launch_bounds__(HT_BLOCK) k_heavy_tail_fused(
    const double* __restrict__ y, const double* __restrict__ nu, const double* __restrict__ mu,
    const double* __restrict__ sg, double y0, double nu0, double mu0, double s0, long long n, int inc, double* gy,
    double* gnu, double* gmu, double* gs, double* part, unsigned int* counter, double* res, long long* done,
    long long seq) {
  __shared__ double lds[HT_COLS][16];
  __shared__ int last;
  const bool red_y = !y, red_nu = !VNU, red_mu = !mu, red_s = !sg;
  const double inv_s0 = 1.0 / s0;
  const double inv_nu0 = KIND == 0 ? 1.0 / nu0 : 1.0;
  const double w0 = KIND == 0 ? (nu0 + 1.0) * inv_nu0 : 2.0;
  const double hp0 = KIND == 0 ? 0.5 * nu0 + 0.5 : 1.0;
  double v[HT_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int fnu = 0, fs = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const double yv = y ? y[i] : y0, mv = mu ? mu[i] : mu0, s = sg ? sg[i] : s0;
    if (yv != yv) v[1] = 1.0;                               // check_not_nan(y)
    if (!(fabs(mv) <= 1.7976931348623157e308)) v[3] = 1.0;  // check_finite(mu)
    if (!(s > 0.0)) fs |= 1;                                // check_positive_finite(sigma)
    if (s > 1.7976931348623157e308) fs |= 2;
    const double inv_s = sg ? 1.0 / s : inv_s0;
    const double z = (yv - mv) * inv_s;
    const double z2 = z * z;
    double nv = nu0, inv_nu = inv_nu0, w = w0, hp = hp0;
    if (KIND == 0) {
      if (VNU) {
        nv = nu[i];
        inv_nu = 1.0 / nv;
        w = (nv + 1.0) * inv_nu;
        hp = 0.5 * nv + 0.5;
      }
      if (!(nv > 0.0)) fnu |= 1;  // check_positive_finite(nu)
      if (nv > 1.7976931348623157e308) fnu |= 2;
    }
    const double q = KIND == 0 ? z2 * inv_nu : z2;
    const double r = 1.0 / (1.0 + q);
    const double l = log1p(q);
    if (inc & 4) v[0] -= hp * l;
    if ((inc & 2) && sg) v[0] -= log(s);
    if (KIND == 0 && VNU && (inc & 8)) v[0] += dev_lgamma(hp) - dev_lgamma(0.5 * nv) - 0.5 * log(nv);
    const double t = w * r;
    const double sc = t * z * inv_s;  // mu' = -y'
    if (gy) {
      if (red_y) v[5] -= sc; else gy[i] = -sc;
    }
    if (gmu) {
      if (red_mu) v[7] += sc; else gmu[i] = sc;
    }
    if (gs) {
      const double e = t * z2 * inv_s;
      if (red_s) v[8] += e; else gs[i] = e - inv_s;
    }
    if (KIND == 0 && gnu) {
      const double e = 0.5 * (t * q - l);
      if (red_nu) v[6] += e;
      else gnu[i] = e + 0.5 * (dev_digamma(hp) - dev_digamma(0.5 * nv) - inv_nu);
    }
  }
  const int lane = threadIdx.x & 63, w_ = threadIdx.x >> 6, nw = blockDim.x >> 6;
  // flags by ballot; shuffle reductions only for the sums that are used
  const bool any_y = __any(v[1] != 0.0), any_mu = __any(v[3] != 0.0);
  const int bits_nu = (__any(fnu & 1) ? 1 : 0) | (__any(fnu & 2) ? 2 : 0);
  const int bits_s = (__any(fs & 1) ? 1 : 0) | (__any(fs & 2) ? 2 : 0);
  const double t0 = wave_sum(v[0]);
  const double t5 = (gy && red_y) ? wave_sum(v[5]) : 0.0;
  const double t6 = (KIND == 0 && gnu && red_nu) ? wave_sum(v[6]) : 0.0;
  const double t7 = (gmu && red_mu) ? wave_sum(v[7]) : 0.0;
  const double t8 = (gs && red_s) ? wave_sum(v[8]) : 0.0;
  if (lane == 0) {
    lds[0][w_] = t0;
    lds[1][w_] = any_y ? 1.0 : 0.0;
    lds[2][w_] = (double)bits_nu;
    lds[3][w_] = any_mu ? 1.0 : 0.0;
    lds[4][w_] = (double)bits_s;
    lds[5][w_] = t5;
    lds[6][w_] = t6;
    lds[7][w_] = t7;
    lds[8][w_] = t8;
  }
  __syncthreads();
  const int col = threadIdx.x;
  double tot = 0.0;  // thread c < HT_COLS: column c combined over the block's waves in order
  if (col < HT_COLS)
    for (int k = 0; k < nw; ++k) tot = ht_combine(col, tot, lds[col][k]);
  if (gridDim.x > 1) {
    if (col < HT_COLS)
      __hip_atomic_store(part + HT_COLS * blockIdx.x + col, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every wave's partial-vector and part stores have left it before the
    // barrier; then ONE system-scope release by thread 0 makes them all
    // visible (pinned host memory included) ahead of the ticket, and the
    // ticket's acquire orders the last block's reads of every part
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    if (col < HT_COLS) {
      tot = 0.0;
      for (unsigned int b = 0; b < gridDim.x; ++b)
        tot = ht_combine(col, tot, __hip_atomic_load(part + HT_COLS * b + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the terms of scalar operands alone: once per launch, n times the term
  if (n > 0) {
    const double dn = (double)n;
    if (col == 0) {
      double c = 0.0;
      if (inc & 1) c += KIND == 0 ? -0.57236494292470008707 /* -log sqrt(pi) */ : -1.1447298858494001741 /* -log pi */;
      if ((inc & 2) && red_s) c -= log(s0);
      if (KIND == 0 && (inc & 8) && red_nu) c += dev_lgamma(hp0) - dev_lgamma(0.5 * nu0) - 0.5 * log(nu0);
      tot += dn * c;
    }
    if (KIND == 0 && col == 6 && gnu && red_nu)
      tot += dn * (0.5 * (dev_digamma(hp0) - dev_digamma(0.5 * nu0) - inv_nu0));
    if (col == 8 && gs && red_s) tot -= dn * inv_s0;
  }
  if (col < HT_COLS) res[col] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope: the L2 lines of every output
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

template <int KIND>
int heavy_tail_fused(smg_ctx* ctx, const double* y, const double* nu, const double* mu, const double* sigma, double y0,
                     double nu0, double mu0, double sigma0, long long n, int include, double* res, double* gy,
                     double* gnu, double* gmu, double* gsigma) {
  if (!ctx || n < 0 || !res) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_ELEMWISE);
  const int nb = n <= HT_PER_BLOCK ? 1
                                   : (int)(n / HT_PER_BLOCK < HT_MAX_BLOCKS ? (n + HT_PER_BLOCK - 1) / HT_PER_BLOCK
                                                                            : HT_MAX_BLOCKS);
  double* part = nb > 1 ? smg_ws(ctx, SMG_WS_RED, HT_COLS * (size_t)nb) : nullptr;
  if (nb > 1 && !part) return SMG_ERR_OOM;
  const long long seq = ++ctx->done_seq;
  if (KIND == 0 && nu)
    hipLaunchKernelGGL((k_heavy_tail_fused<KIND, KIND == 0>), dim3(nb), dim3(HT_BLOCK), 0, ctx->stream, y, nu, mu, sigma,
                       y0, nu0, mu0, sigma0, n, include, gy, gnu, gmu, gsigma, part, ctx->red_counter_d, res,
                       ctx->done_h, seq);
  else
    hipLaunchKernelGGL((k_heavy_tail_fused<KIND, false>), dim3(nb), dim3(HT_BLOCK), 0, ctx->stream, y, nu, mu, sigma,
                       y0, nu0, mu0, sigma0, n, include, gy, gnu, gmu, gsigma, part, ctx->red_counter_d, res,
                       ctx->done_h, seq);
  SMG_LAUNCH_CHECK();
  return smg_wait_done(ctx, seq);
}

}  // namespace

extern "C" {

int smg_student_t_lpdf_fused(smg_ctx* ctx, const double* y, const double* nu, const double* mu, const double* sigma,
                             double y0, double nu0, double mu0, double sigma0, long long n, int include, double* res,
                             double* gy, double* gnu, double* gmu, double* gsigma) {
  return heavy_tail_fused<0>(ctx, y, nu, mu, sigma, y0, nu0, mu0, sigma0, n, include, res, gy, gnu, gmu, gsigma);
}

int smg_cauchy_lpdf_fused(smg_ctx* ctx, const double* y, const double* mu, const double* sigma, double y0, double mu0,
                          double sigma0, long long n, int include, double* res, double* gy, double* gmu,
                          double* gsigma) {
  return heavy_tail_fused<1>(ctx, y, nullptr, mu, sigma, y0, 1.0, mu0, sigma0, n, include, res, gy, nullptr, gmu,
                             gsigma);
}

}  // extern "C"
