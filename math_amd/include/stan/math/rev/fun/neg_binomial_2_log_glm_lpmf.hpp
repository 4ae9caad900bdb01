#ifndef STAN_MATH_REV_FUN_NEG_BINOMIAL_2_LOG_GLM_LPMF_HPP
#define STAN_MATH_REV_FUN_NEG_BINOMIAL_2_LOG_GLM_LPMF_HPP

// neg_binomial_2_log_glm_lpmf<propto>(y | x, alpha, beta, phi), scalar
// intercept and scalar precision (Stan Math 3.0.0,
// prim/mat/prob/neg_binomial_2_log_glm_lpmf.hpp), with y and x resident on
// the device: ONE fused pass over x (smg_neg_binomial_2_log_glm) yields
//   [A, alpha', beta'(M), B, C, D, phi'],  theta = x beta + alpha,
//   A = sum (y + phi) log(exp theta + phi),  B = sum y theta,
//   C = sum lgamma(y + 1),  D = sum lgamma(y + phi),
//   theta' = y - (y + phi) exp theta / (exp theta + phi),
// every term evaluated from exp(-|theta - log phi|).  The reference's own
// exp(theta) / (exp(theta) + phi) is inf / inf beyond theta = 709; here every
// sum stays finite for finite theta of any size -- a deliberate difference.
//
// The reference's sources were not at hand when this was written: the
// wording of the checks and the propto rules below are as recalled from Stan
// Math 3.0.0.
//   * consistent sizes of y ("Vector of dependent variables") and beta
//     ("Weight vector"), check_nonnegative(y) under "Failures variables",
//     then check_positive_finite(phi) under "Precision parameter";
//   * size_zero(y) -> 0; every operand data with propto -> 0;
//   * a non-finite sum of theta' (or of A or B: theta' itself stays finite at
//     theta = +-inf) runs check_finite on beta, alpha, then the linear
//     predictor under the name of x (poisson_log_glm_lpmf's sequence);
//   * logp = -C + N (phi log phi - lgamma phi) - A + B + D, where
//       -C only without propto,
//       N (phi log phi - lgamma phi) and +D when !propto or phi is a var,
//       +B when !propto or alpha or beta is a var,
//       -A whenever anything is computed;
//   * the partials are always complete: alpha' = sum theta', beta' = x^T
//     theta', phi' = sum (1 - (y + phi)(1 - s)/phi) + (log phi - lse)
//     + (digamma(y + phi) - digamma(phi)).
// Row shards with shard.distributed all-reduce the M + 6 sums and the y flag
// in one call, and N is then the global row count; plain shards summed on the
// tape each use their own rows (as normal_id_glm_lpdf does with N log sigma).
// alpha: a scalar, or one intercept per row (the vector forms of
// bernoulli_logit_glm_lpmf.hpp).
// Not provided: vector phi, M > 256, the fvar<var> tangent.

#include <stan/math/rev/fun/glm_common.hpp>

#include <climits>
#include <cmath>
#include <type_traits>
#include <vector>

namespace stan {
namespace math {
namespace internal {

template <bool propto>
inline glm_result neg_binomial_glm_eval(const glm_shard& s, const glm_params& p, double phi, vari* phi_vi) {
  static const char* fn = "neg_binomial_2_log_glm_lpmf";
  const int M = s.M;
  if (int(p.beta.size()) != M) glm_size_mismatch(fn, "Weight vector", (long long)p.beta.size(), M);
  glm_check_alpha_size(fn, p, s.rows);
  smg_ctx* c = amd::ctx();
  // [alpha, beta(M), phi | out: A, alpha', beta'(M), B, C, D, phi' | flag]
  const size_t nbuf = size_t(2 * M + 9);
  double* buf = amd::alloc_doubles(nbuf);
  double* abp = buf;
  double* out = buf + M + 2;
  double* flag = out + M + 6;
  std::vector<double> h(nbuf, 0.0);
  h[0] = p.alpha;
  for (int j = 0; j < M; ++j) h[1 + j] = p.beta[j];
  h[M + 1] = phi;
  amd::to_device(buf, h.data(), h.size());
  amd::check(smg_check_bounded_int(c, s.y, s.rows, 0, INT_MAX, flag), fn);  // check_nonnegative
  const bool any_var = p.any_var() || phi_vi;
  const bool phi_ok = phi > 0 && std::isfinite(phi);  // its error follows y's
  const bool run = phi_ok && s.total_rows > 0 && (any_var || !propto);
  glm_vec_alpha va;  // one intercept per row: theta' is row-local, not reduced
  if (run && s.rows > 0) {
    double* ws = amd::alloc_doubles(size_t(smg_neg_binomial_2_log_glm_ws_doubles(s.rows, M)));
    va = glm_vec_alpha_prepare(p, s.rows);
    amd::check(p.alpha_vec ? smg_glm_vec_intercept(c, 3, s.y, s.x, s.rows, M, s.ldx, va.av, abp, ws, out, va.thp)
                           : smg_neg_binomial_2_log_glm(c, s.y, s.x, s.rows, M, s.ldx, abp, ws, out), fn);
  }
  // the M + 6 sums and the y flag are contiguous (zeros when not run): one
  // all-reduce carries them, so every rank throws together
  if (s.distributed) amd::allreduce_sum(out, M + 7, fn);
  amd::to_host(h.data(), buf, h.size());
  const double* o = h.data() + M + 2;
  if (o[M + 6] != 0.0) glm_throw_negative_y(fn, s.y, s.rows, s.row0, "Failures variables");
  glm_check_positive_finite(fn, "Precision parameter", phi);
  if (!run) return glm_result{};
  // the stable forms keep theta' finite at theta = +-inf, where alpha' alone
  // would pass; B = sum y theta is non-finite whenever a theta is (0 inf = NaN)
  if (!std::isfinite(o[1]) || !std::isfinite(o[M + 2]) || !std::isfinite(o[0])) {
    glm_throw_nonfinite_operands(fn, p, va);
    glm_throw_nonfinite_x(fn);
  }
  const double N = double(s.distributed ? s.total_rows : s.rows);
  double lp = 0.0;
  if (!propto) lp -= o[M + 3];
  if (!propto || phi_vi) lp += N * (phi * std::log(phi) - std::lgamma(phi)) + o[M + 4];
  if (!propto || p.any_var()) lp += o[M + 2];
  lp -= o[0];
  if (!any_var) return glm_result{lp, nullptr};
  double* g = ChainableStack::instance_->memalloc_.alloc_array<double>(size_t(M + 2));
  for (int j = 0; j <= M; ++j) g[j] = o[1 + j];
  g[M + 1] = o[M + 5];
  if (p.alpha_vec) return glm_result{lp, glm_vec_node(fn, lp, p, va, s.rows, phi_vi, g, out + 2, M)};
  return glm_result{lp, new glm_dev_vari(lp, p.alpha_vi, p.beta_vi, p.beta_dev, phi_vi, g, out + 2, M, fn)};
}

}  // namespace internal

/** Device-resident (y, x) row block. */
template <bool propto = false, typename T_alpha, typename T_beta, typename T_precision>
inline auto neg_binomial_2_log_glm_lpmf(const glm_shard& s, const T_alpha& alpha, const T_beta& beta,
                                        const T_precision& phi) {
  internal::glm_params p;
  internal::glm_alpha(p, alpha);
  internal::glm_beta(p, beta);
  return internal::glm_return<internal::glm_is_var<T_alpha>::value || internal::glm_is_var<T_beta>::value ||
                              std::is_same<T_precision, var>::value>(
      internal::neg_binomial_glm_eval<propto>(s, p, internal::glm_sigma_val(phi), internal::glm_sigma_vi(phi)));
}

template <bool propto = false, typename T_alpha, typename T_beta, typename T_precision>
inline auto neg_binomial_2_log_glm_lpmf(const dev_data<int>& y, const dev_data<double>& x,
                                        const T_alpha& alpha, const T_beta& beta, const T_precision& phi) {
  return neg_binomial_2_log_glm_lpmf<propto>(internal::glm_shard_of("neg_binomial_2_log_glm_lpmf", y, x), alpha,
                                             beta, phi);
}

/** Host data (uploaded per call, like the reference reading host memory). */
template <bool propto = false, typename T_alpha, typename T_beta, typename T_precision>
inline auto neg_binomial_2_log_glm_lpmf(const std::vector<int>& y, const std::vector<double>& x_colmajor,
                                        int M, const T_alpha& alpha, const T_beta& beta,
                                        const T_precision& phi) {
  const auto d = internal::glm_upload("neg_binomial_2_log_glm_lpmf", y, x_colmajor, M);
  return neg_binomial_2_log_glm_lpmf<propto>(d.y, d.x, alpha, beta, phi);
}

}  // namespace math
}  // namespace stan
#endif
