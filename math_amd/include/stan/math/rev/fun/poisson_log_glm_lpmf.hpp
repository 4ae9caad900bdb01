#ifndef STAN_MATH_REV_FUN_POISSON_LOG_GLM_LPMF_HPP
#define STAN_MATH_REV_FUN_POISSON_LOG_GLM_LPMF_HPP

// poisson_log_glm_lpmf<propto>(y | x, alpha, beta), scalar intercept or one per
// row (the vector forms of bernoulli_logit_glm_lpmf.hpp: exposure offsets,
// random effects, a latent GP mean on the device)
// (prim/mat/prob/poisson_log_glm_lpmf.hpp:37-123), with y and x resident on
// the device: ONE fused pass over x (smg_poisson_log_glm) yields
// [sum(y theta - exp theta), sum theta', x^T theta', sum lgamma(y + 1)],
// theta = x beta + alpha, theta' = y - exp(theta).  Semantics kept:
//   * consistent sizes of y and beta (:55-56), check_nonnegative(y) (:61);
//   * size_zero(y) -> 0 (:63-65); every operand data with propto -> 0 (:67-69);
//   * a non-finite sum of theta' runs check_finite on beta, alpha, then the
//     linear predictor under the name of x (:87-91);
//   * logp (:92-100): -sum lgamma(y + 1) unless propto, and
//     + sum(y theta - exp theta) only when include_summand<propto,
//     T_partials_return> -- T_partials_return is double, so with propto the
//     reference returns 0 while its partials are kept; so does this layer;
//   * partials (:102-116): alpha' = sum theta', beta' = x^T theta'.
// Row shards all-reduce the M + 3 sums over RCCL like bernoulli_logit_glm_lpmf.

#include <stan/math/rev/fun/glm_common.hpp>

#include <climits>
#include <cmath>
#include <vector>

namespace stan {
namespace math {
namespace internal {

template <bool propto>
inline glm_result poisson_glm_eval(const glm_shard& s, const glm_params& p) {
  static const char* fn = "poisson_log_glm_lpmf";
  const int M = s.M;
  if (int(p.beta.size()) != M) glm_size_mismatch(fn, "Weight vector", (long long)p.beta.size(), M);
  glm_check_alpha_size(fn, p, s.rows);
  smg_ctx* c = amd::ctx();
  // [alpha, beta(M) | out: s, alpha', beta'(M), lgamma sum | flag]
  double* buf = amd::alloc_doubles(size_t(2 * M + 5));
  double* ab = buf;
  double* out = buf + M + 1;
  double* flag = buf + 2 * M + 4;
  std::vector<double> h(size_t(2 * M + 5), 0.0);
  h[0] = p.alpha;
  for (int j = 0; j < M; ++j) h[1 + j] = p.beta[j];
  amd::to_device(buf, h.data(), h.size());
  amd::check(smg_check_bounded_int(c, s.y, s.rows, 0, INT_MAX, flag), fn);  // check_nonnegative (:61)
  const bool run = s.total_rows > 0 && (p.any_var() || !propto);
  glm_vec_alpha va;  // one intercept per row: theta' is row-local, not reduced
  if (run) {
    if (s.rows > 0) {
      double* ws = amd::alloc_doubles(size_t(smg_glm_ws_doubles(s.rows, M)));
      va = glm_vec_alpha_prepare(p, s.rows);
      amd::check(p.alpha_vec ? smg_glm_vec_intercept(c, 2, s.y, s.x, s.rows, M, s.ldx, va.av, ab, ws, out, va.thp)
                             : smg_poisson_log_glm(c, s.y, s.x, s.rows, M, s.ldx, ab, ws, out), fn);
    }
  }
  // [s, alpha', beta'(M), lgamma sum | flag] are contiguous (zeros when not
  // run): the y flag is summed with them, so every rank throws together
  if (s.distributed) amd::allreduce_sum(out, M + 4, fn);
  amd::to_host(h.data(), buf, h.size());
  if (h[2 * M + 4] != 0.0) glm_throw_negative_y(fn, s.y, s.rows, s.row0);
  if (!run) return glm_result{};
  const double sd = h[M + 2];
  if (!std::isfinite(sd)) {  // (:87-91)
    glm_throw_nonfinite_operands(fn, p, va);
    glm_throw_nonfinite_x(fn);
  }
  const double lp = propto ? 0.0 : h[M + 1] - h[2 * M + 3];
  if (!p.any_var()) return glm_result{lp, nullptr};
  double* g = ChainableStack::instance_->memalloc_.alloc_array<double>(size_t(M + 2));
  for (int j = 0; j <= M; ++j) g[j] = h[M + 2 + j];
  if (p.alpha_vec) return glm_result{lp, glm_vec_node(fn, lp, p, va, s.rows, nullptr, g, out + 2, M)};
  return glm_result{lp, new glm_dev_vari(lp, p.alpha_vi, p.beta_vi, p.beta_dev, nullptr, g, out + 2, M, fn)};
}

}  // namespace internal

/** Device-resident (y, x) row block. */
template <bool propto, typename T_alpha, typename T_beta>
inline auto poisson_log_glm_lpmf(const glm_shard& s, const T_alpha& alpha, const T_beta& beta) {
  internal::glm_params p;
  internal::glm_alpha(p, alpha);
  internal::glm_beta(p, beta);
  return internal::glm_return<internal::glm_is_var<T_alpha>::value || internal::glm_is_var<T_beta>::value>(
      internal::poisson_glm_eval<propto>(s, p));
}

template <bool propto = false, typename T_alpha, typename T_beta>
inline auto poisson_log_glm_lpmf(const dev_data<int>& y, const dev_data<double>& x,
                                 const T_alpha& alpha, const T_beta& beta) {
  return poisson_log_glm_lpmf<propto>(internal::glm_shard_of("poisson_log_glm_lpmf", y, x), alpha, beta);
}

/** Host data (uploaded per call, like the reference reading host memory). */
template <bool propto = false, typename T_alpha, typename T_beta>
inline auto poisson_log_glm_lpmf(const std::vector<int>& y, const std::vector<double>& x_colmajor,
                                 int M, const T_alpha& alpha, const T_beta& beta) {
  const auto d = internal::glm_upload("poisson_log_glm_lpmf", y, x_colmajor, M);
  return poisson_log_glm_lpmf<propto>(d.y, d.x, alpha, beta);
}

}  // namespace math
}  // namespace stan
#endif
