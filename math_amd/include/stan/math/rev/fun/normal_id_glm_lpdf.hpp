#ifndef STAN_MATH_REV_FUN_NORMAL_ID_GLM_LPDF_HPP
#define STAN_MATH_REV_FUN_NORMAL_ID_GLM_LPDF_HPP

// normal_id_glm_lpdf<propto>(y | x, alpha, beta, sigma), scalar intercept and
// scale (prim/mat/prob/normal_id_glm_lpdf.hpp:40-150), with y and x resident
// on the device: ONE fused pass over x (smg_normal_id_glm) yields
// [sum y_scaled^2, sum mu', x^T mu'], y_scaled = (y - x beta - alpha)/sigma,
// mu' = y_scaled / sigma.  Semantics kept:
//   * check_positive_finite(sigma) first (:58), then the consistent sizes of
//     y and beta (:59-60);
//   * size_zero(y, sigma) -> 0 (:68-70); include_summand<propto, ...> -> 0
//     when every operand is data (:72-74);
//   * partials (:90-128): alpha' = sum mu', beta' = x^T mu',
//     sigma' = (sum y_scaled^2 - N) / sigma;
//   * a non-finite sum of squares runs check_finite on y, beta, alpha, then
//     on the sum itself under the name of x (:130-136);
//   * logp (:139-150): -N log sqrt(2 pi) unless propto; -N log sigma when
//     !propto or sigma is a var; -sum y_scaled^2 / 2.
// Row shards (glm_shard with yd set) all-reduce the M + 2 sums over RCCL like
// bernoulli_logit_glm_lpmf; N is then the global row count.

#include <stan/math/rev/fun/glm_common.hpp>

#include <algorithm>
#include <cmath>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace stan {
namespace math {
namespace internal {

// first non-finite y (host copy: error path only) -> check_finite's message
inline void glm_throw_nonfinite_y(const char* fn, const double* y, long long n, long long row0 = 0) {
  std::vector<double> h(size_t(n > 0 ? n : 0));
  for (long long i0 = 0; i0 < n; i0 += 1 << 20) {
    const long long c = std::min<long long>(1 << 20, n - i0);
    amd::to_host(h.data() + i0, y + i0, size_t(c));
  }
  for (long long i = 0; i < n; ++i)
    if (!std::isfinite(h[size_t(i)])) {
      std::ostringstream m;
      m << fn << ": Vector of dependent variables[" << row0 + i + 1 << "] is " << h[size_t(i)]
        << ", but must be finite!";
      throw std::domain_error(m.str());
    }
}

template <bool propto>
inline glm_result normal_glm_eval(const glm_shard& s, const glm_params& p, double sigma,
                                  vari* sigma_vi) {
  static const char* fn = "normal_id_glm_lpdf";
  glm_check_positive_finite(fn, "Scale vector", sigma);  // first (:58)
  const int M = s.M;
  if (int(p.beta.size()) != M) glm_size_mismatch(fn, "Weight vector", (long long)p.beta.size(), M);
  glm_check_alpha_size(fn, p, s.rows);
  const bool any_var = p.any_var() || sigma_vi;
  if (s.total_rows == 0 || (propto && !any_var)) return glm_result{};
  smg_ctx* c = amd::ctx();
  // [alpha, beta(M), sigma | out: sq, alpha', beta'(M)]
  double* buf = amd::alloc_doubles(size_t(2 * M + 4));
  double* abs = buf;
  double* out = buf + M + 2;
  std::vector<double> h(size_t(2 * M + 4), 0.0);
  h[0] = p.alpha;
  for (int j = 0; j < M; ++j) h[1 + j] = p.beta[j];
  h[M + 1] = sigma;
  amd::to_device(buf, h.data(), h.size());
  glm_vec_alpha va;  // one intercept per row: mu' is row-local, not reduced
  if (s.rows > 0) {
    double* ws = amd::alloc_doubles(size_t(smg_glm_ws_doubles(s.rows, M)));
    va = glm_vec_alpha_prepare(p, s.rows);
    amd::check(p.alpha_vec ? smg_glm_vec_intercept(c, 1, s.yd, s.x, s.rows, M, s.ldx, va.av, abs, ws, out, va.thp)
                           : smg_normal_id_glm(c, s.yd, s.x, s.rows, M, s.ldx, abs, ws, out), fn);
  } else {
    amd::zero(out, size_t(M + 2));
  }
  if (s.distributed) amd::allreduce_sum(out, M + 2, fn);
  amd::to_host(h.data(), buf, h.size());
  const double sq = h[M + 2];
  if (!std::isfinite(sq)) {  // (:130-136)
    glm_throw_nonfinite_y(fn, s.yd, s.rows, s.row0);
    glm_throw_nonfinite_operands(fn, p, va);
    std::ostringstream m;
    m << fn << ": Matrix of independent variables is " << sq << ", but must be finite!";
    throw std::domain_error(m.str());
  }
  const double N = double(s.total_rows);
  double lp = 0.0;
  if (!propto) lp += -0.91893853320467274178 * N;           // NEG_LOG_SQRT_TWO_PI * N
  if (!propto || sigma_vi) lp -= N * std::log(sigma);
  lp -= 0.5 * sq;
  if (!any_var) return glm_result{lp, nullptr};
  double* g = ChainableStack::instance_->memalloc_.alloc_array<double>(size_t(M + 2));
  for (int j = 0; j <= M; ++j) g[j] = h[M + 3 + j];
  g[M + 1] = (sq - N) / sigma;
  if (p.alpha_vec) return glm_result{lp, glm_vec_node(fn, lp, p, va, s.rows, sigma_vi, g, out + 2, M)};
  return glm_result{lp, new glm_dev_vari(lp, p.alpha_vi, p.beta_vi, p.beta_dev, sigma_vi, g, out + 2, M, fn)};
}

}  // namespace internal

/** Device-resident (y, x) row block: shard.yd (double y), shard.x. */
template <bool propto, typename T_alpha, typename T_beta, typename T_scale>
inline auto normal_id_glm_lpdf(const glm_shard& s, const T_alpha& alpha, const T_beta& beta, const T_scale& sigma) {
  internal::glm_params p;
  internal::glm_alpha(p, alpha);
  internal::glm_beta(p, beta);
  return internal::glm_return<internal::glm_is_var<T_alpha>::value || internal::glm_is_var<T_beta>::value ||
                              std::is_same<T_scale, var>::value>(
      internal::normal_glm_eval<propto>(s, p, internal::glm_sigma_val(sigma), internal::glm_sigma_vi(sigma)));
}

template <bool propto = false, typename T_alpha, typename T_beta, typename T_scale>
inline auto normal_id_glm_lpdf(const dev_data<double>& y, const dev_data<double>& x,
                               const T_alpha& alpha, const T_beta& beta, const T_scale& sigma) {
  static const char* fn = "normal_id_glm_lpdf";
  internal::glm_check_positive_finite(fn, "Scale vector", internal::glm_sigma_val(sigma));  // first (:58)
  return normal_id_glm_lpdf<propto>(internal::glm_shard_of(fn, y, x), alpha, beta, sigma);
}

/** Host data (uploaded per call, like the reference reading host memory). */
template <bool propto = false, typename T_alpha, typename T_beta, typename T_scale>
inline auto normal_id_glm_lpdf(const std::vector<double>& y, const std::vector<double>& x_colmajor,
                               int M, const T_alpha& alpha, const T_beta& beta, const T_scale& sigma) {
  const auto d = internal::glm_upload("normal_id_glm_lpdf", y, x_colmajor, M);
  return normal_id_glm_lpdf<propto>(d.y, d.x, alpha, beta, sigma);
}

}  // namespace math
}  // namespace stan
#endif
