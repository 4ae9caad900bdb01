#ifndef STAN_MATH_REV_FUN_ORDERED_LOGISTIC_GLM_LPMF_HPP
#define STAN_MATH_REV_FUN_ORDERED_LOGISTIC_GLM_LPMF_HPP

// ordered_logistic_glm_lpmf<propto>(y | x, beta, cuts): y in 1..C, C - 1
// cut-points c_1 < ... < c_{C-1} (c_0 = -inf, c_C = +inf), no intercept, with
// y and x resident on the device: ONE fused pass over x
// (smg_ordered_logistic_glm) yields [logp, beta'(M), cuts'(C - 1)].  With
// eta = x beta, k = y_i, a = c_k - eta, b = c_{k-1} - eta:
//   logp   = sum log(logistic(a) - logistic(b))
//          = sum [k < C] ll(a) + [k > 1] ll(-b) + log1m_exp(-(c_k - c_{k-1})),
//   theta' = [k > 1] logistic(b) - [k < C] logistic(-a),  beta' = x^T theta',
//   cuts'_j = sum_{y = j} (logistic(-a) + r_j) - sum_{y = j+1} (logistic(b) + r_{j+1}),
//   r_k = 1 / expm1(c_k - c_{k-1}),
// every term evaluated from exp(-|a|), exp(-|b|) and the cut-point gaps: logp
// is finite for finite eta of any size and for adjacent cut-points one ulp
// apart.
//
// The reference's sources were not at hand when this was written: the
// wording of the checks and the propto rule below are as recalled from Stan
// Math.
//   * consistent sizes of y ("Vector of dependent variables") and beta
//     ("Weight vector"), check_bounded(y, 1, C), check_ordered(cuts) under
//     "Cut-points", then check_finite of the last and the first cut-point
//     ("Final cut-point", "First cut-point");
//   * size_zero(y) -> 0; every operand data with propto -> 0; otherwise
//     nothing is dropped (no term is constant in the parameters);
//   * a non-finite logp or partial runs check_finite on beta, then throws
//     under the name of x ("Matrix of independent variables");
//   * C = 1 (no cut-points): every probability is 1, logp and the partials
//     are 0.
// Row shards with shard.distributed all-reduce the M + C sums and the y flag
// in one call.
// Not provided: M > 256 or C > 16 (smg_ordered_logistic_glm's SMG_ERR_ARG
// surfaces as an exception), a vector of cut-point vectors, the fvar<var>
// tangent.

#include <stan/math/rev/fun/glm_common.hpp>

#include <cmath>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace stan {
namespace math {
namespace internal {

/** The cut-points: host values and, when they are vars, their varis. */
struct glm_cuts {
  std::vector<double> val;
  vari** vi = nullptr;
};
inline void glm_cuts_of(glm_cuts& c, const std::vector<double>& v) { c.val = v; }
inline void glm_cuts_of(glm_cuts& c, const std::vector<var>& v) {
  c.val.resize(v.size());
  c.vi = ChainableStack::instance_->memalloc_.alloc_array<vari*>(v.size() ? v.size() : 1);
  for (size_t j = 0; j < v.size(); ++j) {
    c.val[j] = v[j].val();
    c.vi[j] = v[j].vi_;
  }
}

/** One node over (beta, cuts): partials g = [beta'(M), cuts'(K)] on the host
 * (arena), beta' also on the device for device-resident beta. */
class glm_ordered_dev_vari : public local_adjoint_vari {
 public:
  vari** beta_vi_;
  dev_matrix_vari* beta_dev_;
  vari** cuts_vi_;
  double* g_;
  const double* g_dev_;
  int M_, K_;
  glm_ordered_dev_vari(double lp, vari** b, dev_matrix_vari* bd, vari** cu, double* g, const double* gd, int M,
                       int K)
      : local_adjoint_vari(lp), beta_vi_(b), beta_dev_(bd), cuts_vi_(cu), g_(g), g_dev_(gd), M_(M), K_(K) {}
  bool touches_adjoints_in(const vari* lo, const vari* hi) const override {
    auto in = [&](const vari* v) { return v && v >= lo && v < hi; };
    if (beta_vi_)
      for (int j = 0; j < M_; ++j)
        if (in(beta_vi_[j])) return true;
    if (cuts_vi_)
      for (int j = 0; j < K_; ++j)
        if (in(cuts_vi_[j])) return true;
    return false;
  }
  void chain() override {
    if (beta_vi_)
      for (int j = 0; j < M_; ++j) beta_vi_[j]->adj_ += adj_ * g_[j];
    if (beta_dev_)
      amd::check(smg_axpy(amd::ctx(), M_, adj_, g_dev_, 1, beta_dev_->adj(), 1), "ordered_logistic_glm_lpmf");
    if (cuts_vi_)
      for (int j = 0; j < K_; ++j) cuts_vi_[j]->adj_ += adj_ * g_[M_ + j];
  }
};

// check_ordered(fn, "Cut-points", c), then check_finite of the last and the
// first cut-point
inline void ordered_glm_check_cuts(const char* fn, const std::vector<double>& c) {
  for (size_t n = 1; n < c.size(); ++n)
    if (!(c[n] > c[n - 1])) {
      std::ostringstream m;
      m << fn << ": Cut-points is not a valid ordered vector. The element at " << n + 1 << " is " << c[n]
        << ", but should be greater than the previous element, " << c[n - 1];
      throw std::domain_error(m.str());
    }
  if (c.empty()) return;
  if (!std::isfinite(c.back())) {
    std::ostringstream m;
    m << fn << ": Final cut-point is " << c.back() << ", but must be finite!";
    throw std::domain_error(m.str());
  }
  if (!std::isfinite(c.front())) {
    std::ostringstream m;
    m << fn << ": First cut-point is " << c.front() << ", but must be finite!";
    throw std::domain_error(m.str());
  }
}

inline bool ordered_glm_cuts_ok(const std::vector<double>& c) {
  for (size_t n = 1; n < c.size(); ++n)
    if (!(c[n] > c[n - 1])) return false;
  return c.empty() || (std::isfinite(c.front()) && std::isfinite(c.back()));
}

template <bool propto>
inline glm_result ordered_glm_eval(const glm_shard& s, const glm_params& p, const glm_cuts& cu) {
  static const char* fn = "ordered_logistic_glm_lpmf";
  const int M = s.M;
  if (int(p.beta.size()) != M) glm_size_mismatch(fn, "Weight vector", (long long)p.beta.size(), M);
  const int K = int(cu.val.size()), C = K + 1;
  smg_ctx* c = amd::ctx();
  // [beta(M), cuts(K) | out: logp, beta'(M), cuts'(K) | flag]
  const size_t nbuf = size_t(2 * (M + K) + 2);
  double* buf = amd::alloc_doubles(nbuf);
  double* bc = buf;
  double* out = buf + M + K;
  double* flag = out + M + C;
  std::vector<double> h(nbuf, 0.0);
  for (int j = 0; j < M; ++j) h[j] = p.beta[j];
  for (int j = 0; j < K; ++j) h[M + j] = cu.val[j];
  amd::to_device(buf, h.data(), h.size());
  amd::check(smg_check_bounded_int(c, s.y, s.rows, 1, C, flag), fn);
  const bool any_var = p.any_var() || cu.vi;
  const bool cuts_ok = ordered_glm_cuts_ok(cu.val);  // their errors follow y's
  // (C = 1: every probability is 1; the zeros uploaded into `out` stand)
  const bool run = cuts_ok && s.total_rows > 0 && (any_var || !propto);
  if (run && s.rows > 0 && C > 1) {
    double* ws = amd::alloc_doubles(size_t(smg_ordered_logistic_glm_ws_doubles(s.rows, M, C)));
    amd::check(smg_ordered_logistic_glm(c, s.y, s.x, s.rows, M, s.ldx, C, bc, ws, out), fn);
  }
  // the M + C sums and the y flag are contiguous (zeros when not run): one
  // all-reduce carries them, so every rank throws together
  if (s.distributed) amd::allreduce_sum(out, M + C + 1, fn);
  amd::to_host(h.data(), buf, h.size());
  const double* o = h.data() + M + K;
  if (o[M + C] != 0.0) glm_throw_y_bounds(fn, s.y, s.rows, 1, C, s.row0);
  ordered_glm_check_cuts(fn, cu.val);
  if (!run) return glm_result{};
  // (theta' stays finite at eta = +-inf, and logp can: every sum is looked at)
  bool finite = true;
  for (int j = 0; j < M + C; ++j) finite = finite && std::isfinite(o[j]);
  if (!finite) {
    glm_throw_nonfinite_operands(fn, p, glm_vec_alpha());  // (no intercept: beta alone)
    glm_throw_nonfinite_x(fn);
  }
  const double lp = o[0];
  if (!any_var) return glm_result{lp, nullptr};
  double* g = ChainableStack::instance_->memalloc_.alloc_array<double>(size_t(M + K > 0 ? M + K : 1));
  for (int j = 0; j < M + K; ++j) g[j] = o[1 + j];
  return glm_result{lp, new glm_ordered_dev_vari(lp, p.beta_vi, p.beta_dev, cu.vi, g, out + 1, M, K)};
}

}  // namespace internal

/** Device-resident (y, x) row block. */
template <bool propto = false, typename T_beta, typename T_cuts>
inline auto ordered_logistic_glm_lpmf(const glm_shard& s, const T_beta& beta, const T_cuts& cuts) {
  internal::glm_params p;
  internal::glm_beta(p, beta);
  internal::glm_cuts cu;
  internal::glm_cuts_of(cu, cuts);
  return internal::glm_return<internal::glm_is_var<T_beta>::value || internal::glm_is_var<T_cuts>::value>(
      internal::ordered_glm_eval<propto>(s, p, cu));
}

template <bool propto = false, typename T_beta, typename T_cuts>
inline auto ordered_logistic_glm_lpmf(const dev_data<int>& y, const dev_data<double>& x, const T_beta& beta,
                                      const T_cuts& cuts) {
  return ordered_logistic_glm_lpmf<propto>(internal::glm_shard_of("ordered_logistic_glm_lpmf", y, x), beta, cuts);
}

/** Host data (uploaded per call, like the reference reading host memory). */
template <bool propto = false, typename T_beta, typename T_cuts>
inline auto ordered_logistic_glm_lpmf(const std::vector<int>& y, const std::vector<double>& x_colmajor, int M,
                                      const T_beta& beta, const T_cuts& cuts) {
  const auto d = internal::glm_upload("ordered_logistic_glm_lpmf", y, x_colmajor, M);
  return ordered_logistic_glm_lpmf<propto>(d.y, d.x, beta, cuts);
}

}  // namespace math
}  // namespace stan
#endif
