#ifndef STAN_MATH_REV_FUN_BERNOULLI_LOGIT_GLM_LPMF_HPP
#define STAN_MATH_REV_FUN_BERNOULLI_LOGIT_GLM_LPMF_HPP

// bernoulli_logit_glm_lpmf<propto>(y | x, alpha, beta), scalar intercept or one
// intercept per row (a host vector of double or var, dev_data<double>, or a
// dev_var_matrix R x 1 / 1 x R: smg_glm_vec_intercept, alpha' = theta' per row)
// (prim/mat/prob/bernoulli_logit_glm_lpmf.hpp:46-144), with x and y resident
// on the device: ONE fused pass over x yields [logp, sum theta', x^T theta',
// y-bounds count] (smg_bernoulli_logit_glm_io: parameters in the kernel
// arguments, results written to pinned host memory by the pass's last
// workgroup).
// Semantics kept: check_consistent_size of y / beta (:63-64), check_bounded(y,
// 0, 1) (:69), size_zero -> 0 (:71-73), include_summand<propto, x, alpha,
// beta> (:75-77), the non-finite logp checks of beta, alpha, then the linear
// predictor (:106-110), partials beta' = x^T theta', alpha' = sum theta'
// (:113-135) in one precomputed-gradients node.
//
// Row sharding (the reduce_sum / map_rect path): each rank
// holds a contiguous row block of (y, x) on its own GPU (glm_shard); every
// rank computes its local [logp, alpha', beta'] and ONE RCCL all-reduce sums
// the M + 2 doubles and the y-bounds flag across ranks (amd::allreduce_sum);
// every rank then builds the same node (or throws the same error).  Replaces map_rect's MPI/TBB gather
// (prim/mat/functor/map_rect.hpp:120-177, map_rect_combine.hpp:36-92).

#include <stan/math/rev/fun/glm_common.hpp>

#include <cmath>
#include <new>
#include <vector>

namespace stan {
namespace math {
namespace internal {

template <bool propto>
inline glm_result glm_eval(const glm_shard& s, const glm_params& p) {
  static const char* fn = "bernoulli_logit_glm_lpmf";
  const int M = s.M;
  if (int(p.beta.size()) != M) glm_size_mismatch(fn, "Weight vector", (long long)p.beta.size(), M);
  glm_check_alpha_size(fn, p, s.rows);
  smg_ctx* c = amd::ctx();
  // (alpha, beta) travel in the launch's kernel arguments; the fused pass also
  // counts y outside {0, 1}, and its last workgroup writes [logp, alpha',
  // beta'(M), bad-y count] to `out` (device) and -- on one GPU with no
  // latched-status launch outstanding -- straight to pinned host memory,
  // publishing a completion word the host spins on (no copy, no stream sync)
  double* out = amd::alloc_doubles(size_t(M + 3));
  double* ws = amd::alloc_doubles(size_t(smg_glm_ws_doubles(s.rows > 0 ? s.rows : 1, M)));
  int armed = 0;
  amd::check(smg_status_armed(c, &armed), fn);
  const double* h;
  glm_vec_alpha va;
  if (p.alpha_vec) {
    // one intercept per row: the staged path -- [-, beta(M)] uploaded, the
    // vector entry, the M + 3 sums copied back (theta' is row-local: not reduced)
    va = glm_vec_alpha_prepare(p, s.rows);
    double* ab = amd::alloc_doubles(size_t(M + 1));
    std::vector<double> hab(size_t(M + 1), 0.0);
    for (int j = 0; j < M; ++j) hab[size_t(1 + j)] = p.beta[j];
    amd::to_device(ab, hab.data(), hab.size());
    amd::check(smg_glm_vec_intercept(c, 0, s.y, s.x, s.rows, M, s.ldx, va.av, ab, ws, out, va.thp), fn);
    if (s.distributed) amd::allreduce_sum(out, M + 3, fn);
    double* o = ChainableStack::instance_->memalloc_.alloc_array<double>(size_t(M + 3));
    amd::to_host(o, out, size_t(M + 3));  // (with the armed status' check)
    h = o;
  } else if (!s.distributed && !armed) {
    double* o = static_cast<double*>(smg_pinned_result(c, size_t(M + 3) * sizeof(double)));
    if (!o) throw std::bad_alloc();
    amd::check(smg_bernoulli_logit_glm_io(c, s.y, s.x, s.rows, M, s.ldx, p.alpha, p.beta.data(), ws, out, o), fn);
    h = o;
  } else if (!armed) {
    // sharded: the local results, ONE all-reduce of the M + 3 doubles (the
    // y-support count is summed with the rest, so a bad y on any rank makes
    // every rank throw), then the same zero-copy read of the sums
    amd::check(smg_bernoulli_logit_glm_io(c, s.y, s.x, s.rows, M, s.ldx, p.alpha, p.beta.data(), ws, out,
                                          nullptr), fn);
    amd::allreduce_sum(out, M + 3, fn);
    double* o = static_cast<double*>(smg_pinned_result(c, size_t(M + 3) * sizeof(double)));
    if (!o) throw std::bad_alloc();
    amd::check(smg_publish_to_host(c, out, M + 3, o), fn);
    h = o;
  } else {
    amd::check(smg_bernoulli_logit_glm_io(c, s.y, s.x, s.rows, M, s.ldx, p.alpha, p.beta.data(), ws, out,
                                          nullptr), fn);
    if (s.distributed) amd::allreduce_sum(out, M + 3, fn);
    double* o = static_cast<double*>(smg_host_scratch(c, size_t(M + 4) * sizeof(double)));
    if (!o) throw std::bad_alloc();
    amd::check(smg_memcpy_d2h(c, o, out, size_t(M + 3) * sizeof(double)), fn);
    if (armed) amd::check(smg_status_enqueue(c, reinterpret_cast<int*>(o + M + 3)), fn);
    amd::check(smg_sync(c), fn);
    if (armed) amd::throw_if_sync(*reinterpret_cast<int*>(o + M + 3), fn, "a persistent solve");
    h = o;
  }
  if (h[M + 2] != 0.0) glm_throw_y_bounds(fn, s.y, s.rows, 0, 1, s.row0);
  if (s.total_rows == 0 || !(p.any_var() || !propto)) return glm_result{};
  const double lp = h[0];
  if (!std::isfinite(lp)) {
    glm_throw_nonfinite_operands(fn, p, va);
    glm_throw_nonfinite_x(fn);
  }
  if (!p.any_var()) return glm_result{lp, nullptr};
  double* g = ChainableStack::instance_->memalloc_.alloc_array<double>(size_t(M + 2));
  for (int j = 0; j <= M; ++j) g[j] = h[1 + j];
  if (p.alpha_vec) return glm_result{lp, glm_vec_node(fn, lp, p, va, s.rows, nullptr, g, out + 2, M)};
  return glm_result{lp, new glm_dev_vari(lp, p.alpha_vi, p.beta_vi, p.beta_dev, nullptr, g, out + 2, M, fn)};
}

}  // namespace internal

/** Device-resident (y, x) -- the config-4 layout; one GPU or one shard. */
template <bool propto, typename T_alpha, typename T_beta>
inline auto bernoulli_logit_glm_lpmf(const glm_shard& s, const T_alpha& alpha, const T_beta& beta) {
  internal::glm_params p;
  internal::glm_alpha(p, alpha);
  internal::glm_beta(p, beta);
  return internal::glm_return<internal::glm_is_var<T_alpha>::value || internal::glm_is_var<T_beta>::value>(
      internal::glm_eval<propto>(s, p));
}

template <bool propto = false, typename T_alpha, typename T_beta>
inline auto bernoulli_logit_glm_lpmf(const dev_data<int>& y, const dev_data<double>& x,
                                     const T_alpha& alpha, const T_beta& beta) {
  return bernoulli_logit_glm_lpmf<propto>(internal::glm_shard_of("bernoulli_logit_glm_lpmf", y, x), alpha, beta);
}

/** Host data (uploaded per call, like the reference reading host memory). */
template <bool propto = false, typename T_alpha, typename T_beta>
inline auto bernoulli_logit_glm_lpmf(const std::vector<int>& y, const std::vector<double>& x_colmajor,
                                     int M, const T_alpha& alpha, const T_beta& beta) {
  const auto d = internal::glm_upload("bernoulli_logit_glm_lpmf", y, x_colmajor, M);
  return bernoulli_logit_glm_lpmf<propto>(d.y, d.x, alpha, beta);
}

/**
 * Row-sharded reducer (reduce_sum-style entry point): `shard` holds this
 * rank's rows with shard.distributed = true and the communicator joined via
 * amd::comm_init; every rank calls it with the same (alpha, beta) and gets the
 * full-data log density and gradient.
 */
template <bool propto = false, typename T_alpha, typename T_beta>
inline auto reduce_sum_bernoulli_logit_glm(const glm_shard& shard, const T_alpha& alpha,
                                           const T_beta& beta) {
  return bernoulli_logit_glm_lpmf<propto>(shard, alpha, beta);
}

}  // namespace math
}  // namespace stan
#endif
