#ifndef STAN_MATH_REV_FUN_GP_ARD_COV_HPP
#define STAN_MATH_REV_FUN_GP_ARD_COV_HPP

// gp_exp_quad_cov, gp_exponential_cov, gp_matern32_cov and gp_matern52_cov
// with one length scale per input dimension (ARD): the
// (std::vector<Eigen vector> x, sigma, std::vector<T_l> length_scale)
// overloads, declared in eigen/interop.hpp.  The reference computes them as
// divide_columns(x, length_scale) followed by the kernel of unit length scale;
// the node below does the same on the device: z = x / l once at construction
// (smg_gp_ard_scale, which also writes the coordinate-major copy the reducers
// read), then
//   values     smg_gp_cov_fwd(family, z, D, n, sigma, 1.0), deferred as
//              gp_exp_quad_cov's are
//   gp_source  {family, D, n, x = z, sigma, l = 1}: under add_diag ->
//              cholesky_decompose the factorisation generates K + d I from z
//              straight into the factor's buffer, K never formed
//   reverse    sigma' and l_1' .. l_D' in one pass over K^{-1}
//              (smg_gp_ard_cov_inverse_adjoint), or over K's dense adjoint when
//              K has another consumer (smg_gp_ard_cov_rev).
// With t_d = (x_id - x_jd) / l_d, r^2 = sum_d t_d^2 and a = c r:
//   dK_ij/dl_d = sigma^2 h(a) t_d^2 / l_d,   h = exp(-r^2 / 2) | exp(-a) / a |
//   3 exp(-a) | (5/3)(1 + a) exp(-a)   (c = 1, 1, sqrt 3, sqrt 5).
//
// Argument checks, in this order: every x entry is not NaN ("<fn>: x is nan,
// but must not be nan!"), sigma positive and finite under the name
// "magnitude", every length scale in order under "length scale[<d + 1>]"
// (std::domain_error), then std::invalid_argument for the number of length
// scales against the points' dimension, for more than SMG_GP_ARD_MAX_D of
// them, and for points of unequal sizes (as gp_points_to_device reports it).
// As for the Matern families these are the reference's messages as recalled;
// its sources are not part of this repository.
// The cross-covariance (x1, x2) overloads are rev/fun/gp_cross_cov.hpp.
// Not provided: the fvar<var> tangent, scalar x with a one-element
// length-scale vector, D > 64.

#include <stan/math/rev/fun/gp_matern_cov.hpp>

#include <cmath>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace stan {
namespace math {

namespace internal {

class gp_ard_cov_dev_vari : public device_vari, public structured_adjoint_sink, public deferred_value_source {
 public:
  const int family_;
  const char* fn_;   // the function's name in error messages
  const double* x_;  // D x n column-major (point i at x_ + i D), kept alive with the tape
  double* z_;        // x / l, the same layout (the forward's and the generator's input)
  double* zt_;       // z coordinate-major, n x D (the reducers' input)
  const int n_;
  const int D_;
  const double sigma_d_;
  double* l_d_;      // D host values (arena)
  vari* sigma_vi_;   // null when sigma is data
  vari** l_vis_;     // D varis, null when the length scales are data (arena: a vari is never destroyed)
  dev_matrix_vari* K_;
  double* out_;      // device [sigma', l_1' .. l_D']
  size_t pos_;       // this node's index in var_stack_
  inverse_adjoint dep_, exp_;  // as gp_exp_quad_cov_dev_vari's

  gp_ard_cov_dev_vari(int family, const char* fn, const double* x, int n, int D, double sigma, vari* sigma_vi,
                      const double* l, vari* const* l_vis)
      : device_vari(0.0),
        family_(family),
        fn_(fn),
        x_(x),
        z_(amd::alloc_doubles(size_t(n) * D)),
        zt_(amd::alloc_doubles(size_t(n) * D)),
        n_(n),
        D_(D),
        sigma_d_(sigma),
        l_d_(ChainableStack::instance_->memalloc_.alloc_array<double>(D)),
        sigma_vi_(sigma_vi),
        l_vis_(l_vis ? ChainableStack::instance_->memalloc_.alloc_array<vari*>(D) : nullptr),
        K_(new dev_matrix_vari(n, n, dev_structure::symmetric)),
        out_(amd::alloc_doubles(size_t(1 + D))),
        pos_(ChainableStack::instance_->var_stack_.size() - 1) {
    for (int d = 0; d < D; ++d) {
      l_d_[d] = l[d];
      if (l_vis_) l_vis_[d] = l_vis[d];
    }
    amd::check(smg_gp_ard_scale(amd::ctx(), x_, D_, n_, l_d_, z_, zt_), fn_);
    K_->sink_ = this;
    if (amd::deferred_values_enabled())
      K_->defer_values(this);
    else
      form_values(K_);
  }

  void form_values(dev_matrix_vari*) override {
    amd::check(smg_gp_cov_fwd(amd::ctx(), family_, z_, D_, n_, sigma_d_, 1.0, K_->raw_val(), n_), fn_);
  }

  bool gp_source(smg_gp_source* out) override {
    if (!std::isfinite(sigma_d_)) return false;
    out->family = family_;
    out->D = D_;
    out->n = n_;
    out->x = z_;
    out->sigma = sigma_d_;
    out->l = 1.0;
    out->d = 0.0;
    return true;
  }

  bool may_write_device_adjoint(const void*) const override { return false; }  // (host scalars only)

  bool wants_out() const { return sigma_vi_ || l_vis_; }
  void deposit_out() {
    if (sigma_vi_) add_pending_adjoint(sigma_vi_, out_);
    if (l_vis_)
      for (int d = 0; d < D_; ++d) add_pending_adjoint(l_vis_[d], out_ + 1 + d);
  }

  // one deposit per sweep, reduced right away (gp_exp_quad_cov_dev_vari::take_inverse_adjoint);
  // K_ij is always recomputed from z
  bool take_inverse_adjoint(const inverse_adjoint& d, double* dadj) override {
    if (d.n != n_) return false;
    if (dep_.C && dep_.sweep == ChainableStack::instance_->sweep_) return false;
    amd::check(smg_gp_ard_cov_inverse_adjoint(amd::ctx(), family_, d.C, n_, n_, d.s, d.k, d.ss, d.adj, zt_, D_, sigma_d_,
                                              l_d_, dadj, wants_out() ? out_ : nullptr),
               fn_);
    dep_ = d;
    return true;
  }

  void expand_adjoint() override {
    const size_t sw = ChainableStack::instance_->sweep_;
    if (exp_.C && exp_.sweep == sw) exp_.expand_into(K_->adj());
    exp_ = inverse_adjoint{};
    if (dep_.C && dep_.sweep == sw) dep_.expand_into(K_->adj());
    dep_ = inverse_adjoint{};
  }

  void chain() override {
    auto* st = ChainableStack::instance_;
    if (dep_.C && dep_.sweep == st->sweep_) {
      const inverse_adjoint d = dep_;
      dep_ = inverse_adjoint{};
      if (!others_write_device_adjoint(pos_, K_, d.owner)) {
        deposit_out();
        exp_ = d;
        return;
      }
      d.expand_into(K_->adj());  // another node wrote K's adjoint too: the dense sum
    }
    if (!wants_out()) return;
    smg_ctx* c = amd::ctx();
    amd::check(smg_memset(c, out_, 0, size_t(1 + D_) * sizeof(double)), fn_);
    amd::check(smg_gp_ard_cov_rev(c, family_, zt_, D_, n_, sigma_d_, l_d_, K_->adj(), n_, out_), fn_);
    deposit_out();
  }
};

/** The checks on the hyperparameters and the count of length scales (after
 * the x entries', before the point sizes'). */
inline void gp_ard_check_hyper(const char* fn, double sigma, const std::vector<double>& l, size_t D) {
  gp_check_positive_finite(fn, "magnitude", sigma);
  for (size_t d = 0; d < l.size(); ++d) {
    const std::string name = "length scale[" + std::to_string(d + 1) + "]";
    gp_check_positive_finite(fn, name.c_str(), l[d]);
  }
  if (l.size() != D) {
    std::ostringstream m;
    m << fn << ": x dimension (" << D << ") and number of length scales (" << l.size() << ") must match in size";
    throw std::invalid_argument(m.str());
  }
  if (l.size() > size_t(SMG_GP_ARD_MAX_D)) {
    std::ostringstream m;
    m << fn << ": number of length scales (" << l.size() << ") exceeds the supported " << SMG_GP_ARD_MAX_D;
    throw std::invalid_argument(m.str());
  }
}

/** The node over checked arguments (x D x n on the device, D == l.size()). */
inline dev_var_matrix gp_ard_cov_dev(int family, const char* fn, const dev_data<double>& x, int D, double sigma,
                                     vari* sigma_vi, const std::vector<double>& l, const std::vector<vari*>& l_vis) {
  const int n = D > 0 ? int(x.size() / size_t(D)) : 0;
  auto* node = new gp_ard_cov_dev_vari(family, fn, x.data(), n, D, sigma, sigma_vi, l.data(),
                                       l_vis.empty() ? nullptr : l_vis.data());
  return dev_var_matrix(node->K_);
}

}  // namespace internal
}  // namespace math
}  // namespace stan
#endif
