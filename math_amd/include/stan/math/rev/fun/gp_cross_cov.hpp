#ifndef STAN_MATH_REV_FUN_GP_CROSS_COV_HPP
#define STAN_MATH_REV_FUN_GP_CROSS_COV_HPP

// The cross-covariance between two point sets: the (x1, x2, sigma,
// length_scale) overloads of gp_exp_quad_cov, gp_exponential_cov,
// gp_matern32_cov and gp_matern52_cov (Stan Math 3.0.0, prim/mat/fun/), what a
// GP's posterior mean K(x*, x) Kd^{-1} y and covariance are written with.
// K is n1 x n2 with K_ij = k(x1_i, x2_j), a general matrix: no diagonal, no
// symmetry; a coincident pair comes out of the family's expression as
// sigma^2 exactly.  This header has the scalar-point forms (std::vector<double>
// and device-resident dev_data<double>); the std::vector<Eigen vector> forms
// and the ARD form (std::vector<T_l> length_scale) are in eigen/interop.hpp
// and share the nodes below.
//
// The nodes are plain device nodes: K's values are formed in the constructor
// (smg_gp_cross_cov_fwd; a consumer always reads them, and a rectangle has no
// factorisation to generate them into, so nothing is deferred and there is no
// inverse-form adjoint), chain() reduces K's dense adjoint to the
// hyperparameter sums (smg_gp_cross_cov_rev, smg_gp_ard_cross_cov_rev) and
// hands them to the host varis as the single-x nodes' dense branch does.  With
// every hyperparameter data, chain() launches nothing.
//
// Argument checks: each function's single-x checks in their order and wording
// (gp_exp_quad_cov.hpp, gp_matern_cov.hpp, gp_ard_cov.hpp), the points checked
// as x1 then x2 under those names ("<fn>: x1 is nan, but must not be nan!"),
// the point sizes across both sets against the first point's.  As there, these
// are the reference's messages as recalled; its sources are not part of this
// repository and the messages could not be compared with them.
// One convention for the degenerate shapes, in every form: an empty x1 or x2
// gives an n1 x n2 matrix with no entries and no node on the tape; points
// without coordinates (Eigen vectors of size 0) are all at distance 0, so K is
// sigma^2 everywhere with a zero length-scale derivative.
// Not provided: the fvar<var> tangent, D > 64 for ARD.

#include <stan/math/rev/fun/gp_ard_cov.hpp>

#include <cmath>
#include <sstream>
#include <stdexcept>
#include <vector>

namespace stan {
namespace math {

namespace internal {

class gp_cross_cov_dev_vari : public device_vari {
 public:
  const int family_;
  const char* fn_;    // the function's name in error messages
  const double* x1_;  // D x n1 column-major (point i at x1_ + i D), kept alive with the tape
  const double* x2_;  // D x n2
  const int n1_, n2_, D_;
  const double sigma_d_, l_d_;
  vari* sigma_vi_;  // null when sigma is data
  vari* l_vi_;      // null when l is data
  dev_matrix_vari* K_;
  double* out2_;  // device [sigma', l']

  gp_cross_cov_dev_vari(int family, const char* fn, const double* x1, int n1, const double* x2, int n2, int D,
                        double sigma, vari* sigma_vi, double l, vari* l_vi)
      : device_vari(0.0),
        family_(family),
        fn_(fn),
        x1_(x1),
        x2_(x2),
        n1_(n1),
        n2_(n2),
        D_(D),
        sigma_d_(sigma),
        l_d_(l),
        sigma_vi_(sigma_vi),
        l_vi_(l_vi),
        K_(new dev_matrix_vari(n1, n2, dev_structure::general)),
        out2_(amd::alloc_doubles(2)) {
    amd::check(smg_gp_cross_cov_fwd(amd::ctx(), family_, x1_, n1_, x2_, n2_, D_, sigma_d_, l_d_, K_->raw_val(), n1_),
               fn_);
  }

  bool may_write_device_adjoint(const void*) const override { return false; }  // (host scalars only)

  void chain() override {
    if (!sigma_vi_ && !l_vi_) return;
    smg_ctx* c = amd::ctx();
    amd::check(smg_memset(c, out2_, 0, 2 * sizeof(double)), fn_);
    amd::check(smg_gp_cross_cov_rev(c, family_, x1_, n1_, x2_, n2_, D_, sigma_d_, l_d_, K_->adj(), n1_, out2_), fn_);
    if (sigma_vi_) add_pending_adjoint(sigma_vi_, out2_);
    if (l_vi_) add_pending_adjoint(l_vi_, out2_ + 1);
  }
};

/** One length scale per dimension: both sets scaled at construction
 * (smg_gp_ard_scale), K from the scaled points with l = 1. */
class gp_ard_cross_cov_dev_vari : public device_vari {
 public:
  const int family_;
  const char* fn_;
  const int n1_, n2_, D_;
  double* z1_;   // x1 / l, D x n1 point-major (the forward's input)
  double* z1t_;  // z1 coordinate-major, n1 x D (the reducer's input)
  double* z2_;
  double* z2t_;
  const double sigma_d_;
  double* l_d_;     // D host values (arena)
  vari* sigma_vi_;  // null when sigma is data
  vari** l_vis_;    // D varis, null when the length scales are data
  dev_matrix_vari* K_;
  double* out_;  // device [sigma', l_1' .. l_D']

  gp_ard_cross_cov_dev_vari(int family, const char* fn, const double* x1, int n1, const double* x2, int n2, int D,
                            double sigma, vari* sigma_vi, const double* l, vari* const* l_vis)
      : device_vari(0.0),
        family_(family),
        fn_(fn),
        n1_(n1),
        n2_(n2),
        D_(D),
        z1_(amd::alloc_doubles(size_t(n1) * D)),
        z1t_(amd::alloc_doubles(size_t(n1) * D)),
        z2_(amd::alloc_doubles(size_t(n2) * D)),
        z2t_(amd::alloc_doubles(size_t(n2) * D)),
        sigma_d_(sigma),
        l_d_(ChainableStack::instance_->memalloc_.alloc_array<double>(D)),
        sigma_vi_(sigma_vi),
        l_vis_(l_vis ? ChainableStack::instance_->memalloc_.alloc_array<vari*>(D) : nullptr),
        K_(new dev_matrix_vari(n1, n2, dev_structure::general)),
        out_(amd::alloc_doubles(size_t(1 + D))) {
    for (int d = 0; d < D; ++d) {
      l_d_[d] = l[d];
      if (l_vis_) l_vis_[d] = l_vis[d];
    }
    smg_ctx* c = amd::ctx();
    amd::check(smg_gp_ard_scale(c, x1, D_, n1_, l_d_, z1_, z1t_), fn_);
    amd::check(smg_gp_ard_scale(c, x2, D_, n2_, l_d_, z2_, z2t_), fn_);
    amd::check(smg_gp_cross_cov_fwd(c, family_, z1_, n1_, z2_, n2_, D_, sigma_d_, 1.0, K_->raw_val(), n1_), fn_);
  }

  bool may_write_device_adjoint(const void*) const override { return false; }  // (host scalars only)

  void chain() override {
    if (!sigma_vi_ && !l_vis_) return;
    smg_ctx* c = amd::ctx();
    amd::check(smg_memset(c, out_, 0, size_t(1 + D_) * sizeof(double)), fn_);
    amd::check(smg_gp_ard_cross_cov_rev(c, family_, z1t_, n1_, z2t_, n2_, D_, sigma_d_, l_d_, K_->adj(), n1_, out_), fn_);
    if (sigma_vi_) add_pending_adjoint(sigma_vi_, out_);
    if (l_vis_)
      for (int d = 0; d < D_; ++d) add_pending_adjoint(l_vis_[d], out_ + 1 + d);
  }
};

inline void gp_cross_throw_nan(const char* fn, const char* name) {
  std::ostringstream m;
  m << fn << ": " << name << " is nan, but must not be nan!";
  throw std::domain_error(m.str());
}
inline void gp_cross_check_not_nan(const char* fn, const char* name, const std::vector<double>& x) {
  for (size_t i = 0; i < x.size(); ++i)
    if (std::isnan(x[i])) gp_cross_throw_nan(fn, name);
}

/** The single-x functions' hyperparameter checks: gp_exp_quad_cov's
 * check_positive under the names of its (sigma, length_scale) kind
 * (rev/fun/gp_exp_quad_cov.hpp), the Matern family's positive and finite
 * "magnitude" / "length scale" (rev/fun/gp_matern_cov.hpp). */
inline void gp_cross_check_hyper(int family, const char* fn, double sigma, const vari* sigma_vi, double l,
                                 const vari* l_vi) {
  if (family != SMG_GP_EXP_QUAD) {
    gp_check_hyper(fn, sigma, l);
    return;
  }
  const bool vv = sigma_vi && l_vi, dv = !sigma_vi;
  gp_check_positive(fn, vv ? "sigma" : dv ? "marginal variance" : "magnitude", sigma);
  gp_check_positive(fn, vv ? "length_scale" : dv ? "length-scale" : "length scale", l);
}

/** The node over checked arguments (x1 D x n1 and x2 D x n2 on the device,
 * D >= 1); no node for a matrix without entries. */
inline dev_var_matrix gp_cross_cov_dev(int family, const char* fn, const dev_data<double>& x1,
                                       const dev_data<double>& x2, int D, double sigma, vari* sigma_vi, double l,
                                       vari* l_vi) {
  const int n1 = int(x1.size() / size_t(D)), n2 = int(x2.size() / size_t(D));
  if (n1 == 0 || n2 == 0) return dev_var_matrix(new dev_matrix_vari(n1, n2, dev_structure::general));
  auto* node = new gp_cross_cov_dev_vari(family, fn, x1.data(), n1, x2.data(), n2, D, sigma, sigma_vi, l, l_vi);
  return dev_var_matrix(node->K_);
}
inline dev_var_matrix gp_ard_cross_cov_dev(int family, const char* fn, const dev_data<double>& x1,
                                           const dev_data<double>& x2, int D, double sigma, vari* sigma_vi,
                                           const std::vector<double>& l, const std::vector<vari*>& l_vis) {
  const int n1 = int(x1.size() / size_t(D)), n2 = int(x2.size() / size_t(D));
  if (n1 == 0 || n2 == 0) return dev_var_matrix(new dev_matrix_vari(n1, n2, dev_structure::general));
  auto* node = new gp_ard_cross_cov_dev_vari(family, fn, x1.data(), n1, x2.data(), n2, D, sigma, sigma_vi, l.data(),
                                             l_vis.empty() ? nullptr : l_vis.data());
  return dev_var_matrix(node->K_);
}

/** Scalar points: x1 then x2 not NaN, then the hyperparameters. */
inline dev_var_matrix gp_cross_cov(int family, const char* fn, const std::vector<double>& x1,
                                   const std::vector<double>& x2, double sigma, vari* sigma_vi, double l,
                                   vari* l_vi) {
  gp_cross_check_not_nan(fn, "x1", x1);
  gp_cross_check_not_nan(fn, "x2", x2);
  gp_cross_check_hyper(family, fn, sigma, sigma_vi, l, l_vi);
  return gp_cross_cov_dev(family, fn, to_dev_data(x1), to_dev_data(x2), 1, sigma, sigma_vi, l, l_vi);
}
/** Device-resident scalar points: their entries are the caller's to check. */
inline dev_var_matrix gp_cross_cov(int family, const char* fn, const dev_data<double>& x1,
                                   const dev_data<double>& x2, double sigma, vari* sigma_vi, double l, vari* l_vi) {
  gp_cross_check_hyper(family, fn, sigma, sigma_vi, l, l_vi);
  return gp_cross_cov_dev(family, fn, x1, x2, 1, sigma, sigma_vi, l, l_vi);
}
}  // namespace internal

// (var, var), (double, var) and (var, double) for (sigma, length_scale), over
// two std::vector<double> and two device-resident point sets
#define STAN_MATH_AMD_GP_CROSS_OVERLOADS(FN, FAMILY, X)                                                      \
  inline dev_var_matrix FN(const X& x1, const X& x2, const var& sigma, const var& length_scale) {           \
    return internal::gp_cross_cov(FAMILY, #FN, x1, x2, sigma.val(), sigma.vi_, length_scale.val(),          \
                                  length_scale.vi_);                                                        \
  }                                                                                                         \
  inline dev_var_matrix FN(const X& x1, const X& x2, double sigma, const var& length_scale) {               \
    return internal::gp_cross_cov(FAMILY, #FN, x1, x2, sigma, nullptr, length_scale.val(),                  \
                                  length_scale.vi_);                                                        \
  }                                                                                                         \
  inline dev_var_matrix FN(const X& x1, const X& x2, const var& sigma, double length_scale) {               \
    return internal::gp_cross_cov(FAMILY, #FN, x1, x2, sigma.val(), sigma.vi_, length_scale, nullptr);      \
  }
#define STAN_MATH_AMD_GP_CROSS_BOTH(FN, FAMILY)                       \
  STAN_MATH_AMD_GP_CROSS_OVERLOADS(FN, FAMILY, std::vector<double>)   \
  STAN_MATH_AMD_GP_CROSS_OVERLOADS(FN, FAMILY, dev_data<double>)

STAN_MATH_AMD_GP_CROSS_BOTH(gp_exp_quad_cov, SMG_GP_EXP_QUAD)
STAN_MATH_AMD_GP_CROSS_BOTH(gp_exponential_cov, SMG_GP_EXPONENTIAL)
STAN_MATH_AMD_GP_CROSS_BOTH(gp_matern32_cov, SMG_GP_MATERN32)
STAN_MATH_AMD_GP_CROSS_BOTH(gp_matern52_cov, SMG_GP_MATERN52)

#undef STAN_MATH_AMD_GP_CROSS_BOTH
#undef STAN_MATH_AMD_GP_CROSS_OVERLOADS

}  // namespace math
}  // namespace stan
#endif
