#ifndef STAN_MATH_REV_FUN_GP_PERIODIC_COV_HPP
#define STAN_MATH_REV_FUN_GP_PERIODIC_COV_HPP

// gp_periodic_cov and gp_dot_prod_cov (Stan Math 3.0.0, prim/mat/fun/), each
// over one point set, K(x, x), and over two, K(x1, x2):
//   gp_periodic_cov(x, sigma, l, p), gp_periodic_cov(x1, x2, sigma, l, p)
//     K_ij = sigma^2 exp(-2 sin^2(pi d_ij / p) / l^2)
//     each of sigma, l, p a var or a double, at least one of them a var
//   gp_dot_prod_cov(x, sigma), gp_dot_prod_cov(x1, x2, sigma), sigma a var
//     K_ij = sigma^2 + x1_i . x2_j
// d_ij is |x1_i - x2_j| for scalar points, the Euclidean distance otherwise.
// This header has the nodes and the scalar-point forms (std::vector<double> and
// device-resident dev_data<double>); the std::vector<Eigen vector> forms are in
// eigen/interop.hpp and share the nodes.  x as var is not provided, nor are the
// all-double forms (no tape function), ARD, or the fvar<var> tangent.
//
// The nodes are plain device nodes, as gp_cross_cov.hpp's: K's values are
// formed in the constructor (smg_gp_periodic_cov_fwd, smg_gp_dot_prod_cov_fwd),
// chain() reduces K's dense adjoint to the hyperparameter sums (the _rev
// entries) and hands them to the host varis; hyperparameters that are data have
// null varis and are skipped, and with all of them data chain() launches
// nothing.  They are no source of the fused factorisation and take no
// inverse-form adjoint: cholesky_decompose(add_diag(K, s)) reads K's stored
// values and writes its adjoint densely.  K(x, x) is computed by the same
// entries with x1 == x2, is bitwise symmetric, and carries
// dev_structure::symmetric as the other single-x covariances do (one host vari
// per (i, j), (j, i) pair when K crosses to the host); K(x1, x2) is general.
//
// Argument checks, all std::domain_error, in this order.  These are the
// reference's messages as recalled; its sources are not part of this
// repository and the messages could not be compared with them.
//   gp_periodic_cov: "signal standard deviation", "length-scale", "period"
//     "<fn>: <name> is <v>, but must be > 0!" (a NaN fails, infinity passes, as
//     in gp_exp_quad_cov), then every point entry: "<fn>: element of x is nan,
//     but must not be nan!" (two sets: "element of x1", then "element of x2").
//   gp_dot_prod_cov: sigma not NaN, ">= 0", finite under the name "sigma", then
//     every point entry not NaN and finite under "x" ("x1", then "x2").
// Device-resident points are the caller's to check.  Point sizes that differ
// throw gp_cross_cov's std::invalid_argument (eigen/interop.hpp).  Degenerate
// shapes follow gp_cross_cov.hpp: an empty set gives a matrix without entries
// and no node; points without coordinates are all coincident (periodic: K =
// sigma^2 everywhere with zero l- and p-derivatives; dot product: K = sigma^2).

#include <stan/math/rev/fun/gp_cross_cov.hpp>

#include <cmath>
#include <sstream>
#include <stdexcept>
#include <type_traits>
#include <vector>

namespace stan {
namespace math {

namespace internal {

class gp_periodic_cov_dev_vari : public device_vari {
 public:
  const char* fn_;
  const double* x1_;  // D x n1 column-major (point i at x1_ + i D), kept alive with the tape
  const double* x2_;  // D x n2 (x1_ itself for K(x, x))
  const int n1_, n2_, D_;
  const double sigma_d_, l_d_, p_d_;
  vari* sigma_vi_;  // each null when that hyperparameter is data
  vari* l_vi_;
  vari* p_vi_;
  dev_matrix_vari* K_;
  double* out3_;  // device [sigma', l', p']

  gp_periodic_cov_dev_vari(const char* fn, const double* x1, int n1, const double* x2, int n2, int D, double sigma,
                           vari* sigma_vi, double l, vari* l_vi, double p, vari* p_vi, dev_structure s)
      : device_vari(0.0),
        fn_(fn),
        x1_(x1),
        x2_(x2),
        n1_(n1),
        n2_(n2),
        D_(D),
        sigma_d_(sigma),
        l_d_(l),
        p_d_(p),
        sigma_vi_(sigma_vi),
        l_vi_(l_vi),
        p_vi_(p_vi),
        K_(new dev_matrix_vari(n1, n2, s)),
        out3_(amd::alloc_doubles(3)) {
    amd::check(smg_gp_periodic_cov_fwd(amd::ctx(), x1_, n1_, x2_, n2_, D_, sigma_d_, l_d_, p_d_, K_->raw_val(), n1_),
               fn_);
  }

  bool may_write_device_adjoint(const void*) const override { return false; }  // (host scalars only)

  void chain() override {
    if (!sigma_vi_ && !l_vi_ && !p_vi_) return;
    smg_ctx* c = amd::ctx();
    amd::check(smg_memset(c, out3_, 0, 3 * sizeof(double)), fn_);
    amd::check(smg_gp_periodic_cov_rev(c, x1_, n1_, x2_, n2_, D_, sigma_d_, l_d_, p_d_, K_->adj(), n1_, out3_), fn_);
    if (sigma_vi_) add_pending_adjoint(sigma_vi_, out3_);
    if (l_vi_) add_pending_adjoint(l_vi_, out3_ + 1);
    if (p_vi_) add_pending_adjoint(p_vi_, out3_ + 2);
  }
};

class gp_dot_prod_cov_dev_vari : public device_vari {
 public:
  const char* fn_;
  const int n1_, n2_;
  const double sigma_d_;
  vari* sigma_vi_;  // null when sigma is data
  dev_matrix_vari* K_;
  double* out1_;  // device [sigma']

  gp_dot_prod_cov_dev_vari(const char* fn, const double* x1, int n1, const double* x2, int n2, int D, double sigma,
                           vari* sigma_vi, dev_structure s)
      : device_vari(0.0),
        fn_(fn),
        n1_(n1),
        n2_(n2),
        sigma_d_(sigma),
        sigma_vi_(sigma_vi),
        K_(new dev_matrix_vari(n1, n2, s)),
        out1_(amd::alloc_doubles(1)) {
    amd::check(smg_gp_dot_prod_cov_fwd(amd::ctx(), x1, n1_, x2, n2_, D, sigma_d_, K_->raw_val(), n1_), fn_);
  }

  bool may_write_device_adjoint(const void*) const override { return false; }  // (host scalars only)

  void chain() override {
    if (!sigma_vi_) return;
    smg_ctx* c = amd::ctx();
    amd::check(smg_memset(c, out1_, 0, sizeof(double)), fn_);
    amd::check(smg_gp_dot_prod_cov_rev(c, n1_, n2_, sigma_d_, K_->adj(), n1_, out1_), fn_);
    add_pending_adjoint(sigma_vi_, out1_);
  }
};

/** A hyperparameter argument, var or arithmetic: its value and its vari (null for data). */
template <typename T>
struct gp_hyper_is_var : std::is_same<std::decay_t<T>, var> {};
template <typename T>
struct gp_hyper_ok : std::integral_constant<bool, gp_hyper_is_var<T>::value || std::is_arithmetic<std::decay_t<T>>::value> {
};
inline double gp_hyper_val(const var& v) { return v.val(); }
inline double gp_hyper_val(double v) { return v; }
inline vari* gp_hyper_vi(const var& v) { return v.vi_; }
inline vari* gp_hyper_vi(double) { return nullptr; }
/** sigma, l, p each a var or a number, at least one a var */
template <typename T_s, typename T_l, typename T_p>
using gp_periodic_kinds = std::enable_if_t<gp_hyper_ok<T_s>::value && gp_hyper_ok<T_l>::value && gp_hyper_ok<T_p>::value &&
                                           (gp_hyper_is_var<T_s>::value || gp_hyper_is_var<T_l>::value ||
                                            gp_hyper_is_var<T_p>::value)>;

/** gp_periodic_cov's hyperparameters, values and varis, and their checks (the header comment) */
struct gp_periodic_hyper {
  double sigma;
  vari* sigma_vi;
  double l;
  vari* l_vi;
  double p;
  vari* p_vi;
  void check(const char* fn) const {
    gp_check_positive(fn, "signal standard deviation", sigma);
    gp_check_positive(fn, "length-scale", l);
    gp_check_positive(fn, "period", p);
  }
};
template <typename T_s, typename T_l, typename T_p>
inline gp_periodic_hyper gp_periodic_hyper_of(const T_s& sigma, const T_l& l, const T_p& p) {
  return gp_periodic_hyper{gp_hyper_val(sigma), gp_hyper_vi(sigma), gp_hyper_val(l), gp_hyper_vi(l),
                           gp_hyper_val(p),     gp_hyper_vi(p)};
}

inline void gp_dot_prod_throw(const char* fn, const char* name, double v, const char* must) {
  std::ostringstream m;
  m << fn << ": " << name << " is " << v << ", but must " << must << "!";
  throw std::domain_error(m.str());
}
inline void gp_dot_prod_check_sigma(const char* fn, double sigma) {
  if (std::isnan(sigma)) gp_dot_prod_throw(fn, "sigma", sigma, "not be nan");
  if (!(sigma >= 0)) gp_dot_prod_throw(fn, "sigma", sigma, "be >= 0");
  if (!std::isfinite(sigma)) gp_dot_prod_throw(fn, "sigma", sigma, "be finite");
}
/** one point entry of gp_dot_prod_cov: not NaN, then finite */
inline void gp_dot_prod_check_entry(const char* fn, const char* name, double v) {
  if (std::isnan(v)) gp_dot_prod_throw(fn, name, v, "not be nan");
  if (!std::isfinite(v)) gp_dot_prod_throw(fn, name, v, "be finite");
}
inline void gp_dot_prod_check_x(const char* fn, const char* name, const std::vector<double>& x) {
  for (size_t i = 0; i < x.size(); ++i) gp_dot_prod_check_entry(fn, name, x[i]);
}

/** The nodes over checked arguments (x1 D x n1 and x2 D x n2 on the device,
 * D >= 1; K(x, x): x1 and x2 the same set, s symmetric); no node for a matrix
 * without entries. */
inline dev_var_matrix gp_periodic_cov_dev(const char* fn, const dev_data<double>& x1, const dev_data<double>& x2, int D,
                                          const gp_periodic_hyper& h, dev_structure s) {
  const int n1 = int(x1.size() / size_t(D)), n2 = int(x2.size() / size_t(D));
  if (n1 == 0 || n2 == 0) return dev_var_matrix(new dev_matrix_vari(n1, n2, s));
  auto* node = new gp_periodic_cov_dev_vari(fn, x1.data(), n1, x2.data(), n2, D, h.sigma, h.sigma_vi, h.l, h.l_vi, h.p,
                                            h.p_vi, s);
  return dev_var_matrix(node->K_);
}
inline dev_var_matrix gp_dot_prod_cov_dev(const char* fn, const dev_data<double>& x1, const dev_data<double>& x2, int D,
                                          double sigma, vari* sigma_vi, dev_structure s) {
  const int n1 = int(x1.size() / size_t(D)), n2 = int(x2.size() / size_t(D));
  if (n1 == 0 || n2 == 0) return dev_var_matrix(new dev_matrix_vari(n1, n2, s));
  auto* node = new gp_dot_prod_cov_dev_vari(fn, x1.data(), n1, x2.data(), n2, D, sigma, sigma_vi, s);
  return dev_var_matrix(node->K_);
}
}  // namespace internal

// ---- gp_periodic_cov over scalar points
template <typename T_s, typename T_l, typename T_p, typename = internal::gp_periodic_kinds<T_s, T_l, T_p>>
inline dev_var_matrix gp_periodic_cov(const std::vector<double>& x, const T_s& sigma, const T_l& l, const T_p& p) {
  const char* fn = "gp_periodic_cov";
  const internal::gp_periodic_hyper h = internal::gp_periodic_hyper_of(sigma, l, p);
  h.check(fn);
  internal::gp_cross_check_not_nan(fn, "element of x", x);
  const dev_data<double> xd = to_dev_data(x);
  return internal::gp_periodic_cov_dev(fn, xd, xd, 1, h, dev_structure::symmetric);
}
template <typename T_s, typename T_l, typename T_p, typename = internal::gp_periodic_kinds<T_s, T_l, T_p>>
inline dev_var_matrix gp_periodic_cov(const std::vector<double>& x1, const std::vector<double>& x2, const T_s& sigma,
                                      const T_l& l, const T_p& p) {
  const char* fn = "gp_periodic_cov";
  const internal::gp_periodic_hyper h = internal::gp_periodic_hyper_of(sigma, l, p);
  h.check(fn);
  internal::gp_cross_check_not_nan(fn, "element of x1", x1);
  internal::gp_cross_check_not_nan(fn, "element of x2", x2);
  return internal::gp_periodic_cov_dev(fn, to_dev_data(x1), to_dev_data(x2), 1, h, dev_structure::general);
}
/** Device-resident scalar points: their entries are the caller's to check. */
template <typename T_s, typename T_l, typename T_p, typename = internal::gp_periodic_kinds<T_s, T_l, T_p>>
inline dev_var_matrix gp_periodic_cov(const dev_data<double>& x, const T_s& sigma, const T_l& l, const T_p& p) {
  const char* fn = "gp_periodic_cov";
  const internal::gp_periodic_hyper h = internal::gp_periodic_hyper_of(sigma, l, p);
  h.check(fn);
  return internal::gp_periodic_cov_dev(fn, x, x, 1, h, dev_structure::symmetric);
}
template <typename T_s, typename T_l, typename T_p, typename = internal::gp_periodic_kinds<T_s, T_l, T_p>>
inline dev_var_matrix gp_periodic_cov(const dev_data<double>& x1, const dev_data<double>& x2, const T_s& sigma,
                                      const T_l& l, const T_p& p) {
  const char* fn = "gp_periodic_cov";
  const internal::gp_periodic_hyper h = internal::gp_periodic_hyper_of(sigma, l, p);
  h.check(fn);
  return internal::gp_periodic_cov_dev(fn, x1, x2, 1, h, dev_structure::general);
}

// ---- gp_dot_prod_cov over scalar points
inline dev_var_matrix gp_dot_prod_cov(const std::vector<double>& x, const var& sigma) {
  const char* fn = "gp_dot_prod_cov";
  internal::gp_dot_prod_check_sigma(fn, sigma.val());
  internal::gp_dot_prod_check_x(fn, "x", x);
  const dev_data<double> xd = to_dev_data(x);
  return internal::gp_dot_prod_cov_dev(fn, xd, xd, 1, sigma.val(), sigma.vi_, dev_structure::symmetric);
}
inline dev_var_matrix gp_dot_prod_cov(const std::vector<double>& x1, const std::vector<double>& x2, const var& sigma) {
  const char* fn = "gp_dot_prod_cov";
  internal::gp_dot_prod_check_sigma(fn, sigma.val());
  internal::gp_dot_prod_check_x(fn, "x1", x1);
  internal::gp_dot_prod_check_x(fn, "x2", x2);
  return internal::gp_dot_prod_cov_dev(fn, to_dev_data(x1), to_dev_data(x2), 1, sigma.val(), sigma.vi_,
                                       dev_structure::general);
}
/** Device-resident scalar points: their entries are the caller's to check. */
inline dev_var_matrix gp_dot_prod_cov(const dev_data<double>& x, const var& sigma) {
  const char* fn = "gp_dot_prod_cov";
  internal::gp_dot_prod_check_sigma(fn, sigma.val());
  return internal::gp_dot_prod_cov_dev(fn, x, x, 1, sigma.val(), sigma.vi_, dev_structure::symmetric);
}
inline dev_var_matrix gp_dot_prod_cov(const dev_data<double>& x1, const dev_data<double>& x2, const var& sigma) {
  const char* fn = "gp_dot_prod_cov";
  internal::gp_dot_prod_check_sigma(fn, sigma.val());
  return internal::gp_dot_prod_cov_dev(fn, x1, x2, 1, sigma.val(), sigma.vi_, dev_structure::general);
}

}  // namespace math
}  // namespace stan
#endif
