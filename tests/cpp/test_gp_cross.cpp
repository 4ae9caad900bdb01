// The cross-covariance overloads (x1, x2, sigma, length_scale) of
// gp_exp_quad_cov / gp_exponential_cov / gp_matern32_cov / gp_matern52_cov
// (rev/fun/gp_cross_cov.hpp, eigen/interop.hpp) through stan::math::gradient on
// the device.
//
// stdin, mode "bilinear":  f = sum(multiply(multiply(U, K(x1, x2)), V)), data U (3 x n1), V (n2 x 2)
//   bilinear <family> <vv|dv|vd> <form 0|1|2> <D> <n1> <n2> sigma l(1, or D with form 1)
//            x1(n1 D, point-major) x2(n2 D) U(3 n1, column-major) V(n2 2, column-major)
// vv: theta = (sigma, l..); dv: sigma is data, theta = (l..); vd: the length
// scale(s) are data, theta = (sigma).  form 0: one length scale, host points
// (std::vector<double> for D == 1, otherwise std::vector<Eigen::VectorXd>);
// form 1: ARD over Eigen points; form 2: D == 1, device-resident points
// (dev_data<double>, made inside the functor: they live with the tape).
// mode "mean":  the GP posterior mean's weighted sum, theta = (sigma, l, noise):
//   mean <family> <N> <m> sigma l noise x(N) xs(m) y(N) w(m)
//   K = cov(x, sigma, l), L = cholesky_decompose(add_diag(K, noise^2)),
//   alpha = L^-T L^-1 y (mdivide_left_tri), f = sum(multiply(w, multiply(cov(xs, x, sigma, l), alpha)))
// Both print fx and the gradient of two evaluations (re-use of the recovered
// arenas), then the stack sizes.
// mode "degenerate":  degenerate <family>
//   sum(K(x1, x2)) with theta = (sigma, l) for three points against two points
//   without coordinates (Eigen vectors of size 0), the same through the ARD
//   form with no length scales (theta = (sigma)), and for an empty x1 against
//   two scalar points: one row [fx, gradient] each, then the stack sizes.
// mode "errors": every argument check of the four functions, one line
// "<fn>|<case>|<exception type>|<message>" each.
#include <stan/math.hpp>
#include <cmath>
#include <cstdio>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

using stan::math::var;
using points = std::vector<Eigen::VectorXd>;

template <typename X, typename S, typename L>
stan::math::dev_var_matrix cov(const std::string& family, const X& x, const S& sigma, const L& l) {
  if (family == "exp_quad") return stan::math::gp_exp_quad_cov(x, sigma, l);
  if (family == "exponential") return stan::math::gp_exponential_cov(x, sigma, l);
  if (family == "matern32") return stan::math::gp_matern32_cov(x, sigma, l);
  if (family == "matern52") return stan::math::gp_matern52_cov(x, sigma, l);
  throw std::runtime_error("unknown family " + family);
}

template <typename X, typename S, typename L>
stan::math::dev_var_matrix cross(const std::string& family, const X& x1, const X& x2, const S& sigma, const L& l) {
  if (family == "exp_quad") return stan::math::gp_exp_quad_cov(x1, x2, sigma, l);
  if (family == "exponential") return stan::math::gp_exponential_cov(x1, x2, sigma, l);
  if (family == "matern32") return stan::math::gp_matern32_cov(x1, x2, sigma, l);
  if (family == "matern52") return stan::math::gp_matern52_cov(x1, x2, sigma, l);
  throw std::runtime_error("unknown family " + family);
}

bool read(std::vector<double>& v) {
  for (auto& e : v)
    if (!(std::cin >> e)) return false;
  return true;
}

points to_points(const std::vector<double>& flat, int n, int D) {
  points p(n, Eigen::VectorXd(D));
  for (int i = 0; i < n; ++i)
    for (int d = 0; d < D; ++d) p[i](d) = flat[size_t(i) * D + d];
  return p;
}

void print_row(double fx, const std::vector<double>& g) {
  std::printf("%.17g", fx);
  for (double v : g) std::printf(" %.17g", v);  // as many entries as theta has
  std::printf("\n");
}

void print_stack() {
  std::printf("stack %zu %zu\n", stan::math::ChainableStack::instance_->var_stack_.size(),
              stan::math::ChainableStack::instance_->dev_adj_stack_.size());
}

// ---------------------------------------------------------------- bilinear
template <typename X>
struct bilinear_functor {
  const std::string& family;
  const std::string& kinds;
  bool ard;
  bool dev;  // scalar points handed over as dev_data<double>
  const X& x1;
  const X& x2;
  double sigma;                  // the data arguments' values (dv / vd)
  const std::vector<double>& l;  // one entry, or D with ard
  const std::vector<double>& U;  // 3 x n1
  const std::vector<double>& V;  // n2 x 2
  int n1, n2;

  // the ARD overloads exist for Eigen points only
  template <typename S, typename L>
  stan::math::dev_var_matrix ard_cross(const S& s, const L& lv) const {
    if constexpr (std::is_same<X, points>::value)
      return cross(family, x1, x2, s, lv);
    else
      throw std::runtime_error("ard needs D-dimensional points");
  }

  // one length scale: the host points, or their device-resident copies
  template <typename S, typename L>
  stan::math::dev_var_matrix one_l_cross(const S& s, const L& lv) const {
    if constexpr (std::is_same<X, std::vector<double>>::value) {
      if (dev) return cross(family, stan::math::to_dev_data(x1), stan::math::to_dev_data(x2), s, lv);
    }
    return cross(family, x1, x2, s, lv);
  }

  template <typename T>
  var operator()(const T& th) const {
    using namespace stan::math;
    const size_t nl = l.size();
    dev_var_matrix Kx;
    if (kinds == "vv")
      Kx = ard ? ard_cross(th[0], std::vector<var>(th.begin() + 1, th.begin() + 1 + nl))
               : one_l_cross(th[0], th[1]);
    else if (kinds == "dv")
      Kx = ard ? ard_cross(sigma, std::vector<var>(th.begin(), th.begin() + nl)) : one_l_cross(sigma, th[0]);
    else
      Kx = ard ? ard_cross(th[0], l) : one_l_cross(th[0], l[0]);
    const dev_data<double> Ud = to_dev_data(U.data(), U.size(), 3, n1);
    const dev_data<double> Vd = to_dev_data(V.data(), V.size(), n2, 2);
    return sum(multiply(multiply(Ud, Kx), Vd));
  }
};

template <typename X>
int bilinear_grad(const std::string& family, const std::string& kinds, bool ard, bool dev, const X& x1, const X& x2,
                  double sigma, const std::vector<double>& l, const std::vector<double>& U,
                  const std::vector<double>& V, int n1, int n2) {
  std::vector<double> th;
  if (kinds != "dv") th.push_back(sigma);
  if (kinds != "vd") th.insert(th.end(), l.begin(), l.end());
  for (int rep = 0; rep < 2; ++rep) {
    double fx;
    std::vector<double> g;
    stan::math::gradient(bilinear_functor<X>{family, kinds, ard, dev, x1, x2, sigma, l, U, V, n1, n2}, th, fx, g);
    print_row(fx, g);
  }
  print_stack();
  return 0;
}

int run_bilinear() {
  std::string family, kinds;
  int form, D, n1, n2;
  double sigma;
  if (!(std::cin >> family >> kinds >> form >> D >> n1 >> n2 >> sigma)) return 2;
  if (D < 1 || n1 < 0 || n2 < 0 || (kinds != "vv" && kinds != "dv" && kinds != "vd")) return 2;
  if (form < 0 || form > 2 || (form == 2 && D != 1)) return 2;
  const bool ard = form == 1;
  std::vector<double> l(ard ? D : 1), x1(size_t(n1) * D), x2(size_t(n2) * D), U(size_t(3) * n1), V(size_t(n2) * 2);
  if (!read(l) || !read(x1) || !read(x2) || !read(U) || !read(V)) return 2;
  if (D == 1 && !ard) return bilinear_grad(family, kinds, false, form == 2, x1, x2, sigma, l, U, V, n1, n2);
  return bilinear_grad(family, kinds, ard, false, to_points(x1, n1, D), to_points(x2, n2, D), sigma, l, U, V, n1, n2);
}

// ---------------------------------------------------------- posterior mean
struct mean_functor {
  const std::string& family;
  const std::vector<double>& x;
  const std::vector<double>& xs;
  const std::vector<double>& y;
  const std::vector<double>& w;
  template <typename T>
  var operator()(const T& th) const {
    using namespace stan::math;
    const int N = int(x.size()), m = int(xs.size());
    dev_var_matrix K = cov(family, x, th[0], th[1]);
    dev_var_matrix L = cholesky_decompose(add_diag(K, square(th[2])));
    const dev_data<double> yd = to_dev_data(y.data(), y.size(), N, 1);
    dev_var_matrix alpha = mdivide_left_tri<Eigen::Upper>(transpose(L), mdivide_left_tri<Eigen::Lower>(L, yd));
    dev_var_matrix Ks = cross(family, xs, x, th[0], th[1]);
    const dev_data<double> wd = to_dev_data(w.data(), w.size(), 1, m);
    return sum(multiply(wd, multiply(Ks, alpha)));
  }
};

int run_mean() {
  std::string family;
  int N, m;
  std::vector<double> th(3);
  if (!(std::cin >> family >> N >> m >> th[0] >> th[1] >> th[2]) || N < 1 || m < 1) return 2;
  std::vector<double> x(N), xs(m), y(N), w(m);
  if (!read(x) || !read(xs) || !read(y) || !read(w)) return 2;
  for (int rep = 0; rep < 2; ++rep) {
    double fx;
    std::vector<double> g;
    stan::math::gradient(mean_functor{family, x, xs, y, w}, th, fx, g);
    print_row(fx, g);
  }
  print_stack();
  return 0;
}

// ------------------------------------------------------------------ errors
// sum(K(x1, x2)) of one call under gradient() (the tape is recovered when it throws)
template <typename F>
void report(const std::string& family, const char* what, std::vector<double> th, const F& f) {
  const std::string fn = "gp_" + family + "_cov";
  std::vector<double> g;
  double fx;
  try {
    stan::math::gradient([&](const std::vector<var>& t) { return stan::math::sum(f(t)); }, th, fx, g);
    std::printf("%s|%s|none|\n", fn.c_str(), what);
  } catch (const std::domain_error& e) {
    std::printf("%s|%s|domain_error|%s\n", fn.c_str(), what, e.what());
  } catch (const std::invalid_argument& e) {
    std::printf("%s|%s|invalid_argument|%s\n", fn.c_str(), what, e.what());
  } catch (const std::exception& e) {
    std::printf("%s|%s|exception|%s\n", fn.c_str(), what, e.what());
  }
}

// the (var, var) scalar-length-scale overload
template <typename X>
void rep_vv(const std::string& family, const char* what, const X& x1, const X& x2, double sigma, double l) {
  report(family, what, {sigma, l},
         [&](const std::vector<var>& t) { return cross(family, x1, x2, t[0], t[1]); });
}
// (double, var) and (var, double): gp_exp_quad_cov names its arguments by the kind
template <typename X>
void rep_dv(const std::string& family, const char* what, const X& x1, const X& x2, double sigma, double l) {
  report(family, what, {l}, [&](const std::vector<var>& t) { return cross(family, x1, x2, sigma, t[0]); });
}
template <typename X>
void rep_vd(const std::string& family, const char* what, const X& x1, const X& x2, double sigma, double l) {
  report(family, what, {sigma}, [&](const std::vector<var>& t) { return cross(family, x1, x2, t[0], l); });
}
void rep_ard(const std::string& family, const char* what, const points& x1, const points& x2, double sigma,
             const std::vector<double>& l) {
  std::vector<double> th = {sigma};
  th.insert(th.end(), l.begin(), l.end());
  report(family, what, th, [&](const std::vector<var>& t) {
    return cross(family, x1, x2, t[0], std::vector<var>(t.begin() + 1, t.end()));
  });
}

int run_errors() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> xa = {0.5, -1.0, 2.0}, xb = {0.25, 1.5}, xan = {0.5, nan, 2.0}, xbn = {nan, 1.5}, none;
  points pa(3, Eigen::VectorXd(3)), pb(2, Eigen::VectorXd(3)), pan, pbn, pb2(2, Eigen::VectorXd(2)), pbad, pnone;
  for (int i = 0; i < 3; ++i)
    for (int d = 0; d < 3; ++d) pa[i](d) = 0.25 * i - 0.5 * d;
  for (int i = 0; i < 2; ++i)
    for (int d = 0; d < 3; ++d) pb[i](d) = 0.4 * i + 0.3 * d;
  for (int i = 0; i < 2; ++i)
    for (int d = 0; d < 2; ++d) pb2[i](d) = 1.0 + i + d;
  pan = pa;
  pan[1](2) = nan;
  pbn = pb;
  pbn[0](1) = nan;
  pbad = pa;  // x1's own points differ in size
  pbad[2] = Eigen::VectorXd(2);
  pbad[2](0) = pbad[2](1) = 1.0;
  const std::vector<double> l3 = {0.9, 1.1, 1.4}, l2 = {0.9, 1.1}, l65(65, 1.2);
  for (const char* f : {"exp_quad", "exponential", "matern32", "matern52"}) {
    const std::string family = f;
    rep_vv(family, "ok", xa, xb, 1.3, 0.9);
    rep_vv(family, "x1 empty", none, xb, 1.3, 0.9);
    rep_vv(family, "x2 empty", xa, none, 1.3, 0.9);
    rep_vv(family, "x1 nan", xan, xb, 1.3, 0.9);
    rep_vv(family, "x2 nan", xa, xbn, 1.3, 0.9);
    rep_vv(family, "x1 nan, x2 nan", xan, xbn, 1.3, 0.9);  // the first wins
    rep_vv(family, "x2 nan, sigma=0, l=0", xa, xbn, 0.0, 0.0);
    rep_vv(family, "sigma=0", xa, xb, 0.0, 0.9);
    rep_vv(family, "sigma=-1", xa, xb, -1.0, 0.9);
    rep_vv(family, "sigma=inf", xa, xb, inf, 0.9);
    rep_vv(family, "l=0", xa, xb, 1.3, 0.0);
    rep_vv(family, "l=-1", xa, xb, 1.3, -1.0);
    rep_vv(family, "l=inf", xa, xb, 1.3, inf);
    rep_vv(family, "sigma=0, l=0", xa, xb, 0.0, 0.0);
    rep_dv(family, "dv sigma=0", xa, xb, 0.0, 0.9);
    rep_dv(family, "dv l=0", xa, xb, 1.3, 0.0);
    rep_vd(family, "vd sigma=0", xa, xb, 0.0, 0.9);
    rep_vd(family, "vd l=0", xa, xb, 1.3, 0.0);
    rep_vv(family, "points ok", pa, pb, 1.3, 0.9);
    rep_vv(family, "points x1 nan", pan, pb, 1.3, 0.9);
    rep_vv(family, "points x2 nan", pa, pbn, 1.3, 0.9);
    rep_vv(family, "points x1 nan, x2 nan", pan, pbn, 1.3, 0.9);
    rep_vv(family, "points sigma=0", pa, pb, 0.0, 0.9);
    rep_vv(family, "points l=inf", pa, pb, 1.3, inf);
    rep_vv(family, "points l=-1", pa, pb, 1.3, -1.0);
    rep_vv(family, "points sizes across", pa, pb2, 1.3, 0.9);
    rep_vv(family, "points sizes within x1", pbad, pb, 1.3, 0.9);
    rep_vv(family, "points sizes across, l=0", pa, pb2, 1.3, 0.0);  // the hyperparameters before the sizes
    rep_vv(family, "points x2 nan, sigma=0", pa, pbn, 0.0, 0.9);    // gp_exp_quad_cov: the hyperparameters first
    rep_ard(family, "ard ok", pa, pb, 1.3, l3);
    rep_ard(family, "ard x1 empty", pnone, pb, 1.3, l3);
    rep_ard(family, "ard x1 nan", pan, pb, 1.3, l3);
    rep_ard(family, "ard x2 nan", pa, pbn, 1.3, l3);
    rep_ard(family, "ard x1 nan, x2 nan, sigma=0", pan, pbn, 0.0, l3);
    rep_ard(family, "ard sigma=0", pa, pb, 0.0, l3);
    rep_ard(family, "ard sigma=inf", pa, pb, inf, l3);
    rep_ard(family, "ard l2=0", pa, pb, 1.3, {0.9, 0.0, 1.4});
    rep_ard(family, "ard l3=inf", pa, pb, 1.3, {0.9, 1.1, inf});
    rep_ard(family, "ard l1=-1, l2=0", pa, pb, 1.3, {-1.0, 0.0, 1.4});
    rep_ard(family, "ard count", pa, pb, 1.3, l2);
    rep_ard(family, "ard count 65", pa, pb, 1.3, l65);
    rep_ard(family, "ard sizes across", pa, pb2, 1.3, l3);
    rep_ard(family, "ard sizes across, count", pa, pb2, 1.3, l2);  // the count before the point sizes
  }
  print_stack();
  return 0;
}

int run_degenerate() {
  std::string family;
  if (!(std::cin >> family)) return 2;
  const points a(3, Eigen::VectorXd(0)), b(2, Eigen::VectorXd(0));
  const std::vector<double> none, xb = {0.25, 1.5};
  double fx;
  std::vector<double> g;
  stan::math::gradient(
      [&](const std::vector<var>& t) { return stan::math::sum(cross(family, a, b, t[0], t[1])); },
      std::vector<double>{1.3, 0.9}, fx, g);
  print_row(fx, g);
  stan::math::gradient(
      [&](const std::vector<var>& t) { return stan::math::sum(cross(family, a, b, t[0], std::vector<var>())); },
      std::vector<double>{1.3}, fx, g);
  print_row(fx, g);
  stan::math::gradient(
      [&](const std::vector<var>& t) { return stan::math::sum(cross(family, none, xb, t[0], t[1])); },
      std::vector<double>{1.3, 0.9}, fx, g);
  print_row(fx, g);
  print_stack();
  return 0;
}

int main() {
  std::string mode;
  if (!(std::cin >> mode)) return 2;
  if (mode == "errors") return run_errors();
  if (mode == "bilinear") return run_bilinear();
  if (mode == "mean") return run_mean();
  if (mode == "degenerate") return run_degenerate();
  return 2;
}
