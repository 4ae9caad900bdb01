// gp_periodic_cov and gp_dot_prod_cov (rev/fun/gp_periodic_cov.hpp,
// eigen/interop.hpp), over one point set and over two, through
// stan::math::gradient on the device.
//
// stdin, mode "bilinear":  f = sum(multiply(multiply(U, K), V)), data U (3 x n1), V (n2 x 2)
//   bilinear <per|dot> <kinds> <form 0|2|3> <D> <n1> <n2> sigma l p
//            x1(n1 D, point-major) [x2(n2 D)] U(3 n1, column-major) V(n2 2, column-major)
// kinds: per: one of v / d for each of (sigma, l, p), at least one v; theta
// holds the v arguments in that order, the d arguments are data.  dot: "v",
// theta = (sigma); l and p are read and ignored.  form 0: K(x1, x2) over host
// points (std::vector<double> for D == 1, otherwise std::vector<Eigen::VectorXd>);
// form 2: D == 1, device-resident points (dev_data<double>, made inside the
// functor: they live with the tape); form 3: the single-x overload K(x1, x1)
// over host points (n2 == n1, no x2 on stdin).
// mode "marginal":  the GP marginal likelihood on the stored-matrix path
//   marginal <per|sum> <N> sigma l p noise [sigma_dot] x(N) y(N)
//   K = gp_periodic_cov(x, sigma, l, p) [+ gp_dot_prod_cov(x, sigma_dot) for "sum"],
//   f = multi_normal_cholesky_lpdf(y | 0, cholesky_decompose(add_diag(K, noise^2)))
// Both print fx and the gradient of two evaluations (re-use of the recovered
// arenas), then the stack sizes.
// mode "degenerate":  degenerate <per|dot>
//   sum(K) with theta = (sigma, l, p) | (sigma): three points against two
//   points without coordinates (Eigen vectors of size 0), three such points
//   through the single-x overload, an empty x1 against two scalar points, and
//   an empty x through the single-x overload: one row [fx, gradient] each,
//   then the stack sizes.
// mode "errors": every argument check of the two functions, one line
// "<fn>|<case>|<exception type>|<message>" each.
#include <stan/math.hpp>
#include <cmath>
#include <cstdio>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

using stan::math::dev_var_matrix;
using stan::math::var;
using points = std::vector<Eigen::VectorXd>;

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

bool kinds_ok(const std::string& k) {
  if (k.size() != 3 || k == "ddd") return false;
  for (char c : k)
    if (c != 'v' && c != 'd') return false;
  return true;
}

// f(sigma, l, p) with each argument theta's next var or the data value, by `kinds`
template <typename T, typename F>
dev_var_matrix with_kinds(const std::string& kinds, const T& th, double sigma, double l, double p, const F& f) {
  if (kinds == "vvv") return f(th[0], th[1], th[2]);
  if (kinds == "vvd") return f(th[0], th[1], p);
  if (kinds == "vdv") return f(th[0], l, th[1]);
  if (kinds == "dvv") return f(sigma, th[0], th[1]);
  if (kinds == "vdd") return f(th[0], l, p);
  if (kinds == "dvd") return f(sigma, th[0], p);
  if (kinds == "ddv") return f(sigma, l, th[0]);
  throw std::runtime_error("unknown kinds " + kinds);
}

// ---------------------------------------------------------------- bilinear
template <typename X>
struct bilinear_functor {
  bool dot;
  const std::string& kinds;
  int form;
  const X& x1;
  const X& x2;
  double sigma, l, p;
  const std::vector<double>& U;  // 3 x n1
  const std::vector<double>& V;  // n2 x 2
  int n1, n2;

  template <typename T>
  var operator()(const T& th) const {
    using namespace stan::math;
    dev_var_matrix Kx;
    if (form == 3) {
      Kx = dot ? gp_dot_prod_cov(x1, th[0])
               : with_kinds(kinds, th, sigma, l, p, [&](const auto& s, const auto& ll, const auto& pp) {
                   return gp_periodic_cov(x1, s, ll, pp);
                 });
    } else if (form == 2) {
      if constexpr (std::is_same<X, std::vector<double>>::value) {
        const dev_data<double> d1 = to_dev_data(x1), d2 = to_dev_data(x2);
        Kx = dot ? gp_dot_prod_cov(d1, d2, th[0])
                 : with_kinds(kinds, th, sigma, l, p, [&](const auto& s, const auto& ll, const auto& pp) {
                     return gp_periodic_cov(d1, d2, s, ll, pp);
                   });
      } else {
        throw std::runtime_error("device-resident points are scalar");
      }
    } else {
      Kx = dot ? gp_dot_prod_cov(x1, x2, th[0])
               : with_kinds(kinds, th, sigma, l, p, [&](const auto& s, const auto& ll, const auto& pp) {
                   return gp_periodic_cov(x1, x2, s, ll, pp);
                 });
    }
    const dev_data<double> Ud = to_dev_data(U.data(), U.size(), 3, n1);
    const dev_data<double> Vd = to_dev_data(V.data(), V.size(), n2, 2);
    return sum(multiply(multiply(Ud, Kx), Vd));
  }
};

template <typename X>
int bilinear_grad(bool dot, const std::string& kinds, int form, const X& x1, const X& x2, double sigma, double l,
                  double p, const std::vector<double>& U, const std::vector<double>& V, int n1, int n2) {
  std::vector<double> th;
  if (dot) {
    th.push_back(sigma);
  } else {
    const double full[3] = {sigma, l, p};
    for (int i = 0; i < 3; ++i)
      if (kinds[i] == 'v') th.push_back(full[i]);
  }
  for (int rep = 0; rep < 2; ++rep) {
    double fx;
    std::vector<double> g;
    stan::math::gradient(bilinear_functor<X>{dot, kinds, form, x1, x2, sigma, l, p, U, V, n1, n2}, th, fx, g);
    print_row(fx, g);
  }
  print_stack();
  return 0;
}

int run_bilinear() {
  std::string fn, kinds;
  int form, D, n1, n2;
  double sigma, l, p;
  if (!(std::cin >> fn >> kinds >> form >> D >> n1 >> n2 >> sigma >> l >> p)) return 2;
  if (fn != "per" && fn != "dot") return 2;
  const bool dot = fn == "dot";
  if (D < 1 || n1 < 0 || n2 < 0 || (dot ? kinds != "v" : !kinds_ok(kinds))) return 2;
  if ((form != 0 && form != 2 && form != 3) || (form == 2 && D != 1) || (form == 3 && n1 != n2)) return 2;
  std::vector<double> x1(size_t(n1) * D), x2(form == 3 ? 0 : size_t(n2) * D), U(size_t(3) * n1), V(size_t(n2) * 2);
  if (!read(x1) || !read(x2) || !read(U) || !read(V)) return 2;
  if (form == 3) x2 = x1;
  if (D == 1) return bilinear_grad(dot, kinds, form, x1, x2, sigma, l, p, U, V, n1, n2);
  return bilinear_grad(dot, kinds, form, to_points(x1, n1, D), to_points(x2, n2, D), sigma, l, p, U, V, n1, n2);
}

// ---------------------------------------------------------- marginal likelihood
struct marginal_functor {
  bool with_dot;
  const std::vector<double>& x;
  const std::vector<double>& y;
  template <typename T>
  var operator()(const T& th) const {
    using namespace stan::math;
    dev_var_matrix K = gp_periodic_cov(x, th[0], th[1], th[2]);
    if (with_dot) K = add(K, gp_dot_prod_cov(x, th[4]));
    dev_var_matrix L = cholesky_decompose(add_diag(K, square(th[3])));
    const std::vector<double> mu(y.size(), 0.0);
    return multi_normal_cholesky_lpdf(y, mu, L);
  }
};

int run_marginal() {
  std::string kernel;
  int N;
  if (!(std::cin >> kernel >> N) || N < 1 || (kernel != "per" && kernel != "sum")) return 2;
  std::vector<double> th(kernel == "sum" ? 5 : 4), x(N), y(N);
  if (!read(th) || !read(x) || !read(y)) return 2;
  for (int rep = 0; rep < 2; ++rep) {
    double fx;
    std::vector<double> g;
    stan::math::gradient(marginal_functor{kernel == "sum", x, y}, th, fx, g);
    print_row(fx, g);
  }
  print_stack();
  return 0;
}

// --------------------------------------------------------------- degenerate
int run_degenerate() {
  std::string fn;
  if (!(std::cin >> fn) || (fn != "per" && fn != "dot")) return 2;
  const bool dot = fn == "dot";
  const points a(3, Eigen::VectorXd(0)), b(2, Eigen::VectorXd(0));
  const std::vector<double> none, xb = {0.25, 1.5};
  const std::vector<double> th = dot ? std::vector<double>{1.3} : std::vector<double>{1.3, 0.9, 1.7};
  auto row = [&](const auto& f) {
    double fx;
    std::vector<double> g;
    stan::math::gradient([&](const std::vector<var>& t) { return stan::math::sum(f(t)); }, th, fx, g);
    print_row(fx, g);
  };
  using namespace stan::math;
  row([&](const std::vector<var>& t) {
    return dot ? gp_dot_prod_cov(a, b, t[0]) : gp_periodic_cov(a, b, t[0], t[1], t[2]);
  });
  row([&](const std::vector<var>& t) { return dot ? gp_dot_prod_cov(a, t[0]) : gp_periodic_cov(a, t[0], t[1], t[2]); });
  row([&](const std::vector<var>& t) {
    return dot ? gp_dot_prod_cov(none, xb, t[0]) : gp_periodic_cov(none, xb, t[0], t[1], t[2]);
  });
  row([&](const std::vector<var>& t) {
    return dot ? gp_dot_prod_cov(none, t[0]) : gp_periodic_cov(none, t[0], t[1], t[2]);
  });
  print_stack();
  return 0;
}

// ------------------------------------------------------------------ errors
// sum(K) of one call under gradient() (the tape is recovered when it throws)
template <typename F>
void report(const char* fn, const char* what, std::vector<double> th, const F& f) {
  std::vector<double> g;
  double fx;
  try {
    stan::math::gradient([&](const std::vector<var>& t) { return stan::math::sum(f(t)); }, th, fx, g);
    std::printf("%s|%s|none|\n", fn, what);
  } catch (const std::domain_error& e) {
    std::printf("%s|%s|domain_error|%s\n", fn, what, e.what());
  } catch (const std::invalid_argument& e) {
    std::printf("%s|%s|invalid_argument|%s\n", fn, what, e.what());
  } catch (const std::exception& e) {
    std::printf("%s|%s|exception|%s\n", fn, what, e.what());
  }
}

// gp_periodic_cov, every hyperparameter a var: two sets, one set
template <typename X>
void per2(const char* what, const X& x1, const X& x2, double sigma, double l, double p) {
  report("gp_periodic_cov", what, {sigma, l, p},
         [&](const std::vector<var>& t) { return stan::math::gp_periodic_cov(x1, x2, t[0], t[1], t[2]); });
}
template <typename X>
void per1(const char* what, const X& x, double sigma, double l, double p) {
  report("gp_periodic_cov", what, {sigma, l, p},
         [&](const std::vector<var>& t) { return stan::math::gp_periodic_cov(x, t[0], t[1], t[2]); });
}
template <typename X>
void dot2(const char* what, const X& x1, const X& x2, double sigma) {
  report("gp_dot_prod_cov", what, {sigma},
         [&](const std::vector<var>& t) { return stan::math::gp_dot_prod_cov(x1, x2, t[0]); });
}
template <typename X>
void dot1(const char* what, const X& x, double sigma) {
  report("gp_dot_prod_cov", what, {sigma}, [&](const std::vector<var>& t) { return stan::math::gp_dot_prod_cov(x, t[0]); });
}

int run_errors() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> xa = {0.5, -1.0, 2.0}, xb = {0.25, 1.5}, xan = {0.5, nan, 2.0}, xbn = {nan, 1.5},
                            xai = {0.5, -1.0, inf}, xbi = {-inf, 1.5}, xani = {inf, nan, 2.0}, none;
  points pa(3, Eigen::VectorXd(3)), pb(2, Eigen::VectorXd(3)), pan, pbn, pai, pb2(2, Eigen::VectorXd(2)), pbad;
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
  pai = pa;
  pai[2](0) = inf;
  pbad = pa;  // x1's own points differ in size
  pbad[2] = Eigen::VectorXd(2);
  pbad[2](0) = pbad[2](1) = 1.0;

  // ---- gp_periodic_cov
  per2("ok", xa, xb, 1.3, 0.9, 1.7);
  per2("x1 empty", none, xb, 1.3, 0.9, 1.7);
  per2("x2 empty", xa, none, 1.3, 0.9, 1.7);
  per2("sigma=0", xa, xb, 0.0, 0.9, 1.7);
  per2("sigma=-1", xa, xb, -1.0, 0.9, 1.7);
  per2("sigma=nan", xa, xb, nan, 0.9, 1.7);
  per2("sigma=inf", xa, xb, inf, 0.9, 1.7);
  per2("l=0", xa, xb, 1.3, 0.0, 1.7);
  per2("l=-1", xa, xb, 1.3, -1.0, 1.7);
  per2("l=nan", xa, xb, 1.3, nan, 1.7);
  per2("l=inf", xa, xb, 1.3, inf, 1.7);
  per2("p=0", xa, xb, 1.3, 0.9, 0.0);
  per2("p=-1", xa, xb, 1.3, 0.9, -1.0);
  per2("p=nan", xa, xb, 1.3, 0.9, nan);
  per2("p=inf", xa, xb, 1.3, 0.9, inf);
  per2("sigma=0, l=0, p=0", xa, xb, 0.0, 0.0, 0.0);  // the first wins
  per2("l=0, p=0", xa, xb, 1.3, 0.0, 0.0);
  per2("x1 nan", xan, xb, 1.3, 0.9, 1.7);
  per2("x2 nan", xa, xbn, 1.3, 0.9, 1.7);
  per2("x1 nan, x2 nan", xan, xbn, 1.3, 0.9, 1.7);
  per2("x1 nan, p=0", xan, xb, 1.3, 0.9, 0.0);  // the hyperparameters before the points
  per2("x2 nan, sigma=0", xa, xbn, 0.0, 0.9, 1.7);
  report("gp_periodic_cov", "dvv l=0", {0.0, 1.7},
         [&](const std::vector<var>& t) { return stan::math::gp_periodic_cov(xa, xb, 1.3, t[0], t[1]); });
  report("gp_periodic_cov", "vdd sigma=0", {0.0},
         [&](const std::vector<var>& t) { return stan::math::gp_periodic_cov(xa, xb, t[0], 0.9, 1.7); });
  report("gp_periodic_cov", "ddv sigma=0", {1.7},
         [&](const std::vector<var>& t) { return stan::math::gp_periodic_cov(xa, xb, 0.0, 0.9, t[0]); });
  report("gp_periodic_cov", "ddv p=0", {0.0},
         [&](const std::vector<var>& t) { return stan::math::gp_periodic_cov(xa, xb, 1.3, 0.9, t[0]); });
  per1("single ok", xa, 1.3, 0.9, 1.7);
  per1("single empty", none, 1.3, 0.9, 1.7);
  per1("single x nan", xan, 1.3, 0.9, 1.7);
  per1("single x nan, l=0", xan, 1.3, 0.0, 1.7);
  per1("single p=inf", xa, 1.3, 0.9, inf);
  per2("points ok", pa, pb, 1.3, 0.9, 1.7);
  per2("points x1 nan", pan, pb, 1.3, 0.9, 1.7);
  per2("points x2 nan", pa, pbn, 1.3, 0.9, 1.7);
  per2("points x1 nan, x2 nan", pan, pbn, 1.3, 0.9, 1.7);
  per2("points sigma=0", pa, pb, 0.0, 0.9, 1.7);
  per2("points x2 nan, p=0", pa, pbn, 1.3, 0.9, 0.0);
  per2("points sizes across", pa, pb2, 1.3, 0.9, 1.7);
  per2("points sizes within x1", pbad, pb, 1.3, 0.9, 1.7);
  per2("points sizes across, l=0", pa, pb2, 1.3, 0.0, 1.7);  // the hyperparameters before the sizes
  per2("points sizes across, x1 nan", pan, pb2, 1.3, 0.9, 1.7);  // the entries before the sizes
  per1("single points ok", pa, 1.3, 0.9, 1.7);
  per1("single points x nan", pan, 1.3, 0.9, 1.7);
  per1("single points sizes", pbad, 1.3, 0.9, 1.7);

  // ---- gp_dot_prod_cov
  dot2("ok", xa, xb, 1.3);
  dot2("x1 empty", none, xb, 1.3);
  dot2("x2 empty", xa, none, 1.3);
  dot2("sigma=0", xa, xb, 0.0);
  dot2("sigma=-1", xa, xb, -1.0);
  dot2("sigma=nan", xa, xb, nan);
  dot2("sigma=inf", xa, xb, inf);
  dot2("sigma=-inf", xa, xb, -inf);
  dot2("x1 nan", xan, xb, 1.3);
  dot2("x2 nan", xa, xbn, 1.3);
  dot2("x1 inf", xai, xb, 1.3);
  dot2("x2 inf", xa, xbi, 1.3);
  dot2("x1 inf then nan", xani, xb, 1.3);  // entry by entry: the first offending entry
  dot2("x1 inf, x2 nan", xai, xbn, 1.3);
  dot2("x1 nan, sigma=-1", xan, xb, -1.0);  // sigma before the points
  dot2("x2 inf, sigma=inf", xa, xbi, inf);
  dot1("single ok", xa, 1.3);
  dot1("single empty", none, 1.3);
  dot1("single sigma=0", xa, 0.0);
  dot1("single x nan", xan, 1.3);
  dot1("single x inf", xai, 1.3);
  dot1("single x nan, sigma=nan", xan, nan);
  dot2("points ok", pa, pb, 1.3);
  dot2("points x1 nan", pan, pb, 1.3);
  dot2("points x2 nan", pa, pbn, 1.3);
  dot2("points x1 inf", pai, pb, 1.3);
  dot2("points x1 inf, x2 nan", pai, pbn, 1.3);
  dot2("points sigma=-1", pa, pb, -1.0);
  dot2("points sizes across", pa, pb2, 1.3);
  dot2("points sizes within x1", pbad, pb, 1.3);
  dot2("points sizes across, sigma=-1", pa, pb2, -1.0);
  dot1("single points ok", pa, 1.3);
  dot1("single points x inf", pai, 1.3);
  dot1("single points sizes", pbad, 1.3);
  print_stack();
  return 0;
}

int main() {
  std::string mode;
  if (!(std::cin >> mode)) return 2;
  if (mode == "errors") return run_errors();
  if (mode == "bilinear") return run_bilinear();
  if (mode == "marginal") return run_marginal();
  if (mode == "degenerate") return run_degenerate();
  return 2;
}
