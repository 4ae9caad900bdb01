// The GP marginal gradient of tests/cpp/test_gp_tape.cpp with the covariance
// chosen on stdin: gp_exponential_cov, gp_matern32_cov or gp_matern52_cov
// (rev/fun/gp_matern_cov.hpp), through stan::math::gradient on the device.
//
// stdin, mode "grad":
//   grad <family> <mixed 0|1> <vv|dv|vd> <D> <N> sigma l noise x(N D, point-major) y(N)
// vv: theta = (sigma, l, noise); dv: sigma is data, theta = (l, noise); vd: l
// is data, theta = (sigma, noise).  D == 1: std::vector<double> x, otherwise
// std::vector<Eigen::VectorXd>.  mixed: + 1e-3 sum(L), the factor's second
// consumer (the dense-adjoint fallback).  Prints fx and the gradient of two
// evaluations (re-use of the recovered arenas), then the stack sizes.
// mode "time" (measurement, no check):
//   time <family | exp_quad> <steps> <N> sigma l noise x(N) y(N)
// prints the wall time of each of <steps> gradient evaluations after three
// warm-up evaluations (the closed-form schedule is taken from the second on).
// mode "errors": every argument check of the three functions, one line
// "<fn>|<case>|<exception type>|<message>" each.
#include <stan/math.hpp>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

using stan::math::var;

template <typename X, typename S, typename L>
stan::math::dev_var_matrix cov(const std::string& family, const X& x, const S& sigma, const L& l) {
  if (family == "exponential") return stan::math::gp_exponential_cov(x, sigma, l);
  if (family == "matern32") return stan::math::gp_matern32_cov(x, sigma, l);
  if (family == "matern52") return stan::math::gp_matern52_cov(x, sigma, l);
  if (family == "exp_quad") return stan::math::gp_exp_quad_cov(x, sigma, l);  // the yardstick of mode "time"
  throw std::runtime_error("unknown family " + family);
}

template <typename X>
struct gp_functor {
  const std::string& family;
  const std::string& kinds;  // vv | dv | vd
  const X& x;
  const std::vector<double>& y;
  bool mixed;
  double sigma, l;  // the data argument's value (dv / vd)
  template <typename T>
  var operator()(const T& th) const {
    using namespace stan::math;
    dev_var_matrix K = kinds == "vv"   ? cov(family, x, th[0], th[1])
                       : kinds == "dv" ? cov(family, x, sigma, th[0])
                                       : cov(family, x, th[0], l);
    auto Kd = add_diag(K, square(th[th.size() - 1]));
    auto L = cholesky_decompose(Kd);
    std::vector<double> mu(y.size(), 0.0);
    var lp = multi_normal_cholesky_lpdf(y, mu, L);
    if (mixed) lp += 1e-3 * sum(L);
    return lp;
  }
};

template <typename X>
int run_grad(const std::string& family, const std::string& kinds, bool mixed, const X& x,
             const std::vector<double>& y, const std::vector<double>& full) {
  std::vector<double> th;
  if (kinds == "vv") th = full;
  else if (kinds == "dv") th = {full[1], full[2]};
  else th = {full[0], full[2]};
  for (int rep = 0; rep < 2; ++rep) {
    double fx;
    std::vector<double> g;
    stan::math::gradient(gp_functor<X>{family, kinds, x, y, mixed, full[0], full[1]}, th, fx, g);
    std::printf("%.17g", fx);
    for (double v : g) std::printf(" %.17g", v);  // as many entries as theta has
    std::printf("\n");
  }
  std::printf("stack %zu %zu\n", stan::math::ChainableStack::instance_->var_stack_.size(),
              stan::math::ChainableStack::instance_->dev_adj_stack_.size());
  return 0;
}

// sum(K) of one covariance call under gradient() (the tape is recovered when it throws)
template <typename X>
void report(const std::string& family, const char* what, const X& x, double sigma, double l) {
  const std::string fn = "gp_" + family + "_cov";
  std::vector<double> th = {sigma, l}, g;
  double fx;
  try {
    stan::math::gradient(
        [&](const std::vector<var>& t) { return stan::math::sum(cov(family, x, t[0], t[1])); }, th, fx, g);
    std::printf("%s|%s|none|\n", fn.c_str(), what);
  } catch (const std::domain_error& e) {
    std::printf("%s|%s|domain_error|%s\n", fn.c_str(), what, e.what());
  } catch (const std::invalid_argument& e) {
    std::printf("%s|%s|invalid_argument|%s\n", fn.c_str(), what, e.what());
  } catch (const std::exception& e) {
    std::printf("%s|%s|exception|%s\n", fn.c_str(), what, e.what());
  }
}

int run_errors() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> x = {0.5, -1.0, 2.0}, xn = {0.5, nan, 2.0};
  std::vector<Eigen::VectorXd> pts(3, Eigen::VectorXd(3)), bad(3, Eigen::VectorXd(3)), pn(3, Eigen::VectorXd(3));
  for (int i = 0; i < 3; ++i)
    for (int d = 0; d < 3; ++d) pts[i](d) = bad[i](d) = pn[i](d) = 0.25 * i - 0.5 * d;
  bad[2] = Eigen::VectorXd(2);
  bad[2](0) = bad[2](1) = 1.0;
  pn[1](2) = nan;
  for (const char* f : {"exponential", "matern32", "matern52"}) {
    const std::string family = f;
    report(family, "ok", x, 1.3, 0.9);
    report(family, "sigma=0", x, 0.0, 0.9);
    report(family, "sigma=-1", x, -1.0, 0.9);
    report(family, "sigma=inf", x, inf, 0.9);
    report(family, "l=0", x, 1.3, 0.0);
    report(family, "l=inf", x, 1.3, inf);
    report(family, "x nan", xn, 1.3, 0.9);
    report(family, "x nan, sigma=0, l=0", xn, 0.0, 0.0);  // the first check in order
    report(family, "sigma=0, l=0", x, 0.0, 0.0);
    report(family, "points ok", pts, 1.3, 0.9);
    report(family, "points size", bad, 1.3, 0.9);
    report(family, "points nan", pn, 1.3, 0.9);
    report(family, "points sigma=0", pts, 0.0, 0.9);
    report(family, "points l=inf", pts, 1.3, inf);
    report(family, "points size, l=0", bad, 1.3, 0.0);  // the hyperparameters before the sizes
  }
  std::printf("stack %zu %zu\n", stan::math::ChainableStack::instance_->var_stack_.size(),
              stan::math::ChainableStack::instance_->dev_adj_stack_.size());
  return 0;
}

int run_time() {
  std::string family;
  int steps, N;
  std::vector<double> th(3);
  if (!(std::cin >> family >> steps >> N >> th[0] >> th[1] >> th[2]) || N < 0) return 2;
  std::vector<double> x(N), y(N);
  for (auto& v : x)
    if (!(std::cin >> v)) return 2;
  for (auto& v : y)
    if (!(std::cin >> v)) return 2;
  const std::string kinds = "vv";
  for (int rep = 0; rep < 3 + steps; ++rep) {
    double fx;
    std::vector<double> g;
    const auto t0 = std::chrono::steady_clock::now();
    stan::math::gradient(gp_functor<std::vector<double>>{family, kinds, x, y, false, th[0], th[1]}, th, fx, g);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rep >= 3) std::printf("step %d %.3f ms fx %.17g grad %.17g %.17g %.17g\n", rep - 3, ms, fx, g[0], g[1], g[2]);
  }
  return 0;
}

int main() {
  std::string mode;
  if (!(std::cin >> mode)) return 2;
  if (mode == "errors") return run_errors();
  if (mode == "time") return run_time();
  if (mode != "grad") return 2;
  std::string family, kinds;
  int mixed, D, N;
  std::vector<double> th(3);
  if (!(std::cin >> family >> mixed >> kinds >> D >> N >> th[0] >> th[1] >> th[2])) return 2;
  if (D < 1 || N < 0 || (kinds != "vv" && kinds != "dv" && kinds != "vd")) return 2;
  std::vector<double> xs(size_t(N) * D), y(N);
  for (auto& v : xs)
    if (!(std::cin >> v)) return 2;
  for (auto& v : y)
    if (!(std::cin >> v)) return 2;
  if (D == 1) return run_grad(family, kinds, mixed != 0, xs, y, th);
  std::vector<Eigen::VectorXd> pts(N, Eigen::VectorXd(D));
  for (int i = 0; i < N; ++i)
    for (int d = 0; d < D; ++d) pts[i](d) = xs[size_t(i) * D + d];
  return run_grad(family, kinds, mixed != 0, pts, y, th);
}
