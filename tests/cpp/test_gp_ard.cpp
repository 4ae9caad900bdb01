// The GP marginal gradient with one length scale per input dimension (ARD):
// gp_exp_quad_cov / gp_exponential_cov / gp_matern32_cov / gp_matern52_cov
// over std::vector<Eigen::VectorXd> x and a std::vector of length scales
// (rev/fun/gp_ard_cov.hpp), through stan::math::gradient on the device.
//
// stdin, mode "grad":
//   grad <family> <mixed 0|1> <vv|dv|vd> <deferred 0|1> <D> <N> sigma l_1..l_D noise x(N D, point-major) y(N)
// vv: theta = (sigma, l_1..l_D, noise); dv: sigma is data, theta = (l_1..l_D,
// noise); vd: the length scales are data, theta = (sigma, noise).  mixed:
// + 1e-3 sum(L), the factor's second consumer (the dense-adjoint fallback).
// deferred 0: amd::set_deferred_values(false).  Prints fx and the gradient of
// two evaluations (re-use of the recovered arenas), then
// "materialised <amd::materialisation_count()>", then the stack sizes.
// mode "time" (measurement, no check):
//   time <family> <ard 0|1> <steps> <D> <N> sigma l_1..l_D noise x(N D) y(N)
// prints the wall time of each of <steps> gradient evaluations after three
// warm-up evaluations; ard 0: the scalar overload with l_1 on the same points.
// mode "errors": the argument checks of the four functions, one line
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
using points = std::vector<Eigen::VectorXd>;

template <typename S, typename L>
stan::math::dev_var_matrix cov(const std::string& family, const points& x, const S& sigma, const L& l) {
  if (family == "exp_quad") return stan::math::gp_exp_quad_cov(x, sigma, l);
  if (family == "exponential") return stan::math::gp_exponential_cov(x, sigma, l);
  if (family == "matern32") return stan::math::gp_matern32_cov(x, sigma, l);
  if (family == "matern52") return stan::math::gp_matern52_cov(x, sigma, l);
  throw std::runtime_error("unknown family " + family);
}

struct gp_functor {
  const std::string& family;
  const std::string& kinds;  // vv | dv | vd | sc (time: the scalar-length-scale overload)
  const points& x;
  const std::vector<double>& y;
  bool mixed;
  double sigma;                  // the data arguments' values (dv / vd)
  const std::vector<double>& l;
  template <typename T>
  var operator()(const T& th) const {
    using namespace stan::math;
    const size_t D = l.size();
    dev_var_matrix K;
    if (kinds == "vv")
      K = cov(family, x, th[0], std::vector<var>(th.begin() + 1, th.begin() + 1 + D));
    else if (kinds == "dv")
      K = cov(family, x, sigma, std::vector<var>(th.begin(), th.begin() + D));
    else if (kinds == "vd")
      K = cov(family, x, th[0], l);
    else
      K = cov(family, x, th[0], th[1]);
    auto Kd = add_diag(K, square(th[th.size() - 1]));
    auto L = cholesky_decompose(Kd);
    std::vector<double> mu(y.size(), 0.0);
    var lp = multi_normal_cholesky_lpdf(y, mu, L);
    if (mixed) lp += 1e-3 * sum(L);
    return lp;
  }
};

bool read_problem(int D, int N, double& sigma, std::vector<double>& l, double& noise, points& x,
                  std::vector<double>& y) {
  l.resize(D);
  if (!(std::cin >> sigma)) return false;
  for (auto& v : l)
    if (!(std::cin >> v)) return false;
  if (!(std::cin >> noise)) return false;
  x.assign(N, Eigen::VectorXd(D));
  for (int i = 0; i < N; ++i)
    for (int d = 0; d < D; ++d)
      if (!(std::cin >> x[i](d))) return false;
  y.resize(N);
  for (auto& v : y)
    if (!(std::cin >> v)) return false;
  return true;
}

int run_grad() {
  std::string family, kinds;
  int mixed, deferred, D, N;
  if (!(std::cin >> family >> mixed >> kinds >> deferred >> D >> N)) return 2;
  if (D < 1 || N < 0 || (kinds != "vv" && kinds != "dv" && kinds != "vd")) return 2;
  double sigma, noise;
  std::vector<double> l, y;
  points x;
  if (!read_problem(D, N, sigma, l, noise, x, y)) return 2;
  std::vector<double> th;
  if (kinds != "dv") th.push_back(sigma);
  if (kinds != "vd") th.insert(th.end(), l.begin(), l.end());
  th.push_back(noise);
  stan::math::amd::set_deferred_values(deferred != 0);
  for (int rep = 0; rep < 2; ++rep) {
    double fx;
    std::vector<double> g;
    stan::math::gradient(gp_functor{family, kinds, x, y, mixed != 0, sigma, l}, th, fx, g);
    std::printf("%.17g", fx);
    for (double v : g) std::printf(" %.17g", v);  // as many entries as theta has
    std::printf("\n");
  }
  std::printf("materialised %zu\n", stan::math::amd::materialisation_count());
  std::printf("stack %zu %zu\n", stan::math::ChainableStack::instance_->var_stack_.size(),
              stan::math::ChainableStack::instance_->dev_adj_stack_.size());
  return 0;
}

// sum(K) of one covariance call under gradient() (the tape is recovered when it throws)
void report(const std::string& family, const char* what, const points& x, double sigma,
            const std::vector<double>& l) {
  const std::string fn = "gp_" + family + "_cov";
  std::vector<double> th = {sigma}, g;
  th.insert(th.end(), l.begin(), l.end());
  double fx;
  try {
    stan::math::gradient(
        [&](const std::vector<var>& t) {
          return stan::math::sum(cov(family, x, t[0], std::vector<var>(t.begin() + 1, t.end())));
        },
        th, fx, g);
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
  points pts(3, Eigen::VectorXd(3)), bad(3, Eigen::VectorXd(3)), pn(3, Eigen::VectorXd(3)), none;
  for (int i = 0; i < 3; ++i)
    for (int d = 0; d < 3; ++d) pts[i](d) = bad[i](d) = pn[i](d) = 0.25 * i - 0.5 * d;
  bad[2] = Eigen::VectorXd(2);
  bad[2](0) = bad[2](1) = 1.0;
  pn[1](2) = nan;
  points wide(2, Eigen::VectorXd(65));
  for (int i = 0; i < 2; ++i)
    for (int d = 0; d < 65; ++d) wide[i](d) = 0.01 * d + i;
  const std::vector<double> l3 = {0.9, 1.1, 1.4}, l2 = {0.9, 1.1}, l65(65, 1.2);
  for (const char* f : {"exp_quad", "exponential", "matern32", "matern52"}) {
    const std::string family = f;
    report(family, "ok", pts, 1.3, l3);
    report(family, "empty", none, 1.3, l3);
    report(family, "sigma=0", pts, 0.0, l3);
    report(family, "sigma=inf", pts, inf, l3);
    report(family, "l2=0", pts, 1.3, {0.9, 0.0, 1.4});
    report(family, "l3=inf", pts, 1.3, {0.9, 1.1, inf});
    report(family, "l1=-1, l2=0", pts, 1.3, {-1.0, 0.0, 1.4});  // the first in order
    report(family, "x nan", pn, 1.3, l3);
    report(family, "x nan, sigma=0, l1=0", pn, 0.0, {0.0, 1.1, 1.4});  // the first check in order
    report(family, "sigma=0, l1=0", pts, 0.0, {0.0, 1.1, 1.4});
    report(family, "count", pts, 1.3, l2);
    report(family, "count, l2=0", pts, 1.3, {0.9, 0.0});  // the values before the count
    report(family, "count 65", pts, 1.3, l65);            // the match before the cap
    report(family, "65", wide, 1.3, l65);
    report(family, "points size", bad, 1.3, l3);
    report(family, "points size, count", bad, 1.3, l2);  // the count before the point sizes
  }
  std::printf("stack %zu %zu\n", stan::math::ChainableStack::instance_->var_stack_.size(),
              stan::math::ChainableStack::instance_->dev_adj_stack_.size());
  return 0;
}

int run_time() {
  std::string family;
  int ard, steps, D, N;
  if (!(std::cin >> family >> ard >> steps >> D >> N) || D < 1 || N < 0) return 2;
  double sigma, noise;
  std::vector<double> l, y;
  points x;
  if (!read_problem(D, N, sigma, l, noise, x, y)) return 2;
  std::vector<double> th = {sigma};
  if (ard)
    th.insert(th.end(), l.begin(), l.end());
  else
    th.push_back(l[0]);
  th.push_back(noise);
  const std::string kinds = ard ? "vv" : "sc";
  for (int rep = 0; rep < 3 + steps; ++rep) {
    double fx;
    std::vector<double> g;
    const auto t0 = std::chrono::steady_clock::now();
    stan::math::gradient(gp_functor{family, kinds, x, y, false, sigma, l}, th, fx, g);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rep >= 3) {
      std::printf("step %d %.3f ms fx %.17g grad", rep - 3, ms, fx);
      for (double v : g) std::printf(" %.17g", v);
      std::printf("\n");
    }
  }
  return 0;
}

int main() {
  std::string mode;
  if (!(std::cin >> mode)) return 2;
  if (mode == "errors") return run_errors();
  if (mode == "time") return run_time();
  if (mode == "grad") return run_grad();
  return 2;
}
