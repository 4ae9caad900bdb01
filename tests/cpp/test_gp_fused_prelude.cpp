// The GP prelude generated into the factor's buffer (deferred values of
// gp_*_cov and add_diag, rev/fun/gp_exp_quad_cov.hpp, cholesky_decompose.hpp):
// every scenario runs twice in this process, with deferral switched off
// (stan::math::amd::set_deferred_values(false): every constructor launches
// its forward kernels) and on, and prints what it observed for
// tests/test_gp_fused_prelude.py to compare bit for bit.
//
// stdin:  <scenario> <family> <N> <evals> sigma l noise x(N) y(N)
// stdout: one line "<mode> <tag> v..." per observation (mode eager | deferred,
// values %.17g; messages as "<mode> <tag>|<type>|<text>"), then "stack a b".
//
// Scenarios (K = cov(x, sigma, l), Kd = add_diag(K, noise^2), L =
// cholesky_decompose(Kd), lp = multi_normal_cholesky_lpdf(y | 0, L)):
//   grad      stan::math::gradient of lp, <evals> times: fx and the gradient
//   values    the tape by hand: fx, gradient, K.adj(), Kd.adj(), then K.val(),
//             Kd.val(), L.val(); the materialisation count before the reads
//   twice     values' fx / gradient / K / Kd over two evaluations (recover_memory between)
//   before    K.val() read before add_diag
//   between   K.val() read between add_diag and cholesky_decompose
//   shared    K under two add_diag -> cholesky_decompose chains
//   multiply  + 1e-3 sum(multiply(K, y)): K's dense reverse
//   vecdiag   add_diag with a vector diagonal
//   nested    the tape inside start_nested()
//   winv      cholesky_decompose_with_inverse
//   eigen     the Eigen-typed functor under gradient()
//   count     the materialisation count over one gradient(), then over a tape whose K is read
//   notpd     add_diag(K, -2 sigma^2): the not-positive-definite message
//   nanx      a dev_data x holding a NaN: the not-symmetric message
#include <stan/math.hpp>
#include <cmath>
#include <cstdio>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

using namespace stan::math;

struct input {
  std::string scenario, family;
  int N = 0, evals = 1;
  double sigma = 0, l = 0, noise = 0;
  std::vector<double> x, y;
};

static const char* g_mode = "eager";

static void row(const char* tag, const std::vector<double>& v) {
  std::printf("%s %s", g_mode, tag);
  for (double e : v) std::printf(" %.17g", e);
  std::printf("\n");
}
static void row(const char* tag, double v) { row(tag, std::vector<double>{v}); }

template <typename X, typename S, typename L>
static dev_var_matrix cov(const std::string& family, const X& x, const S& sigma, const L& l) {
  if (family == "exp_quad") return gp_exp_quad_cov(x, sigma, l);
  if (family == "exponential") return gp_exponential_cov(x, sigma, l);
  if (family == "matern32") return gp_matern32_cov(x, sigma, l);
  if (family == "matern52") return gp_matern52_cov(x, sigma, l);
  throw std::runtime_error("unknown family " + family);
}

struct gp_functor {  // the benchmark's composition
  const input& in;
  const dev_data<double>& x;
  const dev_data<double>& y;
  const dev_data<double>& mu;
  template <typename T>
  T operator()(const std::vector<T>& th) const {
    auto K = cov(in.family, x, th[0], th[1]);
    auto Kd = add_diag(K, square(th[2]));
    auto L = cholesky_decompose(Kd);
    return multi_normal_cholesky_lpdf(y, mu, L);
  }
};

struct gp_eigen_functor {
  const input& in;
  const Eigen::VectorXd& y;
  template <typename T>
  T operator()(const Eigen::Matrix<T, -1, 1>& th) const {
    Eigen::Matrix<T, -1, -1> K = gp_exp_quad_cov(in.x, th(0), th(1));
    Eigen::Matrix<T, -1, -1> Kd = add_diag(K, square(th(2)));
    Eigen::Matrix<T, -1, -1> L = cholesky_decompose(Kd);
    Eigen::VectorXd mu = Eigen::VectorXd::Zero(in.N);
    return multi_normal_cholesky_lpdf(y, mu, L);
  }
};

static void run_gradient(const input& in) {
  const dev_data<double> x = to_dev_data(in.x), y = to_dev_data(in.y), mu = to_dev_data(std::vector<double>(in.N, 0.0));
  std::vector<double> th = {in.sigma, in.l, in.noise};
  for (int e = 0; e < in.evals; ++e) {
    double fx;
    std::vector<double> g;
    gradient(gp_functor{in, x, y, mu}, th, fx, g);
    row("fx", fx);
    row("grad", g);
  }
}

// one hand-built tape of the scenario; the caller recovers the memory
static void tape(const input& in, const std::string& sc) {
  const int n = in.N;
  var sigma(in.sigma), l(in.l), s(in.noise);
  const bool nested = sc == "nested";
  if (nested) start_nested();
  const dev_data<double> x = to_dev_data(in.x), y = to_dev_data(in.y), mu = to_dev_data(std::vector<double>(n, 0.0));
  auto K = cov(in.family, x, sigma, l);
  if (sc == "before") row("K_early", K.val());
  dev_var_matrix Kd;
  if (sc == "vecdiag") {
    std::vector<double> dv(n);
    for (int i = 0; i < n; ++i) dv[i] = in.noise * in.noise + 1e-3 * i;
    Kd = add_diag(K, to_dev_data(dv));
  } else {
    Kd = add_diag(K, square(s));
  }
  if (sc == "between") row("K_early", K.val());
  auto L = sc == "winv" ? internal::cholesky_decompose_with_inverse(Kd) : cholesky_decompose(Kd);
  var lp = multi_normal_cholesky_lpdf(y, mu, L);
  dev_var_matrix Kd2;
  if (sc == "shared") {
    Kd2 = add_diag(K, 2.0 * square(s));
    lp += multi_normal_cholesky_lpdf(y, mu, cholesky_decompose(Kd2));
  }
  if (sc == "multiply") lp += 1e-3 * sum(multiply(K, to_dev_data(in.y.data(), size_t(n), n, 1)));
  row("formed_before_reads", double(amd::materialisation_count()));
  lp.grad();
  row("fx", lp.val());
  row("grad", {sigma.adj(), l.adj(), s.adj()});
  if (sc != "twice" && sc != "count") {
    row("Kadj", K.adj());
    row("Kdadj", Kd.adj());
  }
  row("K", K.val());
  if (sc != "count") {
    row("Kd", Kd.val());
    if (sc == "shared") row("Kd2", Kd2.val());
    if (sc != "twice") row("L", L.val());
  }
  row("formed", double(amd::materialisation_count()));
  if (nested) recover_memory_nested();
}

template <typename F>
static void message(const char* tag, F&& f) {
  try {
    f();
    std::printf("%s %s|none|\n", g_mode, tag);
  } catch (const std::domain_error& e) {
    std::printf("%s %s|domain_error|%s\n", g_mode, tag, e.what());
  } catch (const std::invalid_argument& e) {
    std::printf("%s %s|invalid_argument|%s\n", g_mode, tag, e.what());
  } catch (const std::exception& e) {
    std::printf("%s %s|exception|%s\n", g_mode, tag, e.what());
  }
  recover_memory();
}

static void run(const input& in) {
  const std::string& sc = in.scenario;
  amd::materialisation_count() = 0;
  // (the closed-form prediction per tape position starts afresh in each mode)
  internal::cholesky_dev_vari::history().clear();
  if (sc == "grad") {
    run_gradient(in);
  } else if (sc == "eigen") {
    Eigen::VectorXd y(in.N), th(3);
    for (int i = 0; i < in.N; ++i) y(i) = in.y[i];
    th << in.sigma, in.l, in.noise;
    double fx;
    Eigen::VectorXd g;
    gradient(gp_eigen_functor{in, y}, th, fx, g);
    row("fx", fx);
    row("grad", {g(0), g(1), g(2)});
  } else if (sc == "count") {
    input one = in;
    one.evals = 1;
    run_gradient(one);
    row("formed_by_gradient", double(amd::materialisation_count()));
    tape(in, sc);  // reads K once
    recover_memory();
  } else if (sc == "notpd") {
    message("notpd", [&] {
      var sigma(in.sigma), l(in.l);
      auto K = cov(in.family, to_dev_data(in.x), sigma, l);
      cholesky_decompose(add_diag(K, -2.0 * in.sigma * in.sigma));
    });
  } else if (sc == "nanx") {
    message("nanx", [&] {
      std::vector<double> x = in.x;
      x[x.size() / 2] = std::numeric_limits<double>::quiet_NaN();
      var sigma(in.sigma), l(in.l), s(in.noise);
      auto K = cov(in.family, to_dev_data(x), sigma, l);  // (device-resident x: its entries are the caller's)
      cholesky_decompose(add_diag(K, square(s)));
    });
  } else {
    const int reps = sc == "twice" ? 2 : 1;
    for (int r = 0; r < reps; ++r) {
      tape(in, sc);
      recover_memory();
    }
  }
}

int main() {
  input in;
  if (!(std::cin >> in.scenario >> in.family >> in.N >> in.evals >> in.sigma >> in.l >> in.noise) || in.N < 1) return 2;
  in.x.resize(in.N);
  in.y.resize(in.N);
  for (auto& v : in.x)
    if (!(std::cin >> v)) return 2;
  for (auto& v : in.y)
    if (!(std::cin >> v)) return 2;
  for (int deferred = 0; deferred < 2; ++deferred) {
    g_mode = deferred ? "deferred" : "eager";
    amd::set_deferred_values(deferred != 0);
    run(in);
  }
  std::printf("stack %zu %zu\n", ChainableStack::instance_->var_stack_.size(),
              ChainableStack::instance_->dev_adj_stack_.size());
  return 0;
}
