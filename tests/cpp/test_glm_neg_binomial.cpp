// neg_binomial_2_log_glm_lpmf (rev/fun/neg_binomial_2_log_glm_lpmf.hpp,
// eigen/interop.hpp) through stan::math::gradient on the device; the values
// are compared in tests/test_glm_neg_binomial.py.
//
// stdin, mode "tape":
//   tape R M y(R) x(R M, column-major) alpha beta(M) phi
// prints "<tag> values..." lines:
//   fx_<k> / grad_<k> and fxp_<k> / gradp_<k> (propto) for the seven kinds k
//   of (alpha, beta, phi), 'v' var / 'd' double (the gradient holds the var
//   arguments in that order); fx_ddd / fxp_ddd: the all-double form, a double;
//   fx_shards7 / grad_shards7: seven row shards summed on one tape;
//   fx_dist / grad_dist: one shard with distributed = true under a one-rank
//   host collective; fx_eigen / grad_eigen: the Eigen signature;
//   fx_host / grad_host: host vectors; fx_leaf / grad_leaf: beta as the
//   device leaf of gradient(); grad_fd: central differences of fx_ddd's form
//   (h = 1e-5 max(1, |theta_i|)); stack: the stack sizes afterwards.
// mode "errors": one line "<case>|<exception type>|<message>" per check.
#include <stan/math.hpp>

#include <cmath>
#include <cstdio>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

using namespace stan::math;

static std::vector<double> read_vec(size_t n) {
  std::vector<double> v(n);
  for (auto& e : v) std::cin >> e;
  return v;
}

static void print(const std::string& tag, const std::vector<double>& v) {
  std::printf("%s", tag.c_str());
  for (double e : v) std::printf(" %.17g", e);
  std::printf("\n");
}

static void print1(const std::string& tag, double v) { std::printf("%s %.17g\n", tag.c_str(), v); }

static void one_rank_allgather(const double* send, long long count, double* recv, void*) {
  for (long long i = 0; i < count; ++i) recv[i] = send[i];
}

// f(alpha, beta, phi) with each argument theta's next var(s) or the data value, by `kinds`
template <typename F>
static var with_kinds(const std::string& kinds, const std::vector<var>& t, double alpha,
                      const std::vector<double>& beta, double phi, const F& f) {
  const int M = int(beta.size());
  size_t at = 0;
  auto next_alpha = [&] { return t[at++]; };
  auto next_beta = [&] {
    std::vector<var> b(t.begin() + at, t.begin() + at + M);
    at += size_t(M);
    return b;
  };
  if (kinds == "vvv") {
    var a = next_alpha();
    auto b = next_beta();
    return f(a, b, t[at]);
  }
  if (kinds == "vvd") {
    var a = next_alpha();
    return f(a, next_beta(), phi);
  }
  if (kinds == "vdv") {
    var a = next_alpha();
    return f(a, beta, t[at]);
  }
  if (kinds == "dvv") {
    auto b = next_beta();
    return f(alpha, b, t[at]);
  }
  if (kinds == "vdd") return f(next_alpha(), beta, phi);
  if (kinds == "dvd") return f(alpha, next_beta(), phi);
  if (kinds == "ddv") return f(alpha, beta, t[0]);
  throw std::runtime_error("unknown kinds " + kinds);
}

static std::vector<double> theta_of(const std::string& kinds, double alpha, const std::vector<double>& beta,
                                    double phi) {
  std::vector<double> th;
  if (kinds[0] == 'v') th.push_back(alpha);
  if (kinds[1] == 'v') th.insert(th.end(), beta.begin(), beta.end());
  if (kinds[2] == 'v') th.push_back(phi);
  return th;
}

static void cmd_tape() {
  int R, M;
  std::cin >> R >> M;
  const auto yv = read_vec(size_t(R));
  const auto xv = read_vec(size_t(R) * M);
  const auto th = read_vec(size_t(M) + 2);
  const double alpha = th[0], phi = th[size_t(M) + 1];
  const std::vector<double> beta(th.begin() + 1, th.begin() + 1 + M);
  std::vector<int> y(yv.begin(), yv.end());
  const dev_data<int> yd = to_dev_data(y);
  const dev_data<double> xd = to_dev_data(xv.data(), xv.size(), R, M);
  double fx;
  std::vector<double> g;

  for (const char* k : {"vvv", "vvd", "vdv", "dvv", "vdd", "dvd", "ddv"}) {
    const std::string kinds(k);
    const auto t0 = theta_of(kinds, alpha, beta, phi);
    gradient(
        [&](const std::vector<var>& t) {
          return with_kinds(kinds, t, alpha, beta, phi, [&](const auto& a, const auto& b, const auto& p) {
            return var(neg_binomial_2_log_glm_lpmf(yd, xd, a, b, p));
          });
        },
        t0, fx, g);
    print1("fx_" + kinds, fx);
    print("grad_" + kinds, g);
    gradient(
        [&](const std::vector<var>& t) {
          return with_kinds(kinds, t, alpha, beta, phi, [&](const auto& a, const auto& b, const auto& p) {
            return var(neg_binomial_2_log_glm_lpmf<true>(yd, xd, a, b, p));
          });
        },
        t0, fx, g);
    print1("fxp_" + kinds, fx);
    print("gradp_" + kinds, g);
  }

  // all-double arguments: a plain double, no tape
  static_assert(std::is_same<decltype(neg_binomial_2_log_glm_lpmf(yd, xd, alpha, beta, phi)), double>::value,
                "the all-double form returns double");
  static_assert(std::is_same<decltype(neg_binomial_2_log_glm_lpmf(yd, xd, var(), beta, phi)), var>::value, "var");
  start_nested();
  print1("fx_ddd", neg_binomial_2_log_glm_lpmf(yd, xd, alpha, beta, phi));
  print1("fxp_ddd", neg_binomial_2_log_glm_lpmf<true>(yd, xd, alpha, beta, phi));
  recover_memory_nested();

  // seven contiguous row shards summed on the tape (each shard: its own N)
  gradient(
      [&](const std::vector<var>& t) {
        std::vector<var> b(t.begin() + 1, t.begin() + 1 + M);
        var s = 0.0;
        for (int k = 0; k < 7; ++k) {
          long long b0, b1;
          row_partition(R, 7, k, &b0, &b1);
          glm_shard sh;
          sh.y = yd.data() + b0;
          sh.x = xd.data() + b0;
          sh.rows = b1 - b0;
          sh.M = M;
          sh.ldx = R;
          sh.row0 = b0;
          sh.total_rows = b1 - b0;
          s += neg_binomial_2_log_glm_lpmf(sh, t[0], b, t[size_t(M) + 1]);
        }
        return s;
      },
      th, fx, g);
  print1("fx_shards7", fx);
  print("grad_shards7", g);

  // one shard, distributed, under a one-rank host collective
  amd::set_host_collective(1, 0, one_rank_allgather, nullptr);
  gradient(
      [&](const std::vector<var>& t) {
        std::vector<var> b(t.begin() + 1, t.begin() + 1 + M);
        glm_shard sh;
        sh.y = yd.data();
        sh.x = xd.data();
        sh.rows = R;
        sh.M = M;
        sh.ldx = R;
        sh.total_rows = R;
        sh.distributed = true;
        return neg_binomial_2_log_glm_lpmf<false>(sh, t[0], b, t[size_t(M) + 1]);
      },
      th, fx, g);
  amd::set_host_collective(1, 0, nullptr, nullptr);
  print1("fx_dist", fx);
  print("grad_dist", g);

  // the Eigen signature
  const matrix_d xe = Eigen::Map<const matrix_d>(xv.data(), R, M);
  gradient(
      [&](const std::vector<var>& t) {
        Eigen::Matrix<var, Eigen::Dynamic, 1> b(M);
        for (int j = 0; j < M; ++j) b(j) = t[size_t(1 + j)];
        return neg_binomial_2_log_glm_lpmf(y, xe, t[0], b, t[size_t(M) + 1]);
      },
      th, fx, g);
  print1("fx_eigen", fx);
  print("grad_eigen", g);
  {
    Eigen::Matrix<double, Eigen::Dynamic, 1> bd(M);
    for (int j = 0; j < M; ++j) bd(j) = beta[size_t(j)];
    static_assert(std::is_same<decltype(neg_binomial_2_log_glm_lpmf(y, xe, alpha, bd, phi)), double>::value,
                  "the all-double Eigen form returns double");
    start_nested();
    print1("fx_eigen_ddd", neg_binomial_2_log_glm_lpmf(y, xe, alpha, bd, phi));
    recover_memory_nested();
  }

  // host vectors (uploaded per call)
  gradient(
      [&](const std::vector<var>& t) {
        std::vector<var> b(t.begin() + 1, t.begin() + 1 + M);
        return neg_binomial_2_log_glm_lpmf<false>(y, xv, M, t[0], b, t[size_t(M) + 1]);
      },
      th, fx, g);
  print1("fx_host", fx);
  print("grad_host", g);

  // beta as the device leaf of gradient(): the gradient stays on the device
  {
    const dev_data<double> bdev = to_dev_data(beta.data(), beta.size(), M, 1);
    double* gdev = amd::alloc_doubles(size_t(M > 0 ? M : 1));
    gradient([&](const dev_var_matrix& b) { return neg_binomial_2_log_glm_lpmf(yd, xd, alpha, b, phi); }, bdev, fx,
             gdev);
    std::vector<double> gh(static_cast<size_t>(M));
    amd::to_host(gh.data(), gdev, gh.size());
    print1("fx_leaf", fx);
    print("grad_leaf", gh);
  }

  // central differences of the all-double form
  {
    std::vector<double> fd(th.size());
    auto eval = [&](const std::vector<double>& t) {
      const std::vector<double> b(t.begin() + 1, t.begin() + 1 + M);
      start_nested();
      const double v = neg_binomial_2_log_glm_lpmf(yd, xd, t[0], b, t[size_t(M) + 1]);
      recover_memory_nested();
      return v;
    };
    for (size_t i = 0; i < th.size(); ++i) {
      const double h = 1e-5 * std::fmax(1.0, std::fabs(th[i]));
      std::vector<double> tp = th, tm = th;
      tp[i] += h;
      tm[i] -= h;
      fd[i] = (eval(tp) - eval(tm)) / (tp[i] - tm[i]);
    }
    print("grad_fd", fd);
  }
  std::printf("stack %zu %zu\n", ChainableStack::instance_->var_stack_.size(),
              ChainableStack::instance_->dev_adj_stack_.size());
}

template <typename F>
static void expect(const char* name, const F& f) {
  start_nested();
  try {
    const double v = f();
    std::printf("%s|value|%.17g\n", name, v);
  } catch (const std::domain_error& e) {
    std::printf("%s|domain_error|%s\n", name, e.what());
  } catch (const std::invalid_argument& e) {
    std::printf("%s|invalid_argument|%s\n", name, e.what());
  } catch (const std::exception& e) {
    std::printf("%s|other|%s\n", name, e.what());
  }
  recover_memory_nested();
}

static void cmd_errors() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<int> y = {1, 0, 4, 2};
  const std::vector<double> x = {0.5, -0.25, 1.0, 0.75, -1.0, 0.5, 0.25, 0.125};  // 4 x 2
  const std::vector<double> beta = {0.3, -0.2};
  auto call = [&](const std::vector<int>& yy, const std::vector<double>& bb, double phi) {
    std::vector<var> b(bb.begin(), bb.end());
    var a = 0.1, p = phi;
    return neg_binomial_2_log_glm_lpmf(yy, x, 2, a, b, p).val();
  };
  expect("ok", [&] { return call(y, beta, 2.5); });
  expect("negative_y", [&] { return call({1, 0, -2, 2}, beta, 2.5); });
  expect("negative_y_and_phi", [&] { return call({1, 0, -2, 2}, beta, -1.0); });
  expect("phi_zero", [&] { return call(y, beta, 0.0); });
  expect("phi_negative", [&] { return call(y, beta, -1.0); });
  expect("phi_inf", [&] { return call(y, beta, inf); });
  expect("phi_nan", [&] { return call(y, beta, nan); });
  expect("phi_negative_double", [&] { return neg_binomial_2_log_glm_lpmf(y, x, 2, 0.1, beta, -1.0); });
  expect("beta_size", [&] { return call(y, {0.3, -0.2, 0.1}, 2.5); });
  expect("y_size", [&] {
    const dev_data<int> yd = to_dev_data(std::vector<int>{1, 0, 4});
    const dev_data<double> xd = to_dev_data(x.data(), x.size(), 4, 2);
    std::vector<var> b(beta.begin(), beta.end());
    return neg_binomial_2_log_glm_lpmf(yd, xd, var(0.1), b, var(2.5)).val();
  });
  expect("y_size_eigen", [&] {
    const matrix_d xe = Eigen::Map<const matrix_d>(x.data(), 4, 2);
    Eigen::Matrix<var, Eigen::Dynamic, 1> b(2);
    b(0) = 0.3;
    b(1) = -0.2;
    return neg_binomial_2_log_glm_lpmf(std::vector<int>{1, 0, 4}, xe, var(0.1), b, var(2.5)).val();
  });
  expect("nonfinite_beta", [&] { return call(y, {inf, -0.2}, 2.5); });
  expect("nonfinite_alpha", [&] {
    std::vector<var> b(beta.begin(), beta.end());
    return neg_binomial_2_log_glm_lpmf(y, x, 2, var(-inf), b, var(2.5)).val();
  });
  expect("nonfinite_x", [&] {
    std::vector<double> xn = x;
    xn[5] = nan;
    std::vector<var> b(beta.begin(), beta.end());
    return neg_binomial_2_log_glm_lpmf(y, xn, 2, var(0.1), b, var(2.5)).val();
  });
  expect("empty_y", [&] {
    std::vector<var> b(beta.begin(), beta.end());
    return neg_binomial_2_log_glm_lpmf(std::vector<int>{}, std::vector<double>{}, 2, var(0.1), b, var(2.5)).val();
  });
  expect("all_data_propto", [&] { return neg_binomial_2_log_glm_lpmf<true>(y, x, 2, 0.1, beta, 2.5); });
  std::printf("stack|%zu|%zu\n", ChainableStack::instance_->var_stack_.size(),
              ChainableStack::instance_->dev_adj_stack_.size());
}

int main() {
  std::string mode;
  std::cin >> mode;
  try {
    if (mode == "tape") cmd_tape();
    else if (mode == "errors") cmd_errors();
    else {
      std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
      return 2;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
