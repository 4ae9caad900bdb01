// ordered_logistic_glm_lpmf (rev/fun/ordered_logistic_glm_lpmf.hpp,
// eigen/interop.hpp) through stan::math::gradient on the device; the values
// are compared in tests/test_glm_ordered.py.
//
// stdin, mode "tape":
//   tape R M C y(R) x(R M, column-major) beta(M) cuts(C - 1)
// prints "<tag> values..." lines:
//   fx_<k> / grad_<k> and fxp_<k> / gradp_<k> (propto) for the three kinds k
//   of (beta, cuts), 'v' var / 'd' double (the gradient holds the var
//   arguments in that order); fx_dd / fxp_dd: the all-double form, a double;
//   fx_shards7 / grad_shards7: seven row shards summed on one tape;
//   fx_dist / grad_dist: one shard with distributed = true under a one-rank
//   host collective; fx_eigen / grad_eigen: the Eigen signature;
//   fx_host / grad_host: host vectors; fx_leaf / grad_leaf: beta as the
//   device leaf of gradient(); stack: the stack sizes afterwards.
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

// f(beta, cuts) with each argument theta's next vars or the data values, by `kinds`
template <typename F>
static var with_kinds(const std::string& kinds, const std::vector<var>& t, const std::vector<double>& beta,
                      const std::vector<double>& cuts, const F& f) {
  const size_t M = beta.size(), K = cuts.size();
  if (kinds == "vv")
    return f(std::vector<var>(t.begin(), t.begin() + M), std::vector<var>(t.begin() + M, t.begin() + M + K));
  if (kinds == "vd") return f(std::vector<var>(t.begin(), t.begin() + M), cuts);
  if (kinds == "dv") return f(beta, std::vector<var>(t.begin(), t.begin() + K));
  throw std::runtime_error("unknown kinds " + kinds);
}

static std::vector<double> theta_of(const std::string& kinds, const std::vector<double>& beta,
                                    const std::vector<double>& cuts) {
  std::vector<double> th;
  if (kinds[0] == 'v') th.insert(th.end(), beta.begin(), beta.end());
  if (kinds[1] == 'v') th.insert(th.end(), cuts.begin(), cuts.end());
  return th;
}

static void cmd_tape() {
  int R, M, C;
  std::cin >> R >> M >> C;
  const int K = C - 1;
  const auto yv = read_vec(size_t(R));
  const auto xv = read_vec(size_t(R) * M);
  const auto beta = read_vec(size_t(M));
  const auto cuts = read_vec(size_t(K));
  std::vector<double> th = beta;
  th.insert(th.end(), cuts.begin(), cuts.end());
  std::vector<int> y(yv.begin(), yv.end());
  const dev_data<int> yd = to_dev_data(y);
  const dev_data<double> xd = to_dev_data(xv.data(), xv.size(), R, M);
  double fx;
  std::vector<double> g;

  for (const char* k : {"vv", "vd", "dv"}) {
    const std::string kinds(k);
    const auto t0 = theta_of(kinds, beta, cuts);
    gradient(
        [&](const std::vector<var>& t) {
          return with_kinds(kinds, t, beta, cuts, [&](const auto& b, const auto& c) {
            return var(ordered_logistic_glm_lpmf(yd, xd, b, c));
          });
        },
        t0, fx, g);
    print1("fx_" + kinds, fx);
    print("grad_" + kinds, g);
    gradient(
        [&](const std::vector<var>& t) {
          return with_kinds(kinds, t, beta, cuts, [&](const auto& b, const auto& c) {
            return var(ordered_logistic_glm_lpmf<true>(yd, xd, b, c));
          });
        },
        t0, fx, g);
    print1("fxp_" + kinds, fx);
    print("gradp_" + kinds, g);
  }

  // the return type is var iff beta or cuts holds vars
  const std::vector<var> bvar, cvar;  // (types only: no var is created outside a gradient() call)
  static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf(yd, xd, beta, cuts)), double>::value,
                "the all-double form returns double");
  static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf<true>(yd, xd, beta, cuts)), double>::value, "double");
  static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf(yd, xd, bvar, cuts)), var>::value, "var beta");
  static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf(yd, xd, beta, cvar)), var>::value, "var cuts");
  static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf(yd, xd, bvar, cvar)), var>::value, "var both");
  static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf(glm_shard(), beta, cuts)), double>::value, "shard");
  static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf(glm_shard(), beta, cvar)), var>::value, "shard var");
  static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf(y, xv, M, beta, cuts)), double>::value, "host");
  static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf(y, xv, M, bvar, cuts)), var>::value, "host var");
  start_nested();
  print1("fx_dd", ordered_logistic_glm_lpmf(yd, xd, beta, cuts));
  print1("fxp_dd", ordered_logistic_glm_lpmf<true>(yd, xd, beta, cuts));
  recover_memory_nested();

  // seven contiguous row shards summed on the tape
  gradient(
      [&](const std::vector<var>& t) {
        std::vector<var> b(t.begin(), t.begin() + M), c(t.begin() + M, t.end());
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
          s += ordered_logistic_glm_lpmf(sh, b, c);
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
        std::vector<var> b(t.begin(), t.begin() + M), c(t.begin() + M, t.end());
        glm_shard sh;
        sh.y = yd.data();
        sh.x = xd.data();
        sh.rows = R;
        sh.M = M;
        sh.ldx = R;
        sh.total_rows = R;
        sh.distributed = true;
        return ordered_logistic_glm_lpmf<false>(sh, b, c);
      },
      th, fx, g);
  amd::set_host_collective(1, 0, nullptr, nullptr);
  print1("fx_dist", fx);
  print("grad_dist", g);

  // the Eigen signature
  const matrix_d xe = Eigen::Map<const matrix_d>(xv.data(), R, M);
  gradient(
      [&](const std::vector<var>& t) {
        Eigen::Matrix<var, Eigen::Dynamic, 1> b(M), c(K);
        for (int j = 0; j < M; ++j) b(j) = t[size_t(j)];
        for (int j = 0; j < K; ++j) c(j) = t[size_t(M + j)];
        return ordered_logistic_glm_lpmf(y, xe, b, c);
      },
      th, fx, g);
  print1("fx_eigen", fx);
  print("grad_eigen", g);
  {
    Eigen::Matrix<double, Eigen::Dynamic, 1> bd(M), cd(K);
    for (int j = 0; j < M; ++j) bd(j) = beta[size_t(j)];
    for (int j = 0; j < K; ++j) cd(j) = cuts[size_t(j)];
    static_assert(std::is_same<decltype(ordered_logistic_glm_lpmf(y, xe, bd, cd)), double>::value,
                  "the all-double Eigen form returns double");
    start_nested();
    print1("fx_eigen_dd", ordered_logistic_glm_lpmf(y, xe, bd, cd));
    recover_memory_nested();
  }

  // host vectors (uploaded per call)
  gradient(
      [&](const std::vector<var>& t) {
        std::vector<var> b(t.begin(), t.begin() + M), c(t.begin() + M, t.end());
        return ordered_logistic_glm_lpmf<false>(y, xv, M, b, c);
      },
      th, fx, g);
  print1("fx_host", fx);
  print("grad_host", g);

  // beta as the device leaf of gradient(): the gradient stays on the device
  {
    const dev_data<double> bdev = to_dev_data(beta.data(), beta.size(), M, 1);
    double* gdev = amd::alloc_doubles(size_t(M > 0 ? M : 1));
    gradient([&](const dev_var_matrix& b) { return ordered_logistic_glm_lpmf(yd, xd, b, cuts); }, bdev, fx, gdev);
    std::vector<double> gh(static_cast<size_t>(M));
    amd::to_host(gh.data(), gdev, gh.size());
    print1("fx_leaf", fx);
    print("grad_leaf", gh);
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
  const std::vector<int> y = {1, 3, 2, 2};
  const std::vector<double> x = {0.5, -0.25, 1.0, 0.75, -1.0, 0.5, 0.25, 0.125};  // 4 x 2
  const std::vector<double> beta = {0.3, -0.2}, cuts = {-0.5, 0.7};
  auto call = [&](const std::vector<int>& yy, const std::vector<double>& xx, const std::vector<double>& bb,
                  const std::vector<double>& cc) {
    std::vector<var> b(bb.begin(), bb.end()), c(cc.begin(), cc.end());
    return ordered_logistic_glm_lpmf(yy, xx, 2, b, c).val();
  };
  expect("ok", [&] { return call(y, x, beta, cuts); });
  expect("y_size", [&] {
    const dev_data<int> yd = to_dev_data(std::vector<int>{1, 3, 2});
    const dev_data<double> xd = to_dev_data(x.data(), x.size(), 4, 2);
    std::vector<var> b(beta.begin(), beta.end());
    return ordered_logistic_glm_lpmf(yd, xd, b, cuts).val();
  });
  expect("y_size_eigen", [&] {
    const matrix_d xe = Eigen::Map<const matrix_d>(x.data(), 4, 2);
    Eigen::Matrix<var, Eigen::Dynamic, 1> b(2);
    Eigen::Matrix<double, Eigen::Dynamic, 1> c(2);
    b(0) = 0.3;
    b(1) = -0.2;
    c(0) = -0.5;
    c(1) = 0.7;
    return ordered_logistic_glm_lpmf(std::vector<int>{1, 3, 2}, xe, b, c).val();
  });
  expect("beta_size", [&] { return call(y, x, {0.3, -0.2, 0.1}, cuts); });
  expect("beta_size_and_y", [&] { return call({1, 3, 4, 2}, x, {0.3, -0.2, 0.1}, cuts); });  // beta's size first
  expect("y_high", [&] { return call({1, 3, 4, 2}, x, beta, cuts); });
  expect("y_zero", [&] { return call({1, 0, 4, 2}, x, beta, cuts); });  // the first offending row
  expect("y_high_double", [&] { return ordered_logistic_glm_lpmf(std::vector<int>{1, 3, 4, 2}, x, 2, beta, cuts); });
  expect("y_high_propto_double",
         [&] { return ordered_logistic_glm_lpmf<true>(std::vector<int>{1, 3, 4, 2}, x, 2, beta, cuts); });
  expect("y_shard_row0", [&] {
    const dev_data<int> yd = to_dev_data(std::vector<int>{1, 3, 4, 2});
    const dev_data<double> xd = to_dev_data(x.data(), x.size(), 4, 2);
    glm_shard sh;
    sh.y = yd.data();
    sh.x = xd.data();
    sh.rows = 4;
    sh.M = 2;
    sh.ldx = 4;
    sh.row0 = 10;
    sh.total_rows = 4;
    std::vector<var> b(beta.begin(), beta.end());
    return ordered_logistic_glm_lpmf(sh, b, cuts).val();
  });
  expect("y_and_cuts", [&] { return call({1, 3, 4, 2}, x, beta, {0.7, -0.5}); });  // y before the cut-points
  expect("cuts_unordered", [&] { return call(y, x, beta, {0.7, -0.5}); });
  expect("cuts_equal", [&] { return call(y, x, beta, {0.5, 0.5}); });
  expect("cuts_nan", [&] { return call(y, x, beta, {-0.5, nan}); });
  expect("cuts_unordered_and_inf", [&] { return call(y, x, beta, {inf, 0.5}); });  // the order before finiteness
  expect("cut_last_inf", [&] { return call(y, x, beta, {-0.5, inf}); });
  expect("cut_first_inf", [&] { return call(y, x, beta, {-inf, 0.7}); });
  expect("cuts_unordered_double", [&] { return ordered_logistic_glm_lpmf(y, x, 2, beta, std::vector<double>{0.7, -0.5}); });
  expect("nonfinite_beta", [&] { return call(y, x, {inf, -0.2}, cuts); });
  expect("nonfinite_x", [&] {
    std::vector<double> xn = x;
    xn[5] = nan;
    return call(y, xn, beta, cuts);
  });
  expect("infinite_x", [&] {
    std::vector<double> xn = x;
    xn[0] = -inf;  // row 1, class 1: logp itself stays finite there
    return call(y, xn, beta, cuts);
  });
  expect("empty_y", [&] { return call({}, {}, beta, cuts); });
  expect("all_data_propto", [&] { return ordered_logistic_glm_lpmf<true>(y, x, 2, beta, cuts); });
  expect("one_class", [&] { return call({1, 1, 1, 1}, x, beta, {}); });
  expect("one_class_grad", [&] {  // C = 1: the gradient over beta is zero
    double fx;
    std::vector<double> g;
    gradient(
        [&](const std::vector<var>& t) {
          return var(ordered_logistic_glm_lpmf(std::vector<int>{1, 1, 1, 1}, x, 2, t, std::vector<double>{}));
        },
        beta, fx, g);
    return std::fabs(fx) + std::fabs(g[0]) + std::fabs(g[1]);
  });
  expect("one_class_y2", [&] { return call({1, 2, 1, 1}, x, beta, {}); });
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
