// The six GLM log-densities (rev/fun/*_glm_lp[md]f.hpp over rev/fun/glm_common.hpp):
// the whole what() string of the checks their headers share, and one value and
// gradient per likelihood with every operand a var; compared in
// tests/test_glm_messages.py.
//
// stdin, mode "errors": one line "<case>|<exception type>|<message>" per check
// (4 rows, 2 columns).
// mode "values":
//   values R M C x(R M, column-major) beta(M) alpha sigma phi y01(R) yreal(R)
//          ycount(R) yclass(R) alphaC(C) betaC(M C, column-major) cuts(C - 1)
// prints "<likelihood> fx grad..." lines in %a, the gradient over the var
// operands in the order of the signature.
#include <stan/math.hpp>

#include <cstdio>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

using namespace stan::math;

static std::vector<double> read_vec(size_t n) {
  std::vector<double> v(n);
  for (auto& e : v) std::cin >> e;
  return v;
}

static std::vector<int> to_int(const std::vector<double>& v) { return std::vector<int>(v.begin(), v.end()); }

template <typename F>
static void expect(const std::string& name, const F& f) {
  start_nested();
  try {
    const double v = f();
    std::printf("%s|value|%.17g\n", name.c_str(), v);
  } catch (const std::domain_error& e) {
    std::printf("%s|domain_error|%s\n", name.c_str(), e.what());
  } catch (const std::invalid_argument& e) {
    std::printf("%s|invalid_argument|%s\n", name.c_str(), e.what());
  } catch (const std::exception& e) {
    std::printf("%s|other|%s\n", name.c_str(), e.what());
  }
  recover_memory_nested();
}

// kind 0 bernoulli_logit, 1 normal_id, 2 poisson_log: the scalar-intercept
// form on device data, beta (and sigma) vars
template <int K>
static double dev_call(const std::vector<double>& y, int R, const std::vector<double>& x, int xr, double alpha,
                       const std::vector<double>& beta, double sigma) {
  const dev_data<double> xd = to_dev_data(x.data(), x.size(), xr, 2);
  const std::vector<var> b(beta.begin(), beta.end());
  if constexpr (K == 1) {
    const dev_data<double> yd = to_dev_data(std::vector<double>(y.begin(), y.begin() + R));
    return normal_id_glm_lpdf(yd, xd, alpha, b, var(sigma)).val();
  } else {
    const std::vector<int> yi = to_int(y);
    const dev_data<int> yd = to_dev_data(std::vector<int>(yi.begin(), yi.begin() + R));
    if constexpr (K == 0) return bernoulli_logit_glm_lpmf(yd, xd, alpha, b).val();
    else return poisson_log_glm_lpmf(yd, xd, alpha, b).val();
  }
}

template <int K>
static double host_call(const std::vector<double>& y, const std::vector<double>& x, double alpha,
                        const std::vector<double>& beta) {
  const std::vector<var> b(beta.begin(), beta.end());
  if constexpr (K == 1) return normal_id_glm_lpdf(y, x, 2, alpha, b, 1.5).val();
  else if constexpr (K == 0) return bernoulli_logit_glm_lpmf(to_int(y), x, 2, alpha, b).val();
  else return poisson_log_glm_lpmf(to_int(y), x, 2, alpha, b).val();
}

template <int K>
static void errors_of(const std::string& k) {
  const double inf = std::numeric_limits<double>::infinity();
  const std::vector<double> y = {0, 1, 1, 0};  // (valid for each of the three)
  const std::vector<double> x = {0.5, -0.25, 1.0, 0.75, -1.0, 0.5, 0.25, 0.125};  // 4 x 2
  const std::vector<double> beta = {0.3, -0.2};
  expect(k + "_ok", [&] { return dev_call<K>(y, 4, x, 4, 0.1, beta, 1.5); });
  expect(k + "_y_size", [&] { return dev_call<K>(y, 3, x, 4, 0.1, beta, 1.5); });
  expect(k + "_beta_size", [&] { return dev_call<K>(y, 4, x, 4, 0.1, {0.3, -0.2, 0.1}, 1.5); });
  expect(k + "_alpha_inf", [&] { return dev_call<K>(y, 4, x, 4, inf, beta, 1.5); });
  expect(k + "_x_inf", [&] {
    std::vector<double> xi = x;
    xi[0] = inf;  // row 1: theta = +inf, y = 0
    return dev_call<K>(y, 4, xi, 4, 0.1, beta, 1.5);
  });
  expect(k + "_host_x_size", [&] { return host_call<K>(y, {0.5, -0.25, 1.0, 0.75, -1.0, 0.5, 0.25}, 0.1, beta); });
}

static void cmd_errors() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  errors_of<0>("bernoulli");
  errors_of<2>("poisson");
  errors_of<1>("normal");
  const std::vector<double> y = {0, 1, 1, 0};
  const std::vector<double> x = {0.5, -0.25, 1.0, 0.75, -1.0, 0.5, 0.25, 0.125};
  const std::vector<double> beta = {0.3, -0.2};
  expect("normal_sigma_inf", [&] { return dev_call<1>(y, 4, x, 4, 0.1, beta, inf); });
  expect("normal_sigma_nan", [&] { return dev_call<1>(y, 4, x, 4, 0.1, beta, nan); });
  expect("normal_sigma_before_y_size", [&] { return dev_call<1>(y, 3, x, 4, 0.1, beta, inf); });
  // the other two host-vector forms, and ordered's cascade: no "Intercept" line
  const std::vector<double> x7(x.begin(), x.begin() + 7);
  expect("neg_binomial_host_x_size", [&] {
    const std::vector<var> b(beta.begin(), beta.end());
    return neg_binomial_2_log_glm_lpmf(std::vector<int>{0, 1, 1, 0}, x7, 2, 0.1, b, 2.5).val();
  });
  expect("ordered_host_x_size", [&] {
    const std::vector<var> b(beta.begin(), beta.end());
    return ordered_logistic_glm_lpmf(std::vector<int>{1, 3, 2, 2}, x7, 2, b, std::vector<double>{-0.5, 0.7}).val();
  });
  expect("ordered_x_inf", [&] {
    std::vector<double> xi = x;
    xi[0] = inf;
    const std::vector<var> b(beta.begin(), beta.end());
    return ordered_logistic_glm_lpmf(std::vector<int>{1, 3, 2, 2}, xi, 2, b, std::vector<double>{-0.5, 0.7}).val();
  });
  std::printf("stack|%zu|%zu\n", ChainableStack::instance_->var_stack_.size(),
              ChainableStack::instance_->dev_adj_stack_.size());
}

static void print_a(const char* tag, double fx, const std::vector<double>& g) {
  std::printf("%s %a", tag, fx);
  for (double e : g) std::printf(" %a", e);
  std::printf("\n");
}

static void cmd_values() {
  int R, M, C;
  std::cin >> R >> M >> C;
  const auto xv = read_vec(size_t(R) * M);
  const auto beta = read_vec(size_t(M));
  const auto scal = read_vec(3);  // alpha, sigma, phi
  const std::vector<int> y01 = to_int(read_vec(size_t(R)));
  const auto yreal = read_vec(size_t(R));
  const std::vector<int> ycount = to_int(read_vec(size_t(R)));
  const std::vector<int> yclass = to_int(read_vec(size_t(R)));
  const auto alphaC = read_vec(size_t(C));
  const auto betaC = read_vec(size_t(M) * C);
  const auto cuts = read_vec(size_t(C - 1));
  const dev_data<double> xd = to_dev_data(xv.data(), xv.size(), R, M);
  const dev_data<int> y01d = to_dev_data(y01), ycountd = to_dev_data(ycount), yclassd = to_dev_data(yclass);
  const dev_data<double> yreald = to_dev_data(yreal);
  double fx;
  std::vector<double> g;
  auto bvec = [&](const std::vector<var>& t) { return std::vector<var>(t.begin() + 1, t.begin() + 1 + M); };

  std::vector<double> th = {scal[0]};
  th.insert(th.end(), beta.begin(), beta.end());
  gradient([&](const std::vector<var>& t) { return bernoulli_logit_glm_lpmf(y01d, xd, t[0], bvec(t)); }, th, fx, g);
  print_a("bernoulli_logit", fx, g);
  gradient([&](const std::vector<var>& t) { return poisson_log_glm_lpmf(ycountd, xd, t[0], bvec(t)); }, th, fx, g);
  print_a("poisson_log", fx, g);
  th.push_back(scal[1]);
  gradient([&](const std::vector<var>& t) { return normal_id_glm_lpdf(yreald, xd, t[0], bvec(t), t[size_t(M) + 1]); },
           th, fx, g);
  print_a("normal_id", fx, g);
  th.back() = scal[2];
  gradient(
      [&](const std::vector<var>& t) {
        return neg_binomial_2_log_glm_lpmf(ycountd, xd, t[0], bvec(t), t[size_t(M) + 1]);
      },
      th, fx, g);
  print_a("neg_binomial_2_log", fx, g);

  th = alphaC;
  th.insert(th.end(), betaC.begin(), betaC.end());
  gradient(
      [&](const std::vector<var>& t) {
        const dev_var_matrix a = to_dev(std::vector<var>(t.begin(), t.begin() + C), C, 1);
        const dev_var_matrix b = to_dev(std::vector<var>(t.begin() + C, t.end()), M, C);
        return categorical_logit_glm_lpmf(yclassd, xd, a, b);
      },
      th, fx, g);
  print_a("categorical_logit", fx, g);

  th = beta;
  th.insert(th.end(), cuts.begin(), cuts.end());
  gradient(
      [&](const std::vector<var>& t) {
        return ordered_logistic_glm_lpmf(yclassd, xd, std::vector<var>(t.begin(), t.begin() + M),
                                         std::vector<var>(t.begin() + M, t.end()));
      },
      th, fx, g);
  print_a("ordered_logistic", fx, g);
  std::printf("stack %zu %zu\n", ChainableStack::instance_->var_stack_.size(),
              ChainableStack::instance_->dev_adj_stack_.size());
}

int main() {
  std::string mode;
  std::cin >> mode;
  try {
    if (mode == "errors") cmd_errors();
    else if (mode == "values") cmd_values();
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
