// The four row-wise GLMs with one intercept per row (rev/fun/*_glm_lp[md]f.hpp,
// eigen/interop.hpp) through stan::math::gradient on the device; the values
// are compared in tests/test_glm_vec_intercept.py.  Kinds: 0 bernoulli_logit,
// 1 normal_id, 2 poisson_log, 3 neg_binomial_2_log.
//
// stdin, mode "tape":
//   tape R M x(R M, column-major) beta(M) alpha(R) sigma phi y0(R) y1(R) y2(R) y3(R)
//   gp N x(N) sigma l eta(N) ycount(N) y01(N)            (the latent GP, below)
// prints "<tag> values..." lines, k the kind:
//   fx_<k>_<a>_<b> / grad_<k>_<a>_<b> and fxp_ / gradp_ (propto): alpha as
//   hv (std::vector<var>), dv (dev_var_matrix from to_dev of host vars), hd
//   (std::vector<double>), dd (dev_data<double>); b = v: beta and sigma / phi
//   vars, b = d: both data.  The gradient holds [alpha(R)][beta(M)][sigma | phi]
//   for the var arguments.  hd / dd with b = d are plain doubles (no gradient).
//   grad_two: one device alpha used by a poisson and a neg_binomial call on one
//   tape (the gradient over alpha's host vars).
//   fx_<k>_shards7 / grad_: seven row shards, each with its slice of alpha;
//   fx_<k>_dist: one distributed shard under a one-rank host collective;
//   fx_<k>_eigen (column vector of var), fx_<k>_eigenrow (row vector of
//   double), fx_<k>_host (host vectors).
//   fx_gp_<p|b>_<dev|host> / grad_: the latent GP with f on the device / brought
//   to the host; stack: the stack sizes afterwards.
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

struct data {
  int R, M;
  std::vector<double> x, beta, alpha, y1;
  double extra[4];  // sigma at 1, phi at 3
  std::vector<int> y[4];
  dev_data<double> xd, y1d, alpha_dd;
  dev_data<int> yd[4];
};

template <int K, bool propto, typename A, typename B, typename E>
static auto glm(const data& d, const A& a, const B& b, const E& e) {
  if constexpr (K == 0) return bernoulli_logit_glm_lpmf<propto>(d.yd[0], d.xd, a, b);
  else if constexpr (K == 1) return normal_id_glm_lpdf<propto>(d.y1d, d.xd, a, b, e);
  else if constexpr (K == 2) return poisson_log_glm_lpmf<propto>(d.yd[2], d.xd, a, b);
  else return neg_binomial_2_log_glm_lpmf<propto>(d.yd[3], d.xd, a, b, e);
}

template <int K, typename A, typename B, typename E>
static auto glm_shard_call(const glm_shard& s, const A& a, const B& b, const E& e) {
  if constexpr (K == 0) return bernoulli_logit_glm_lpmf<false>(s, a, b);
  else if constexpr (K == 1) return normal_id_glm_lpdf<false>(s, a, b, e);
  else if constexpr (K == 2) return poisson_log_glm_lpmf<false>(s, a, b);
  else return neg_binomial_2_log_glm_lpmf<false>(s, a, b, e);
}

template <int K>
static glm_shard shard_of(const data& d, long long b0, long long b1) {
  glm_shard sh;
  if (K == 1) sh.yd = d.y1d.data() + b0;
  else sh.y = d.yd[K].data() + b0;
  sh.x = d.xd.data() + b0;
  sh.rows = b1 - b0;
  sh.M = d.M;
  sh.ldx = d.R;
  sh.row0 = b0;
  sh.total_rows = b1 - b0;
  return sh;
}

static constexpr bool has_extra(int k) { return k == 1 || k == 3; }

// theta = [alpha(R) if av][beta(M), extra if bv]
template <int K>
static std::vector<double> theta_of(const data& d, bool av, bool bv) {
  std::vector<double> t;
  if (av) t = d.alpha;
  if (bv) {
    t.insert(t.end(), d.beta.begin(), d.beta.end());
    if (has_extra(K)) t.push_back(d.extra[K]);
  }
  return t;
}

// f(alpha vars | nothing, beta vars | data, extra var | data) from theta
template <int K, bool AV, bool BV, typename F>
static var with_theta(const data& d, const std::vector<var>& t, const F& f) {
  size_t at = 0;
  std::vector<var> a;
  if (AV) {
    a.assign(t.begin(), t.begin() + d.R);
    at = size_t(d.R);
  }
  if constexpr (BV) {
    std::vector<var> b(t.begin() + at, t.begin() + at + d.M);
    var e = has_extra(K) ? t[at + size_t(d.M)] : var(0.0);
    return f(a, b, e);
  } else {
    return f(a, d.beta, d.extra[K]);
  }
}

template <int K, bool BV>
static void forms(const data& d, const dev_data<double>& alpha_dd) {
  const std::string k = std::to_string(K), b = BV ? "_v" : "_d";
  double fx;
  std::vector<double> g;
  auto run = [&](const std::string& tag, bool av, auto f, auto fp) {
    const auto t0 = theta_of<K>(d, av, BV);
    gradient(f, t0, fx, g);
    print1("fx_" + k + tag + b, fx);
    print("grad_" + k + tag + b, g);
    gradient(fp, t0, fx, g);
    print1("fxp_" + k + tag + b, fx);
    print("gradp_" + k + tag + b, g);
  };
  run("_hv", true,
      [&](const std::vector<var>& t) {
        return with_theta<K, true, BV>(d, t, [&](const auto& a, const auto& bb, const auto& e) {
          return var(glm<K, false>(d, a, bb, e));
        });
      },
      [&](const std::vector<var>& t) {
        return with_theta<K, true, BV>(d, t, [&](const auto& a, const auto& bb, const auto& e) {
          return var(glm<K, true>(d, a, bb, e));
        });
      });
  run("_dv", true,
      [&](const std::vector<var>& t) {
        return with_theta<K, true, BV>(d, t, [&](const auto& a, const auto& bb, const auto& e) {
          return var(glm<K, false>(d, to_dev(a), bb, e));
        });
      },
      [&](const std::vector<var>& t) {
        return with_theta<K, true, BV>(d, t, [&](const auto& a, const auto& bb, const auto& e) {
          return var(glm<K, true>(d, to_dev(a, 1, int(a.size())), bb, e));  // (a 1 x R row here)
        });
      });
  if constexpr (BV) {
    run("_hd", false,
        [&](const std::vector<var>& t) {
          return with_theta<K, false, true>(d, t, [&](const auto&, const auto& bb, const auto& e) {
            return var(glm<K, false>(d, d.alpha, bb, e));
          });
        },
        [&](const std::vector<var>& t) {
          return with_theta<K, false, true>(d, t, [&](const auto&, const auto& bb, const auto& e) {
            return var(glm<K, true>(d, d.alpha, bb, e));
          });
        });
    run("_dd", false,
        [&](const std::vector<var>& t) {
          return with_theta<K, false, true>(d, t, [&](const auto&, const auto& bb, const auto& e) {
            return var(glm<K, false>(d, alpha_dd, bb, e));
          });
        },
        [&](const std::vector<var>& t) {
          return with_theta<K, false, true>(d, t, [&](const auto&, const auto& bb, const auto& e) {
            return var(glm<K, true>(d, alpha_dd, bb, e));
          });
        });
  } else {
    // every operand data: a plain double, no tape; propto drops everything
    static_assert(std::is_same<decltype(glm<K, false>(d, d.alpha, d.beta, d.extra[K])), double>::value, "double");
    static_assert(std::is_same<decltype(glm<K, false>(d, alpha_dd, d.beta, d.extra[K])), double>::value, "double");
    static_assert(std::is_same<decltype(glm<K, false>(d, std::vector<var>(), d.beta, d.extra[K])), var>::value, "var");
    static_assert(std::is_same<decltype(glm<K, false>(d, dev_var_matrix(), d.beta, d.extra[K])), var>::value, "var");
    start_nested();
    print1("fx_" + k + "_hd_d", glm<K, false>(d, d.alpha, d.beta, d.extra[K]));
    print1("fxp_" + k + "_hd_d", glm<K, true>(d, d.alpha, d.beta, d.extra[K]));
    print1("fx_" + k + "_dd_d", glm<K, false>(d, alpha_dd, d.beta, d.extra[K]));
    print1("fxp_" + k + "_dd_d", glm<K, true>(d, alpha_dd, d.beta, d.extra[K]));
    recover_memory_nested();
  }
}

template <int K>
static void sharding_eigen_host(const data& d) {
  const std::string k = std::to_string(K);
  const int R = d.R, M = d.M;
  const auto th = theta_of<K>(d, true, true);
  double fx;
  std::vector<double> g;
  // seven contiguous row shards summed on the tape, each with its slice of alpha
  gradient(
      [&](const std::vector<var>& t) {
        return with_theta<K, true, true>(d, t, [&](const auto& a, const auto& b, const auto& e) {
          var s = 0.0;
          for (int i = 0; i < 7; ++i) {
            long long b0, b1;
            row_partition(R, 7, i, &b0, &b1);
            const std::vector<var> ai(a.begin() + b0, a.begin() + b1);
            if (i % 2) s += glm_shard_call<K>(shard_of<K>(d, b0, b1), to_dev(ai), b, e);
            else s += glm_shard_call<K>(shard_of<K>(d, b0, b1), ai, b, e);
          }
          return s;
        });
      },
      th, fx, g);
  print1("fx_" + k + "_shards7", fx);
  print("grad_" + k + "_shards7", g);
  // one shard, distributed, under a one-rank host collective
  amd::set_host_collective(1, 0, one_rank_allgather, nullptr);
  gradient(
      [&](const std::vector<var>& t) {
        return with_theta<K, true, true>(d, t, [&](const auto& a, const auto& b, const auto& e) {
          glm_shard sh = shard_of<K>(d, 0, R);
          sh.total_rows = R;
          sh.distributed = true;
          return var(glm_shard_call<K>(sh, a, b, e));
        });
      },
      th, fx, g);
  amd::set_host_collective(1, 0, nullptr, nullptr);
  print1("fx_" + k + "_dist", fx);
  print("grad_" + k + "_dist", g);
  // the Eigen signatures: alpha a column vector of var, then a row vector of double
  const matrix_d xe = Eigen::Map<const matrix_d>(d.x.data(), R, M);
  Eigen::Matrix<double, Eigen::Dynamic, 1> y1e(R);
  for (int i = 0; i < R; ++i) y1e(i) = d.y1[size_t(i)];
  auto eigen_call = [&](const auto& a, const auto& b, const auto& e) {
    if constexpr (K == 0) return bernoulli_logit_glm_lpmf(d.y[0], xe, a, b);
    else if constexpr (K == 1) return normal_id_glm_lpdf(y1e, xe, a, b, e);
    else if constexpr (K == 2) return poisson_log_glm_lpmf(d.y[2], xe, a, b);
    else return neg_binomial_2_log_glm_lpmf(d.y[3], xe, a, b, e);
  };
  gradient(
      [&](const std::vector<var>& t) {
        return with_theta<K, true, true>(d, t, [&](const auto& a, const auto& b, const auto& e) {
          Eigen::Matrix<var, Eigen::Dynamic, 1> ae(R), be(M);
          for (int i = 0; i < R; ++i) ae(i) = a[size_t(i)];
          for (int j = 0; j < M; ++j) be(j) = b[size_t(j)];
          return var(eigen_call(ae, be, e));
        });
      },
      th, fx, g);
  print1("fx_" + k + "_eigen", fx);
  print("grad_" + k + "_eigen", g);
  {
    Eigen::Matrix<double, 1, Eigen::Dynamic> ar(R);
    Eigen::Matrix<double, Eigen::Dynamic, 1> bd(M);
    for (int i = 0; i < R; ++i) ar(i) = d.alpha[size_t(i)];
    for (int j = 0; j < M; ++j) bd(j) = d.beta[size_t(j)];
    static_assert(std::is_same<decltype(eigen_call(ar, bd, d.extra[K])), double>::value, "all double: a double");
    start_nested();
    print1("fx_" + k + "_eigenrow", eigen_call(ar, bd, d.extra[K]));
    recover_memory_nested();
  }
  // host vectors (uploaded per call)
  gradient(
      [&](const std::vector<var>& t) {
        return with_theta<K, true, true>(d, t, [&](const auto& a, const auto& b, const auto& e) {
          if constexpr (K == 0) return var(bernoulli_logit_glm_lpmf<false>(d.y[0], d.x, M, a, b));
          else if constexpr (K == 1) return var(normal_id_glm_lpdf<false>(d.y1, d.x, M, a, b, e));
          else if constexpr (K == 2) return var(poisson_log_glm_lpmf<false>(d.y[2], d.x, M, a, b));
          else return var(neg_binomial_2_log_glm_lpmf<false>(d.y[3], d.x, M, a, b, e));
        });
      },
      th, fx, g);
  print1("fx_" + k + "_host", fx);
  print("grad_" + k + "_host", g);
}

template <int K>
static void kind_all(const data& d) {
  forms<K, true>(d, d.alpha_dd);
  forms<K, false>(d, d.alpha_dd);
  sharding_eigen_host<K>(d);
}

// the latent GP: f = L eta on the device as the intercepts of a GLM without
// columns; `host`: f brought to the host and passed as std::vector<var>
template <bool BERN>
static void latent_gp(const std::string& tag, const std::vector<double>& x, double sigma, double l,
                      const std::vector<double>& eta0, const std::vector<int>& y) {
  const int N = int(x.size());
  std::vector<double> th = {sigma, l};
  th.insert(th.end(), eta0.begin(), eta0.end());
  for (int host = 0; host < 2; ++host) {
    double fx;
    std::vector<double> g;
    gradient(
        [&](const std::vector<var>& t) {
          const std::vector<var> eta(t.begin() + 2, t.end());
          auto L = cholesky_decompose(add_diag(gp_exp_quad_cov(x, t[0], t[1]), 1e-6));
          const dev_var_matrix f = multiply(L, to_dev(eta));
          const dev_data<int> yd = to_dev_data(y);
          const dev_data<double> nox(nullptr, 0, N, 0);
          const std::vector<double> nobeta;
          var lp = normal_lpdf(eta, 0.0, 1.0);
          if (host) {
            const std::vector<var> fh = to_var_vector(f);
            if constexpr (BERN) lp += bernoulli_logit_glm_lpmf(yd, nox, fh, nobeta);
            else lp += poisson_log_glm_lpmf(yd, nox, fh, nobeta);
          } else {
            if constexpr (BERN) lp += bernoulli_logit_glm_lpmf(yd, nox, f, nobeta);
            else lp += poisson_log_glm_lpmf(yd, nox, f, nobeta);
          }
          return lp;
        },
        th, fx, g);
    print1("fx_gp_" + tag + (host ? "_host" : "_dev"), fx);
    print("grad_gp_" + tag + (host ? "_host" : "_dev"), g);
  }
}

static void cmd_tape() {
  data d;
  std::cin >> d.R >> d.M;
  const int R = d.R, M = d.M;
  d.x = read_vec(size_t(R) * M);
  d.beta = read_vec(size_t(M));
  d.alpha = read_vec(size_t(R));
  d.extra[0] = d.extra[2] = 0.0;
  std::cin >> d.extra[1] >> d.extra[3];
  for (int k = 0; k < 4; ++k) {
    const auto yv = read_vec(size_t(R));
    if (k == 1) d.y1 = yv;
    d.y[k].assign(yv.begin(), yv.end());
  }
  d.xd = to_dev_data(d.x.data(), d.x.size(), R, M);
  d.y1d = to_dev_data(d.y1);
  d.alpha_dd = to_dev_data(d.alpha.data(), d.alpha.size(), R, 1);
  for (int k = 0; k < 4; ++k) d.yd[k] = to_dev_data(d.y[k]);

  kind_all<0>(d);
  kind_all<1>(d);
  kind_all<2>(d);
  kind_all<3>(d);

  // one device alpha, two GLM calls on one tape: its adjoint takes both theta'
  {
    double fx;
    std::vector<double> g;
    gradient(
        [&](const std::vector<var>& t) {
          const dev_var_matrix a = to_dev(t);
          return var(poisson_log_glm_lpmf(d.yd[2], d.xd, a, d.beta)) +
                 neg_binomial_2_log_glm_lpmf(d.yd[3], d.xd, a, d.beta, d.extra[3]);
        },
        d.alpha, fx, g);
    print1("fx_two", fx);
    print("grad_two", g);
  }

  std::string word;
  int N;
  std::cin >> word >> N;
  if (word != "gp") throw std::runtime_error("expected the gp block");
  const auto x = read_vec(size_t(N));
  double sigma, l;
  std::cin >> sigma >> l;
  const auto eta = read_vec(size_t(N));
  const auto yc = read_vec(size_t(N)), yb = read_vec(size_t(N));
  latent_gp<false>("p", x, sigma, l, eta, std::vector<int>(yc.begin(), yc.end()));
  latent_gp<true>("b", x, sigma, l, eta, std::vector<int>(yb.begin(), yb.end()));
  std::printf("stack %zu %zu\n", ChainableStack::instance_->var_stack_.size(),
              ChainableStack::instance_->dev_adj_stack_.size());
}

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

template <int K>
static void errors_of_kind() {
  const double inf = std::numeric_limits<double>::infinity();
  const std::string k = std::to_string(K) + "_";
  const std::vector<int> y = K == 0 ? std::vector<int>{1, 0, 1, 0} : std::vector<int>{1, 0, 4, 2};
  const std::vector<double> y1 = {1.0, 0.0, 4.0, 2.0};
  const std::vector<double> x = {0.5, -0.25, 1.0, 0.75, -1.0, 0.5, 0.25, 0.125};  // 4 x 2
  const std::vector<double> beta = {0.3, -0.2}, alpha = {0.1, -0.1, 0.2, 0.05};
  // host vectors; alpha through `wrap` (host vars by default)
  auto call = [&](const std::vector<int>& yy, const std::vector<double>& aa, const std::vector<double>& bb,
                  bool dev = false) {
    std::vector<var> a(aa.begin(), aa.end()), b(bb.begin(), bb.end());
    var e = 2.5;
    const std::vector<double> yd(yy.begin(), yy.end());
    auto go = [&](const auto& av) {
      if constexpr (K == 0) return bernoulli_logit_glm_lpmf(yy, x, 2, av, b).val();
      else if constexpr (K == 1) return normal_id_glm_lpdf(yd, x, 2, av, b, e).val();
      else if constexpr (K == 2) return poisson_log_glm_lpmf(yy, x, 2, av, b).val();
      else return neg_binomial_2_log_glm_lpmf(yy, x, 2, av, b, e).val();
    };
    return dev ? go(to_dev(a)) : go(a);
  };
  expect(k + "ok", [&] { return call(y, alpha, beta); });
  expect(k + "ok_dev", [&] { return call(y, alpha, beta, true); });
  expect(k + "alpha_size", [&] { return call(y, {0.1, -0.1, 0.2}, beta); });
  expect(k + "alpha_size_dev", [&] { return call(y, {0.1, -0.1, 0.2}, beta, true); });
  expect(k + "alpha_matrix_dev", [&] {  // R elements, but 2 x 2: not a vector
    std::vector<var> a(alpha.begin(), alpha.end()), b(beta.begin(), beta.end());
    const dev_var_matrix am = to_dev(a, 2, 2);
    if constexpr (K == 0) return bernoulli_logit_glm_lpmf(y, x, 2, am, b).val();
    else if constexpr (K == 1) return normal_id_glm_lpdf(y1, x, 2, am, b, var(2.5)).val();
    else if constexpr (K == 2) return poisson_log_glm_lpmf(y, x, 2, am, b).val();
    else return neg_binomial_2_log_glm_lpmf(y, x, 2, am, b, var(2.5)).val();
  });
  expect(k + "alpha_null_dev", [&] {  // a default-constructed matrix: the empty vector, a wrong length
    std::vector<var> b(beta.begin(), beta.end());
    const dev_var_matrix am;
    if constexpr (K == 0) return bernoulli_logit_glm_lpmf(y, x, 2, am, b).val();
    else if constexpr (K == 1) return normal_id_glm_lpdf(y1, x, 2, am, b, var(2.5)).val();
    else if constexpr (K == 2) return poisson_log_glm_lpmf(y, x, 2, am, b).val();
    else return neg_binomial_2_log_glm_lpmf(y, x, 2, am, b, var(2.5)).val();
  });
  expect(k + "alpha_size_eigen", [&] {
    const matrix_d xe = Eigen::Map<const matrix_d>(x.data(), 4, 2);
    Eigen::Matrix<var, Eigen::Dynamic, 1> a(3), b(2);
    for (int i = 0; i < 3; ++i) a(i) = alpha[size_t(i)];
    for (int j = 0; j < 2; ++j) b(j) = beta[size_t(j)];
    Eigen::Matrix<double, Eigen::Dynamic, 1> ye(4);
    for (int i = 0; i < 4; ++i) ye(i) = y1[size_t(i)];
    if constexpr (K == 0) return bernoulli_logit_glm_lpmf(y, xe, a, b).val();
    else if constexpr (K == 1) return normal_id_glm_lpdf(ye, xe, a, b, var(2.5)).val();
    else if constexpr (K == 2) return poisson_log_glm_lpmf(y, xe, a, b).val();
    else return neg_binomial_2_log_glm_lpmf(y, xe, a, b, var(2.5)).val();
  });
  expect(k + "alpha_and_beta_size", [&] { return call(y, {0.1, -0.1, 0.2}, {0.3, -0.2, 0.1}); });
  expect(k + "alpha_inf", [&] { return call(y, {0.1, inf, 0.2, 0.05}, beta); });
  expect(k + "alpha_inf_dev", [&] { return call(y, {0.1, inf, 0.2, 0.05}, beta, true); });
  expect(k + "alpha_inf_data", [&] {
    const std::vector<double> a = {0.1, inf, 0.2, 0.05};
    std::vector<var> b(beta.begin(), beta.end());
    if constexpr (K == 0) return bernoulli_logit_glm_lpmf(y, x, 2, a, b).val();
    else if constexpr (K == 1) return normal_id_glm_lpdf(y1, x, 2, a, b, 2.5).val();
    else if constexpr (K == 2) return poisson_log_glm_lpmf(y, x, 2, a, b).val();
    else return neg_binomial_2_log_glm_lpmf(y, x, 2, a, b, 2.5).val();
  });
  expect(k + "beta_and_alpha_inf", [&] { return call(y, {0.1, inf, 0.2, 0.05}, {inf, -0.2}); });
  if (K != 1) {
    const std::vector<int> ybad = K == 0 ? std::vector<int>{1, 0, 2, 0} : std::vector<int>{1, 0, -2, 2};
    expect(k + "y_domain_and_alpha_inf", [&] { return call(ybad, {0.1, inf, 0.2, 0.05}, beta); });
  }
  expect(k + "empty_y", [&] {
    std::vector<var> a, b(beta.begin(), beta.end());
    if constexpr (K == 0) return bernoulli_logit_glm_lpmf(std::vector<int>{}, std::vector<double>{}, 2, a, b).val();
    else if constexpr (K == 1)
      return normal_id_glm_lpdf(std::vector<double>{}, std::vector<double>{}, 2, a, b, var(2.5)).val();
    else if constexpr (K == 2) return poisson_log_glm_lpmf(std::vector<int>{}, std::vector<double>{}, 2, a, b).val();
    else return neg_binomial_2_log_glm_lpmf(std::vector<int>{}, std::vector<double>{}, 2, a, b, var(2.5)).val();
  });
}

static void cmd_errors() {
  errors_of_kind<0>();
  errors_of_kind<1>();
  errors_of_kind<2>();
  errors_of_kind<3>();
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
