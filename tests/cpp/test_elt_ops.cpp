// The element-wise device nodes (rev/fun/elt_ops.hpp) through
// stan::math::gradient; the values are compared in tests/test_elt_ops.py.
//
// stdin, mode "tape":
//   tape N a(N) b(N) w(N) d(N) c
//   scalars K x(K)
//   gp N x(N) gp_sigma gp_l mu eta(N) ycount(N)
//   het N y(N) f(N) g(N) nu
//   hs N M X(N*M, column-major) y(N) z(M) lambda(M) tau sigma
// a: reals, b: positive reals, w: the weights of the objective, d: a positive
// data vector, c: a scalar.  Prints "<tag> values..." lines, every objective
// being dot_product(w, result) so that the adjoints differ per element:
//   fx_u_<fn>_<dev|host> / grad_: the unary fn of a var vector (b for log,
//       sqrt, inv; a for the others), on the device and composed of host
//       scalar vars.
//   fx_b_<fn>_<AB>_<dev|host> / grad_: the binary fn; A, B the operand kinds
//       v (var matrix: a first, b second), d (data matrix d), s (scalar var
//       c), c (double c); the gradient over the var operands in order.
//   fx_two_<mul|sub>_<dev|host> / grad_: elt_multiply(x, x), subtract(exp(x), x).
//   sv_<fn> / sg_<fn>: the new scalar var overloads' values and derivatives on x(K).
//   fx_<gp|het|hs>_<dev|host> / grad_: the three composed models.
//   stack: the stack sizes afterwards; arena: the device arena's use before
//       and after a nested block of every node kind.
// mode "errors": one line "<case>|<exception type or value>|<message>".
#include <stan/math.hpp>

#include <cmath>
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
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

struct data {
  size_t n;
  std::vector<double> a, b, w, d;
  double c;
};

template <typename F>
static void run(const std::string& tag, const std::vector<double>& th, const F& f) {
  double fx;
  std::vector<double> g;
  gradient(f, th, fx, g);
  print1("fx_" + tag, fx);
  print("grad_" + tag, g);
}

static std::vector<var> slice(const std::vector<var>& t, size_t at, size_t n) {
  return std::vector<var>(t.begin() + long(at), t.begin() + long(at + n));
}
static var wdot(const data& d, const dev_var_matrix& m) {
  return dot_product(to_dev_var_matrix(d.w.data(), int(d.n), 1), m);
}
static std::vector<double> cat(const std::vector<double>& x, const std::vector<double>& y) {
  std::vector<double> r(x);
  r.insert(r.end(), y.begin(), y.end());
  return r;
}

// ------------------------------------------------------------------ unary
template <typename Dev, typename Host>
static void unary(const data& d, const std::string& fn, bool positive, const Dev& dev, const Host& host) {
  const std::vector<double>& x0 = positive ? d.b : d.a;
  run("u_" + fn + "_dev", x0, [&](const std::vector<var>& t) { return wdot(d, dev(to_dev(t))); });
  run("u_" + fn + "_host", x0, [&](const std::vector<var>& t) {
    var s = 0.0;
    for (size_t i = 0; i < d.n; ++i) s += d.w[i] * host(t[i]);
    return s;
  });
}
#define UNARY(FN, POS) \
  unary(d, #FN, POS, [](const dev_var_matrix& x) { return FN(x); }, [](const var& x) { return FN(x); })

// ------------------------------------------------------------------ binary
// operand of kind K at the tape position `at`: the device form and element i of the host form
template <char K>
static auto dev_op(const data& d, const std::vector<var>& t, size_t& at) {
  if constexpr (K == 'v') {
    at += d.n;
    return to_dev(slice(t, at - d.n, d.n));
  } else if constexpr (K == 'd') {
    return to_dev_data(d.d);
  } else if constexpr (K == 's') {
    return t[at++];
  } else {
    return d.c;
  }
}
template <char K>
static auto host_op(const data& d, const std::vector<var>& t, size_t at, size_t i) {
  if constexpr (K == 'v') return t[at + i];
  else if constexpr (K == 'd') return d.d[i];
  else if constexpr (K == 's') return t[at];
  else return d.c;
}
template <char K>
static size_t width(const data& d) {
  return K == 'v' ? d.n : K == 's' ? 1 : 0;
}

template <char KA, char KB, typename Dev, typename Host>
static void binary(const data& d, const std::string& fn, const Dev& dev, const Host& host) {
  std::vector<double> th;
  if (KA == 'v') th = d.a;
  if (KA == 's') th.push_back(d.c);
  if (KB == 'v') th = cat(th, d.b);
  if (KB == 's') th.push_back(d.c);
  const std::string tag = "b_" + fn + "_" + KA + KB;
  run(tag + "_dev", th, [&](const std::vector<var>& t) {
    size_t at = 0;
    const auto A = dev_op<KA>(d, t, at);
    const auto B = dev_op<KB>(d, t, at);
    return wdot(d, dev(A, B));
  });
  run(tag + "_host", th, [&](const std::vector<var>& t) {
    var s = 0.0;
    for (size_t i = 0; i < d.n; ++i) s += d.w[i] * host(host_op<KA>(d, t, 0, i), host_op<KB>(d, t, width<KA>(d), i));
    return s;
  });
}
#define DEVFN(FN) [](const auto& x, const auto& y) { return FN(x, y); }
#define HOSTFN(OP) [](const auto& x, const auto& y) { return var(x OP y); }

static void cmd_tape() {
  data d;
  std::cin >> d.n;
  d.a = read_vec(d.n);
  d.b = read_vec(d.n);
  d.w = read_vec(d.n);
  d.d = read_vec(d.n);
  std::cin >> d.c;

  UNARY(exp, false);
  UNARY(log, true);
  UNARY(sqrt, true);
  UNARY(square, false);
  UNARY(inv, true);
  UNARY(inv_logit, false);
  UNARY(log_inv_logit, false);
  UNARY(log1p_exp, false);
  UNARY(tanh, false);

  // matrix with matrix: every pairing with at least one var (add(v, v) is the existing node)
  binary<'v', 'v'>(d, "add", DEVFN(add), HOSTFN(+));
  binary<'v', 'd'>(d, "add", DEVFN(add), HOSTFN(+));
  binary<'d', 'v'>(d, "add", DEVFN(add), HOSTFN(+));
  binary<'v', 'v'>(d, "subtract", DEVFN(subtract), HOSTFN(-));
  binary<'v', 'd'>(d, "subtract", DEVFN(subtract), HOSTFN(-));
  binary<'d', 'v'>(d, "subtract", DEVFN(subtract), HOSTFN(-));
  binary<'v', 'v'>(d, "elt_multiply", DEVFN(elt_multiply), HOSTFN(*));
  binary<'v', 'd'>(d, "elt_multiply", DEVFN(elt_multiply), HOSTFN(*));
  binary<'d', 'v'>(d, "elt_multiply", DEVFN(elt_multiply), HOSTFN(*));
  binary<'v', 'v'>(d, "elt_divide", DEVFN(elt_divide), HOSTFN(/));
  binary<'v', 'd'>(d, "elt_divide", DEVFN(elt_divide), HOSTFN(/));
  binary<'d', 'v'>(d, "elt_divide", DEVFN(elt_divide), HOSTFN(/));
  // matrix with scalar, var and double
  binary<'v', 's'>(d, "add", DEVFN(add), HOSTFN(+));
  binary<'v', 'c'>(d, "add", DEVFN(add), HOSTFN(+));
  binary<'s', 'v'>(d, "add", DEVFN(add), HOSTFN(+));
  binary<'c', 'v'>(d, "add", DEVFN(add), HOSTFN(+));
  binary<'v', 's'>(d, "subtract", DEVFN(subtract), HOSTFN(-));
  binary<'v', 'c'>(d, "subtract", DEVFN(subtract), HOSTFN(-));
  binary<'s', 'v'>(d, "subtract", DEVFN(subtract), HOSTFN(-));
  binary<'c', 'v'>(d, "subtract", DEVFN(subtract), HOSTFN(-));
  binary<'v', 's'>(d, "divide", DEVFN(divide), HOSTFN(/));
  binary<'v', 'c'>(d, "divide", DEVFN(divide), HOSTFN(/));
  binary<'s', 'v'>(d, "elt_divide", DEVFN(elt_divide), HOSTFN(/));
  binary<'c', 'v'>(d, "elt_divide", DEVFN(elt_divide), HOSTFN(/));

  // one operand in two places: a node's adjoint fed by two consumers
  run("two_mul_dev", d.a, [&](const std::vector<var>& t) {
    const dev_var_matrix x = to_dev(t);
    return wdot(d, elt_multiply(x, x));
  });
  run("two_mul_host", d.a, [&](const std::vector<var>& t) {
    var s = 0.0;
    for (size_t i = 0; i < d.n; ++i) s += d.w[i] * (t[i] * t[i]);
    return s;
  });
  run("two_sub_dev", d.a, [&](const std::vector<var>& t) {
    const dev_var_matrix x = to_dev(t);
    return wdot(d, subtract(exp(x), x));
  });
  run("two_sub_host", d.a, [&](const std::vector<var>& t) {
    var s = 0.0;
    for (size_t i = 0; i < d.n; ++i) s += d.w[i] * (exp(t[i]) - t[i]);
    return s;
  });
}

// ------------------------------------------------------------------ the new scalar overloads
template <typename F>
static void scalar_fn(const std::string& fn, const std::vector<double>& x, const F& f) {
  std::vector<double> v(x.size()), g(x.size());
  for (size_t i = 0; i < x.size(); ++i) {
    std::vector<double> gi;
    gradient([&](const std::vector<var>& t) { return f(t[0]); }, std::vector<double>{x[i]}, v[i], gi);
    g[i] = gi[0];
  }
  print("sv_" + fn, v);
  print("sg_" + fn, g);
}

static void cmd_scalars() {
  size_t k;
  std::cin >> k;
  const auto x = read_vec(k);
  scalar_fn("inv", x, [](const var& a) { return inv(a); });
  scalar_fn("inv_logit", x, [](const var& a) { return inv_logit(a); });
  scalar_fn("log_inv_logit", x, [](const var& a) { return log_inv_logit(a); });
  scalar_fn("log1p_exp", x, [](const var& a) { return log1p_exp(a); });
  scalar_fn("tanh", x, [](const var& a) { return tanh(a); });
}

// ------------------------------------------------------------------ composed models
// shifted latent GP: f = mu + L eta as the per-row intercept of a Poisson GLM without columns
static void cmd_gp() {
  size_t N;
  std::cin >> N;
  const auto x = read_vec(N);
  double gs, gl, mu;
  std::cin >> gs >> gl >> mu;
  const auto eta0 = read_vec(N), yc = read_vec(N);
  const std::vector<int> y(yc.begin(), yc.end());
  std::vector<double> th = {gs, gl, mu};
  th = cat(th, eta0);
  for (int host = 0; host < 2; ++host)
    run(std::string("gp_") + (host ? "host" : "dev"), th, [&](const std::vector<var>& t) {
      const std::vector<var> eta = slice(t, 3, N);
      auto L = cholesky_decompose(add_diag(gp_exp_quad_cov(x, t[0], t[1]), 1e-6));
      const dev_var_matrix Le = multiply(L, to_dev(eta));
      const dev_data<int> yd = to_dev_data(y);
      const dev_data<double> nox(nullptr, 0, int(N), 0);
      const std::vector<double> nobeta;
      var lp = normal_lpdf(eta, 0.0, 1.0);
      if (host) {
        std::vector<var> fh = to_var_vector(Le);
        for (auto& e : fh) e = t[2] + e;
        lp += poisson_log_glm_lpmf(yd, nox, fh, nobeta);
      } else {
        lp += poisson_log_glm_lpmf(yd, nox, add(t[2], Le), nobeta);
      }
      return lp;
    });
}

// heteroscedastic robust regression: student_t_lpdf(y | nu, f, exp(g)), f and g device vectors
static void cmd_het() {
  size_t N;
  std::cin >> N;
  const auto y = read_vec(N), f0 = read_vec(N), g0 = read_vec(N);
  double nu;
  std::cin >> nu;
  std::vector<double> th = cat(f0, g0);
  th.push_back(nu);
  for (int host = 0; host < 2; ++host)
    run(std::string("het_") + (host ? "host" : "dev"), th, [&](const std::vector<var>& t) {
      const std::vector<var> f = slice(t, 0, N), g = slice(t, N, N);
      if (host) {
        std::vector<var> s(N);
        for (size_t i = 0; i < N; ++i) s[i] = exp(g[i]);
        return var(student_t_lpdf(y, t[2 * N], f, s));
      }
      return var(student_t_lpdf(to_dev_data(y), t[2 * N], to_dev(f), exp(to_dev(g))));
    });
}

// horseshoe: beta = tau (z .* lambda), lambda ~ cauchy(0, 1), y ~ normal(X beta, sigma)
static void cmd_hs() {
  size_t N, M;
  std::cin >> N >> M;
  const auto X = read_vec(N * M), y = read_vec(N), z0 = read_vec(M), l0 = read_vec(M);
  double tau, sigma;
  std::cin >> tau >> sigma;
  std::vector<double> th = cat(z0, l0);
  th.push_back(tau);
  th.push_back(sigma);
  for (int host = 0; host < 2; ++host)
    run(std::string("hs_") + (host ? "host" : "dev"), th, [&](const std::vector<var>& t) {
      const std::vector<var> z = slice(t, 0, M), lam = slice(t, M, M);
      const var tv = t[2 * M], sv = t[2 * M + 1];
      if (host) {
        std::vector<var> mu(N);
        for (size_t i = 0; i < N; ++i) {
          var s = 0.0;
          for (size_t j = 0; j < M; ++j) s += X[i + j * N] * (tv * (z[j] * lam[j]));
          mu[i] = s;
        }
        return var(cauchy_lpdf(lam, 0.0, 1.0) + normal_lpdf(y, mu, sv));
      }
      const dev_var_matrix ld = to_dev(lam);
      const dev_var_matrix beta = multiply(tv, elt_multiply(to_dev(z), ld));
      const dev_data<double> Xd = to_dev_data(X.data(), X.size(), int(N), int(M));
      return var(cauchy_lpdf(ld, 0.0, 1.0) + normal_lpdf(to_dev_data(y), multiply(Xd, beta), sv));
    });
}

// the device arena's use around a nested block holding every node kind
static void cmd_arena() {
  const std::vector<double> v = {0.5, 1.5, 2.5, 3.5, 4.5};
  {  // (the context and its first blocks exist before the mark)
    start_nested();
    sum(exp(to_dev_var_matrix(v.data(), 5, 1))).grad();
    recover_memory_nested();
  }
  const size_t before = smg_arena_used(amd::ctx());
  start_nested();
  const dev_var_matrix x = to_dev_var_matrix(v.data(), 5, 1);
  var c = 1.25;
  var s = sum(elt_divide(c, add(subtract(log1p_exp(x), c), elt_multiply(x, to_dev_data(v)))));
  s.grad();
  const size_t inside = smg_arena_used(amd::ctx());
  recover_memory_nested();
  std::printf("arena %zu %zu %zu\n", before, inside, (size_t)smg_arena_used(amd::ctx()));
}

// ------------------------------------------------------------------ errors
template <typename F>
static void expect(const std::string& name, const F& f) {
  start_nested();
  try {
    const std::string v = f();
    std::printf("%s|value|%s\n", name.c_str(), v.c_str());
  } catch (const std::invalid_argument& e) {
    std::printf("%s|invalid_argument|%s\n", name.c_str(), e.what());
  } catch (const std::exception& e) {
    std::printf("%s|other|%s\n", name.c_str(), e.what());
  }
  recover_memory_nested();
}

static std::string shape_of(const dev_var_matrix& m) {
  return std::to_string(m.rows()) + "x" + std::to_string(m.cols()) + ":" + std::to_string(m.size());
}

static void cmd_errors() {
  const std::vector<double> v4 = {1.0, 2.0, 3.0, 4.0}, v3 = {1.0, 2.0, 3.0}, v6 = {1, 2, 3, 4, 5, 6};
  auto A4 = [&] { return to_dev_var_matrix(v4.data(), 4, 1); };
  auto A3 = [&] { return to_dev_var_matrix(v3.data(), 3, 1); };
  expect("subtract_vv", [&] { return shape_of(subtract(A4(), A3())); });
  expect("subtract_vd", [&] { return shape_of(subtract(A4(), to_dev_data(v3))); });
  expect("subtract_dv", [&] { return shape_of(subtract(to_dev_data(v3), A4())); });
  expect("elt_multiply_vv", [&] { return shape_of(elt_multiply(A3(), A4())); });
  expect("elt_multiply_vd", [&] { return shape_of(elt_multiply(A3(), to_dev_data(v4))); });
  expect("elt_multiply_dv", [&] { return shape_of(elt_multiply(to_dev_data(v4), A3())); });
  expect("elt_divide_vv", [&] { return shape_of(elt_divide(A4(), A3())); });
  expect("elt_divide_vd", [&] { return shape_of(elt_divide(A4(), to_dev_data(v3))); });
  expect("elt_divide_dv", [&] { return shape_of(elt_divide(to_dev_data(v3), A4())); });
  expect("add_vd", [&] { return shape_of(add(A4(), to_dev_data(v3))); });
  expect("add_dv", [&] { return shape_of(add(to_dev_data(v3), A4())); });
  // the same count in another shape is a mismatch too
  expect("subtract_reshaped", [&] {
    return shape_of(subtract(to_dev_var_matrix(v6.data(), 2, 3), to_dev_var_matrix(v6.data(), 3, 2)));
  });
  expect("ok_matrix", [&] {
    return shape_of(elt_multiply(to_dev_var_matrix(v6.data(), 2, 3), to_dev_data(v6.data(), 6, 2, 3)));
  });
  // a size-zero operand: an empty matrix, and the tape still sweeps
  expect("empty", [&] {
    const dev_var_matrix e = to_dev_var_matrix(v4.data(), 0, 1);
    const dev_data<double> ed(nullptr, 0, 0, 1);
    var c = 2.0;
    const dev_var_matrix r[] = {exp(e),       tanh(e),        inv_logit(e),    subtract(e, e), elt_multiply(e, ed),
                                add(ed, e),   add(e, c),      subtract(1.5, e), divide(e, c),   elt_divide(c, e)};
    std::string s;
    for (const auto& m : r) s += shape_of(m) + " ";
    const dev_var_matrix x = A4();
    var f = sum(square(x)) + c * c;
    f.grad();
    const std::vector<double> g = x.adj();
    return s + std::to_string(g[3]) + " " + std::to_string(c.adj());
  });
  std::printf("stack|%zu|%zu\n", ChainableStack::instance_->var_stack_.size(),
              ChainableStack::instance_->dev_adj_stack_.size());
}

int main() {
  std::string mode;
  try {
    while (std::cin >> mode) {
      if (mode == "tape") cmd_tape();
      else if (mode == "scalars") cmd_scalars();
      else if (mode == "gp") cmd_gp();
      else if (mode == "het") cmd_het();
      else if (mode == "hs") cmd_hs();
      else if (mode == "arena") cmd_arena();
      else if (mode == "errors") cmd_errors();
      else {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
      }
    }
    std::printf("stack %zu %zu\n", ChainableStack::instance_->var_stack_.size(),
                ChainableStack::instance_->dev_adj_stack_.size());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
