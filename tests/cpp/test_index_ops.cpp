// Indexing device vectors of vars by group (rev/fun/index_ops.hpp) through
// stan::math::gradient; the values are compared in tests/test_index_ops.py.
//
// stdin, mode "tape":
//   tape R J M g(R) y(R) u(J) sigma ycount(R) x(R*M, column-major) beta(M) v(R) w(J)
// g: 1-based groups, y: reals, u: the group-level vector, ycount: counts,
// v: a row-level vector, w: group weights.  The index is built ONCE, before
// every gradient() call.  Prints "<tag> values..." lines:
//   fx_/grad_normal_hostvec   normal_lpdf(y | gather(u, idx), sigma), u a std::vector<var>
//   fx_/grad_normal_leaf      the same with u a dev_var_matrix leaf
//   fx_/grad_normal_sigma     the same over (u, sigma)
//   fx_/grad_poisson_dev      poisson_log_glm_lpmf(ycount, x, gather(u, idx), beta) over (u, beta)
//   fx_/grad_poisson_host     the same with alpha a std::vector<var>, alpha[i] = u[g[i]-1]
//   fx_/grad_segsum           sum(elt_multiply(segment_sum(v, idx), w)) over v
//   fx_/grad_scale            normal_lpdf(y | 0, exp(gather(u, idx))) over u
//   fx_/grad_twice_a, _b      normal_hostvec again, twice
//   gather_data               gather of constant device data u
//   stack                     the stack sizes afterwards
// mode "bench R J M reps": timing of the hierarchical Poisson GLM (see cmd_bench).
// mode "errors": one line "<case>|<exception type or value>|<message>|tape (un)changed|arena (un)changed".
#include <stan/math.hpp>

#include <algorithm>
#include <chrono>
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

static void cmd_tape() {
  size_t R, J, M;
  std::cin >> R >> J >> M;
  std::vector<int> g(R);
  for (auto& e : g) std::cin >> e;
  const auto y = read_vec(R), u0 = read_vec(J);
  double sigma;
  std::cin >> sigma;
  const auto yc = read_vec(R), x = read_vec(R * M), beta0 = read_vec(M), v0 = read_vec(R), w = read_vec(J);
  const std::vector<int> ycount(yc.begin(), yc.end());

  // built once, outside every gradient(): they survive the nested recoveries
  const dev_index idx = to_dev_index(g, int(J));
  const dev_data<double> yd = to_dev_data(y), wd = to_dev_data(w);
  const dev_data<int> ycd = to_dev_data(ycount);
  const dev_data<double> xd = to_dev_data(x.data(), x.size(), int(R), int(M));

  const auto normal_hostvec = [&](const std::vector<var>& t) { return var(normal_lpdf(yd, gather(t, idx), sigma)); };
  run("normal_hostvec", u0, normal_hostvec);
  {
    start_nested();
    const dev_var_matrix u = to_dev_var_matrix(u0.data(), int(J), 1);
    var lp = normal_lpdf(yd, gather(u, idx), sigma);
    lp.grad();
    print1("fx_normal_leaf", lp.val());
    print("grad_normal_leaf", u.adj());
    recover_memory_nested();
  }
  {
    std::vector<double> th = u0;
    th.push_back(sigma);
    run("normal_sigma", th,
        [&](const std::vector<var>& t) { return var(normal_lpdf(yd, gather(slice(t, 0, J), idx), t[J])); });
  }
  {
    std::vector<double> th = u0;
    th.insert(th.end(), beta0.begin(), beta0.end());
    run("poisson_dev", th, [&](const std::vector<var>& t) {
      return var(poisson_log_glm_lpmf(ycd, xd, gather(slice(t, 0, J), idx), slice(t, J, M)));
    });
    run("poisson_host", th, [&](const std::vector<var>& t) {
      std::vector<var> alpha(R);
      for (size_t i = 0; i < R; ++i) alpha[i] = t[size_t(g[i]) - 1];
      return var(poisson_log_glm_lpmf(ycd, xd, alpha, slice(t, J, M)));
    });
  }
  run("segsum", v0, [&](const std::vector<var>& t) { return sum(elt_multiply(segment_sum(to_dev(t), idx), wd)); });
  run("scale", u0, [&](const std::vector<var>& t) { return var(normal_lpdf(yd, 0.0, exp(gather(t, idx)))); });
  run("twice_a", u0, normal_hostvec);
  run("twice_b", u0, normal_hostvec);
  {
    const dev_data<double> ug = gather(to_dev_data(u0), idx);
    std::vector<double> h(ug.size());
    amd::to_host(h.data(), ug.data(), h.size());
    print("gather_data", h);
  }
}

// ------------------------------------------------------------------ timing (tools/time_index.py)
// bench R J M reps: the hierarchical Poisson GLM
//   y ~ poisson_log(x beta + u[group]),  u ~ normal(0, tau)
// over (u, beta, tau), inputs generated here from a fixed stream, the index
// and the data resident.  The device form (gather) and the host-vari form
// (alpha a std::vector<var>) alternate, three warm-up evaluations of each
// first; prints the wall milliseconds of every gradient() call and the
// largest difference of the two gradients over the largest entry.
static void cmd_bench() {
  size_t R, J, M;
  int reps;
  std::cin >> R >> J >> M >> reps;
  unsigned long long s = 20260101ULL;
  auto u01 = [&s] {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return double(s >> 11) * (1.0 / 9007199254740992.0);
  };
  std::vector<int> g(R), y(R);
  std::vector<double> x(R * M), th(J + M + 1);
  for (auto& e : g) e = 1 + int(u01() * double(J));
  for (auto& e : y) e = int(u01() * 6.0);
  for (auto& e : x) e = 2.0 * u01() - 1.0;
  for (size_t j = 0; j < J; ++j) th[j] = 0.6 * (u01() - 0.5);
  for (size_t m = 0; m < M; ++m) th[J + m] = (2.0 * u01() - 1.0) * std::sqrt(3.0 / double(M));
  th[J + M] = 0.7;
  const dev_index idx = to_dev_index(g, int(J));
  const dev_data<int> yd = to_dev_data(y);
  const dev_data<double> xd = to_dev_data(x.data(), x.size(), int(R), int(M));
  const auto dev = [&](const std::vector<var>& t) {
    const dev_var_matrix u = to_dev(slice(t, 0, J));
    return var(poisson_log_glm_lpmf(yd, xd, gather(u, idx), slice(t, J, M)) + normal_lpdf(u, 0.0, t[J + M]));
  };
  const auto host = [&](const std::vector<var>& t) {
    const std::vector<var> u = slice(t, 0, J);
    std::vector<var> alpha(R);
    for (size_t i = 0; i < R; ++i) alpha[i] = u[size_t(g[i]) - 1];
    return var(poisson_log_glm_lpmf(yd, xd, alpha, slice(t, J, M)) + normal_lpdf(u, 0.0, t[J + M]));
  };
  std::vector<double> ms_dev, ms_host, g_dev, g_host;
  double fx;
  for (int rep = -3; rep < reps; ++rep)
    for (int form = 0; form < 2; ++form) {
      const auto t0 = std::chrono::steady_clock::now();
      if (form == 0) gradient(dev, th, fx, g_dev);
      else gradient(host, th, fx, g_host);
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (rep >= 0) (form == 0 ? ms_dev : ms_host).push_back(ms);
    }
  double big = 0.0, diff = 0.0;
  for (size_t k = 0; k < g_dev.size(); ++k) {
    big = std::max(big, std::fabs(g_host[k]));
    diff = std::max(diff, std::fabs(g_dev[k] - g_host[k]));
  }
  print("ms_dev", ms_dev);
  print("ms_host", ms_host);
  print1("gradient_diff", diff / big);
}

// ------------------------------------------------------------------ errors
struct marks {
  size_t vars, arena;
};
static marks now() { return {ChainableStack::instance_->var_stack_.size(), (size_t)smg_arena_used(amd::ctx())}; }

template <typename F>
static void expect(const std::string& name, const F& f) {
  const marks before = now();
  std::string kind, text;
  try {
    text = f();
    kind = "value";
  } catch (const std::out_of_range& e) {
    kind = "out_of_range";
    text = e.what();
  } catch (const std::invalid_argument& e) {
    kind = "invalid_argument";
    text = e.what();
  } catch (const std::exception& e) {
    kind = "other";
    text = e.what();
  }
  const marks after = now();
  std::printf("%s|%s|%s|%s|%s\n", name.c_str(), kind.c_str(), text.c_str(),
              before.vars == after.vars ? "tape unchanged" : "tape changed",
              before.arena == after.arena ? "arena unchanged" : "arena changed");
}

static std::string shape_of(const dev_var_matrix& m) {
  return std::to_string(m.rows()) + "x" + std::to_string(m.cols()) + ":" + std::to_string(m.size());
}

static void cmd_errors() {
  const std::vector<double> v4 = {1.0, 2.0, 3.0, 4.0}, v3 = {1.0, 2.0, 3.0};
  start_nested();
  const dev_index idx = to_dev_index({1, 4, 2, 2, 3}, 4);  // R = 5, J = 4
  const dev_index none = to_dev_index({}, 4);               // R = 0
  const dev_var_matrix u4 = to_dev_var_matrix(v4.data(), 4, 1), u3 = to_dev_var_matrix(v3.data(), 3, 1),
                       u22 = to_dev_var_matrix(v4.data(), 2, 2), row4 = to_dev_var_matrix(v4.data(), 1, 4);
  const std::vector<var> hv3(3, var(1.0));
  const dev_data<double> d3 = to_dev_data(v3), d4 = to_dev_data(v4);
  expect("index_zero", [&] { return std::to_string(to_dev_index({1, 2, 0, 3}, 4).rows()); });
  expect("index_past", [&] { return std::to_string(to_dev_index({1, 5, 0}, 4).rows()); });
  expect("index_empty", [&] { return std::to_string(to_dev_index({1}, 0).rows()); });
  expect("index_negative_size", [&] { return std::to_string(to_dev_index({}, -1).rows()); });
  expect("gather_short", [&] { return shape_of(gather(u3, idx)); });
  expect("gather_matrix", [&] { return shape_of(gather(u22, idx)); });
  expect("gather_short_hostvec", [&] { return shape_of(gather(hv3, idx)); });
  expect("gather_short_data", [&] { return std::to_string(gather(d3, idx).size()); });
  expect("segment_sum_short", [&] { return shape_of(segment_sum(u4, idx)); });
  // R = 0: an empty result and no node
  expect("gather_none", [&] { return shape_of(gather(u4, none)); });
  expect("gather_none_data", [&] { return std::to_string(gather(d4, none).size()); });
  // (these allocate: their marks change)
  expect("gather_row", [&] { return shape_of(gather(row4, idx)); });
  expect("segment_sum_none", [&] {
    const dev_var_matrix e = to_dev_var_matrix(v4.data(), 0, 1);
    const size_t nodes = ChainableStack::instance_->var_stack_.size();
    const dev_var_matrix s = segment_sum(e, none);
    const std::vector<double> z = s.val();
    std::string r = shape_of(s) + (ChainableStack::instance_->var_stack_.size() == nodes ? " no node" : " a node");
    for (double e2 : z) r += " " + std::to_string(e2);
    return r;
  });
  recover_memory_nested();
  std::printf("stack|%zu|%zu\n", ChainableStack::instance_->var_stack_.size(),
              ChainableStack::instance_->dev_adj_stack_.size());
}

int main() {
  std::string mode;
  try {
    while (std::cin >> mode) {
      if (mode == "tape") cmd_tape();
      else if (mode == "errors") cmd_errors();
      else if (mode == "bench") cmd_bench();
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
