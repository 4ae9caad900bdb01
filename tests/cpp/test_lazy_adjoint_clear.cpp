// Large device adjoints are zeroed when their first dense user appears
// (rev/core/grad.hpp clear_device_adjoint), driven by
// tests/test_lazy_adjoint_clear.py.  Commands on stdin:
//   unread N reps x y theta    the GP closed-form gradient through gradient(),
//                              the arena NaN-poisoned before every evaluation:
//                              "unread_r fx g0 g1 g2 zeroed_bytes"
//   read N variant x y theta   the same model with its intermediate adjoints
//                              read after the sweep (variant 0) or with a
//                              second writer of L's adjoint (variant 1):
//                              "theta lp g0 g1 g2", "K|Kd|L sum abs_sum l2
//                              samples...", "zeroed bytes"
//   mulchol N reps             sum(cholesky_decompose(A)), A a device leaf:
//                              "mulchol_r f sum abs_sum l2 samples...",
//                              "zeroed_r bytes"
//   setzero N x y theta        grad(), set_zero_all_adjoints(), grad() again:
//                              "first lp g..." and "second lp g..."
#include <stan/math.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

using namespace stan::math;

static std::vector<double> read_vec(size_t n) {
  std::vector<double> v(n);
  std::string t;
  for (auto& x : v) {
    std::cin >> t;
    x = std::strtod(t.c_str(), nullptr);
  }
  return v;
}

// sum, sum of magnitudes, L2 norm and 64 evenly spaced entries
static void print_stats(const std::string& tag, double head, const std::vector<double>& v) {
  double s = 0, a = 0, q = 0;
  for (double x : v) {
    s += x;
    a += std::fabs(x);
    q += x * x;
  }
  std::printf("%s %.17g %.17g %.17g %.17g", tag.c_str(), head, s, a, std::sqrt(q));
  const size_t step = v.size() / 64 ? v.size() / 64 : 1;
  for (size_t i = 0, k = 0; k < 64 && i < v.size(); i += step, ++k) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

// every byte the next evaluation's arena allocations can land on becomes a NaN
static void poison_arena(int N) {
  start_nested();
  const size_t span = size_t(16) * N * N + (size_t(1) << 20);
  double* p = amd::alloc_doubles(span);
  amd::check(smg_memset(amd::ctx(), p, 0xFF, span * sizeof(double)), "poison");
  amd::check(smg_sync(amd::ctx()), "poison");
  recover_memory_nested();
}

static void reset_zeroed() { amd::check(smg_profile_enable(amd::ctx(), 0), "reset"); }
static unsigned long long zeroed() {
  amd::check(smg_sync_all(amd::ctx()), "zeroed");
  return smg_zeroed_bytes(amd::ctx());
}

struct gp_functor {
  const dev_data<double>& x;
  const dev_data<double>& y;
  const dev_data<double>& mu0;
  template <typename T>
  T operator()(const std::vector<T>& th) const {
    auto K = gp_exp_quad_cov(x, th[0], th[1]);
    auto Kd = add_diag(K, square(th[2]));
    auto L = cholesky_decompose(Kd);
    return multi_normal_cholesky_lpdf(y, mu0, L);
  }
};

static void cmd_unread() {
  int N, reps;
  std::cin >> N >> reps;
  const std::vector<double> x = read_vec(N), y = read_vec(N), th = read_vec(3);
  const dev_data<double> xd = to_dev_data(x), yd = to_dev_data(y), mu0 = to_dev_data(std::vector<double>(N, 0.0));
  for (int r = 0; r < reps; ++r) {
    poison_arena(N);
    reset_zeroed();
    double fx = 0;
    std::vector<double> g;
    gradient(gp_functor{xd, yd, mu0}, th, fx, g);
    std::printf("unread_%d %.17g %.17g %.17g %.17g %llu\n", r, fx, g[0], g[1], g[2], zeroed());
  }
}

static void cmd_read() {
  int N, variant;
  std::cin >> N >> variant;
  const std::vector<double> x = read_vec(N), y = read_vec(N), th = read_vec(3);
  const dev_data<double> xd = to_dev_data(x), yd = to_dev_data(y), mu0 = to_dev_data(std::vector<double>(N, 0.0));
  poison_arena(N);
  reset_zeroed();
  start_nested();
  std::vector<var> tv(th.begin(), th.end());
  dev_var_matrix K = gp_exp_quad_cov(xd, tv[0], tv[1]);
  dev_var_matrix Kd = add_diag(K, square(tv[2]));
  dev_var_matrix L = cholesky_decompose(Kd);
  var lp = multi_normal_cholesky_lpdf(yd, mu0, L);
  if (variant == 1) lp = lp + 0.25 * sum(L);
  lp.grad();
  std::printf("theta %.17g %.17g %.17g %.17g\n", lp.val(), tv[0].adj(), tv[1].adj(), tv[2].adj());
  print_stats("K", 0.0, K.adj());
  print_stats("Kd", 0.0, Kd.adj());
  print_stats("L", 0.0, L.adj());
  std::printf("zeroed %llu\n", zeroed());
  recover_memory_nested();
}

static void cmd_mulchol() {
  int N, reps;
  std::cin >> N >> reps;
  std::vector<double> a(size_t(N) * N);
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i) a[size_t(j) * N + i] = (i == j ? double(N) : 0.0) + std::cos(0.37 * (i + j));
  for (int r = 0; r < reps; ++r) {
    poison_arena(N);
    reset_zeroed();
    start_nested();
    dev_var_matrix A = to_dev_var_matrix(a.data(), N, N);
    var f = sum(cholesky_decompose(A));
    f.grad();
    print_stats("mulchol_" + std::to_string(r), f.val(), A.adj());
    std::printf("zeroed_%d %llu\n", r, zeroed());
    recover_memory_nested();
  }
}

static void cmd_setzero() {
  int N;
  std::cin >> N;
  const std::vector<double> x = read_vec(N), y = read_vec(N), th = read_vec(3);
  const dev_data<double> xd = to_dev_data(x), yd = to_dev_data(y), mu0 = to_dev_data(std::vector<double>(N, 0.0));
  poison_arena(N);
  std::vector<var> tv(th.begin(), th.end());
  var lp = gp_functor{xd, yd, mu0}(tv);
  lp.grad();
  std::printf("first %.17g %.17g %.17g %.17g\n", lp.val(), tv[0].adj(), tv[1].adj(), tv[2].adj());
  set_zero_all_adjoints();
  lp.grad();
  std::printf("second %.17g %.17g %.17g %.17g\n", lp.val(), tv[0].adj(), tv[1].adj(), tv[2].adj());
  recover_memory();
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "unread") cmd_unread();
    else if (cmd == "read") cmd_read();
    else if (cmd == "mulchol") cmd_mulchol();
    else if (cmd == "setzero") cmd_setzero();
    else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
    std::fflush(stdout);
  }
  return 0;
}
