// The host gates of student_t_lpdf and cauchy_lpdf: one gradient over host
// vectors (y data, mu a std::vector<var>, nu and sigma vars) through the host
// loop (gate above n) and through the device call (gate 0), at n = 2^8 ..
// 2^18, median of 21 timings of `reps` gradients each.  A function's default
// gate is the largest power of two at which the host loop is still the faster
// by the median (DESIGN.md "Heavy-tailed densities" holds the table).
//   g++ -O2 -std=c++17 -Imath_amd/include -Iinclude -isystem <eigen>
//   tools/time_heavy_tail_gate.cpp -Lmath_amd/lib -lsmg_hip -Wl,-rpath,<abs>/math_amd/lib
#include <stan/math.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>

using namespace stan::math;

static double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <int K>
static double median_us(const std::vector<double>& y, const std::vector<double>& th, int reps) {
  const size_t n = y.size();
  auto f = [&](const std::vector<var>& t) {
    const std::vector<var> mu(t.begin(), t.begin() + long(n));
    if constexpr (K == 0) return student_t_lpdf(y, t[n + 1], mu, t[n]);
    else return cauchy_lpdf(y, mu, t[n]);
  };
  double fx;
  std::vector<double> g, times;
  for (int r = 0; r < 3; ++r) gradient(f, th, fx, g);
  for (int round = 0; round < 21; ++round) {
    const double t0 = now();
    for (int r = 0; r < reps; ++r) gradient(f, th, fx, g);
    times.push_back((now() - t0) / reps * 1e6);
  }
  std::sort(times.begin(), times.end());
  return times[10];
}

int main() {
  for (int e = 8; e <= 18; ++e) {
    const size_t n = size_t(1) << e;
    std::vector<double> y(n), th(n + 2);
    for (size_t i = 0; i < n; ++i) {
      th[i] = 0.001 * double(i % 977) - 0.4;
      y[i] = th[i] + 1.3 * std::tan(3.0 * (double((i * 7919) % 1000) / 1000.0 - 0.5));
    }
    th[n] = 1.3;
    th[n + 1] = 4.5;
    const int reps = e <= 12 ? 200 : (e <= 15 ? 40 : 8);
    double us[2][2];
    for (int dev = 0; dev < 2; ++dev) {
      amd::set_student_t_host_max(dev ? 0 : n + 1);
      amd::set_cauchy_host_max(dev ? 0 : n + 1);
      us[0][dev] = median_us<0>(y, th, reps);
      us[1][dev] = median_us<1>(y, th, reps);
    }
    std::printf("n=2^%-2d student_t host %9.2f us  device %9.2f us   cauchy host %9.2f us  device %9.2f us\n", e,
                us[0][0], us[0][1], us[1][0], us[1][1]);
    std::fflush(stdout);
  }
  return 0;
}
