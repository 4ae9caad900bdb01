#ifndef STAN_MATH_REV_FUN_STUDENT_T_CAUCHY_LPDF_HPP
#define STAN_MATH_REV_FUN_STUDENT_T_CAUCHY_LPDF_HPP

// student_t_lpdf<propto>(y | nu, mu, sigma) and cauchy_lpdf<propto>(y | mu, sigma)
// (prim/scal/prob/student_t_lpdf.hpp, cauchy_lpdf.hpp), each as ONE fused
// device launch (smg_student_t_lpdf_fused / smg_cauchy_lpdf_fused: the two
// specialisations of one kernel) in normal_lpdf's pattern (normal_lpdf.hpp):
// the domain checks, the value and one partial per var operand; the node is
// built with operands_and_partials.
//
// With z = (y - mu) / sigma, q = z^2 / nu, h = nu / 2 the Student-t summands
// are -log sqrt(pi), lgamma(h + 1/2) - lgamma(h) - 1/2 log nu, -log sigma and
// -(h + 1/2) log1p(q), each under its include_summand; the partials are
//   y' = -(nu + 1) z / (sigma nu (1 + q)), mu' = -y',
//   nu' = 1/2 [digamma(h + 1/2) - digamma(h) - 1/nu - log1p(q) + (nu + 1) q / (nu (1 + q))],
//   sigma' = -1/sigma + (nu + 1) q / (sigma (1 + q)).
// Cauchy: -log pi, -log sigma, -log1p(z^2); y' = -2z / (sigma (1 + z^2)),
// mu' = -y', sigma' = (z^2 - 1) / (sigma (1 + z^2)); evaluated through z, so
// |z| = 1e150 stays finite.
//
// Operands as normal_lpdf's: double, var, std::vector / Eigen vectors of
// double | var (host values, staged in pinned memory and read zero-copy),
// dev_data<double> and dev_var_matrix (values and partials stay on the
// device: a device edge).  Below a size gate a call over host operands runs
// the reference's loop on the host.
//
// Semantics kept: an operand of size zero -> 0; check_not_nan(y),
// check_positive_finite(nu), check_finite(mu), check_positive_finite(sigma)
// -- reported in that order, within check_positive_finite "> 0" over the
// whole operand before "finite" -- then check_consistent_sizes; all-double
// propto -> 0 after the checks.

#include <stan/math/prim/special.hpp>
#include <stan/math/rev/fun/normal_lpdf.hpp>

#include <cmath>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <vector>

namespace stan {
namespace math {

namespace internal {

// operand slots of the kernel: y, nu, mu, sigma (Cauchy leaves nu's unused)
static const char* const heavy_tail_names[4] = {"Random variable", "Degrees of freedom parameter",
                                                "Location parameter", "Scale parameter"};

inline bool heavy_tail_fails(int slot, double x) {
  if (slot == 0) return std::isnan(x);
  if (slot == 2) return !(std::fabs(x) <= 1.7976931348623157e308);
  return !(x > 0.0 && x <= 1.7976931348623157e308);
}

/**
 * The reference's domain error for one operand (normal_throw_first's index
 * and scalar forms): slot 0 check_not_nan, 2 check_finite, 1 and 3
 * check_positive_finite, which is check_positive over the whole operand and
 * then check_finite over it.  bits (slots 1 and 3): 1 = some element fails
 * "> 0", 2 = some element is infinite, as the kernel reports them; 3 when
 * unknown.  Returns without throwing when no element fails.
 */
inline void heavy_tail_throw_first(const char* fn, int slot, int bits, const double* v, size_t n, bool vec) {
  auto report = [&](size_t i, const char* must) {
    std::ostringstream m;
    m << fn << ": " << heavy_tail_names[slot];
    if (vec) m << "[" << i + 1 << "]";
    m << " is " << v[i] << ", but must " << must;
    throw std::domain_error(m.str());
  };
  if (slot == 0) {
    for (size_t i = 0; i < n; ++i)
      if (std::isnan(v[i])) report(i, "not be nan!");
  } else if (slot == 2) {
    for (size_t i = 0; i < n; ++i)
      if (!(std::fabs(v[i]) <= 1.7976931348623157e308)) report(i, "be finite!");
  } else {
    if (bits & 1)
      for (size_t i = 0; i < n; ++i)
        if (!(v[i] > 0.0)) report(i, "be > 0!");
    for (size_t i = 0; i < n; ++i)
      if (!(std::fabs(v[i]) <= 1.7976931348623157e308)) report(i, "be finite!");
  }
}

/** check_consistent_sizes over the used slots (normal_check_sizes' message). */
inline void heavy_tail_check_sizes(const char* fn, const fused_operand* ops) {
  size_t expect = 0;
  for (int i = 0; i < 4; ++i)
    if (ops[i].vec && ops[i].n > expect) expect = ops[i].n;
  for (int i = 0; i < 4; ++i)
    if (ops[i].vec && ops[i].n != expect) {
      std::ostringstream m;
      m << fn << ": " << heavy_tail_names[i] << " has dimension = " << ops[i].n << ", expecting dimension = " << expect
        << "; a function was called with arguments of different scalar, array, vector, or "
           "matrix types, and they were not consistently sized;  all arguments must be "
           "scalars or multidimensional values of the same shape.";
      throw std::invalid_argument(m.str());
    }
}

/**
 * Largest element count evaluated on the host, per function (KIND 0
 * student_t_lpdf, 1 cauchy_lpdf): the largest power of two at which the host
 * loop was still the faster by the median ("Heavy-tailed
 * densities").  0 sends every call to the device.
 */
template <int KIND>
inline size_t& heavy_tail_host_max_ref() {
  static size_t v = size_t(2048);  // measured for each function: the same power of two
  return v;
}

template <int I, typename OP>
inline auto& heavy_tail_edge(OP& p) {
  if constexpr (I == 0) return p.edge1_;
  else if constexpr (I == 1) return p.edge2_;
  else if constexpr (I == 2) return p.edge3_;
  else return p.edge4_;
}

/** Where the kernel puts operand Op's partial: the device edge, the staging
 * area (host vector), a non-null marker (scalar var: reduced into res), or
 * nowhere (data). */
template <typename Op, typename Edge>
inline double* heavy_tail_partial_ptr(Edge& e, const fused_operand& o, double* staged, double* marker) {
  if constexpr (!op_is_var<Op>::value) {
    return nullptr;
  } else if constexpr (is_device_operand<Op>::value) {
    return e.partials_;
  } else {
    return o.vec ? staged : marker;
  }
}

template <typename Op, typename Edge>
inline void heavy_tail_partial_take(Edge& e, const fused_operand& o, const double* staged, double reduced) {
  if constexpr (op_is_var<Op>::value && !is_device_operand<Op>::value) {
    if (!o.vec) e.partials_[0] = reduced;
    else fused_take(e, staged, o.n);
  }
}

/**
 * Host evaluation over host operands (small calls): the reference's loop,
 * checks in its order, the value's groups accumulated in element order, the
 * terms of a scalar nu / sigma evaluated once.
 */
template <int KIND, bool propto, typename T_y, typename T_dof, typename T_loc, typename T_scale>
inline typename ops_return<T_y, T_dof, T_loc, T_scale>::type heavy_tail_lpdf_host(const char* fn, const T_y& y,
                                                                                  const T_dof& nu, const T_loc& mu,
                                                                                  const T_scale& sigma,
                                                                                  const fused_operand* ops, size_t N,
                                                                                  int include) {
  constexpr bool vy = op_is_var<T_y>::value, vnu = op_is_var<T_dof>::value, vmu = op_is_var<T_loc>::value,
                 vs = op_is_var<T_scale>::value;
  using ret_t = typename ops_return<T_y, T_dof, T_loc, T_scale>::type;
  auto check = [&](int slot, const auto& x) {
    const fused_operand& o = ops[slot];
    bool bad = false;
    for (size_t i = 0; i < o.n; ++i) bad |= heavy_tail_fails(slot, host_val(x, i));
    if (!bad) return;
    std::vector<double> v(o.n);
    for (size_t i = 0; i < o.n; ++i) v[i] = host_val(x, i);
    heavy_tail_throw_first(fn, slot, 3, v.data(), o.n, o.vec);
  };
  auto check_all = [&] {
    check(0, y);
    if (KIND == 0) check(1, nu);
    check(2, mu);
    check(3, sigma);
  };
  check_all();
  heavy_tail_check_sizes(fn, ops);
  if constexpr (!(vy || vnu || vmu || vs)) {
    if (propto) return ret_t(0.0);
  }
  operands_and_partials<T_y, T_dof, T_loc, T_scale> ops_partials(y, nu, mu, sigma);
  const bool nuvec = ops[1].vec, svec = ops[3].vec;
  // lgamma(h + 1/2) - lgamma(h) - 1/2 log nu and 1/2 [digamma(h + 1/2) - digamma(h) - 1/nu]
  auto nu_value = [](double nv) { return lgamma(0.5 * nv + 0.5) - lgamma(0.5 * nv) - 0.5 * std::log(nv); };
  auto nu_partial = [](double nv) { return 0.5 * (digamma(0.5 * nv + 0.5) - digamma(0.5 * nv) - 1.0 / nv); };
  const double nu0 = KIND == 0 ? host_val(nu, 0) : 1.0, s0 = host_val(sigma, 0);
  const double nu_value0 = (KIND == 0 && (include & 8) && !nuvec) ? nu_value(nu0) : 0.0;
  const double nu_partial0 = (KIND == 0 && vnu && !nuvec) ? nu_partial(nu0) : 0.0;
  const double log_s0 = ((include & 2) && !svec) ? std::log(s0) : 0.0;
  double sum_log1p = 0.0, sum_log_s = 0.0, sum_nu = 0.0;
  for (size_t n = 0; n < N; ++n) {
    const double yv = host_val(y, n), mv = host_val(mu, n), sv = host_val(sigma, n);
    const double nv = KIND == 0 ? host_val(nu, n) : 1.0;
    const double inv_s = 1.0 / sv;
    const double z = (yv - mv) * inv_s;
    const double z2 = z * z;
    const double q = KIND == 0 ? z2 / nv : z2;
    const double l = std::log1p(q);
    const double w = KIND == 0 ? (nv + 1.0) / nv : 2.0;
    const double t = w / (1.0 + q);
    sum_log1p += (KIND == 0 ? 0.5 * nv + 0.5 : 1.0) * l;
    if (svec && (include & 2)) sum_log_s += std::log(sv);
    if (KIND == 0 && nuvec && (include & 8)) sum_nu += nu_value(nv);
    const double sc = t * z * inv_s;
    if constexpr (vy) ops_partials.edge1_.partials_[int(n)] -= sc;
    if constexpr (vnu)
      ops_partials.edge2_.partials_[int(n)] += 0.5 * (t * q - l) + (nuvec ? nu_partial(nv) : nu_partial0);
    if constexpr (vmu) ops_partials.edge3_.partials_[int(n)] += sc;
    if constexpr (vs) ops_partials.edge4_.partials_[int(n)] += -inv_s + t * z2 * inv_s;
  }
  double logp = 0.0;
  if (include & 1) logp += (KIND == 0 ? -0.57236494292470008707 : -1.1447298858494001741) * double(N);
  if (KIND == 0 && (include & 8)) logp += nuvec ? sum_nu : nu_value0 * double(N);
  if (include & 2) logp -= svec ? sum_log_s : log_s0 * double(N);
  if (include & 4) logp -= sum_log1p;
  if constexpr (vy || vnu || vmu || vs) {
    return ops_partials.build(logp);
  } else {
    return logp;
  }
}

/** Both densities: KIND 0 student_t_lpdf, 1 cauchy_lpdf (nu: the double 1). */
template <int KIND, bool propto, typename T_y, typename T_dof, typename T_loc, typename T_scale>
inline typename ops_return<T_y, T_dof, T_loc, T_scale>::type heavy_tail_lpdf(const T_y& y, const T_dof& nu,
                                                                             const T_loc& mu, const T_scale& sigma) {
  static const char* fn = KIND == 0 ? "student_t_lpdf" : "cauchy_lpdf";
  constexpr bool vy = op_is_var<T_y>::value, vnu = op_is_var<T_dof>::value, vmu = op_is_var<T_loc>::value,
                 vs = op_is_var<T_scale>::value;
  using ret_t = typename ops_return<T_y, T_dof, T_loc, T_scale>::type;
  fused_operand ops[4] = {fused_of(y), fused_of(nu), fused_of(mu), fused_of(sigma)};
  for (auto& o : ops)
    if (o.vec && o.n == 0) return ret_t(0.0);
  // include_summand<propto, ...>
  const int include = (!propto ? 1 : 0) | ((!propto || vs) ? 2 : 0) | ((!propto || vy || vnu || vmu || vs) ? 4 : 0)
                      | ((KIND == 0 && (!propto || vnu)) ? 8 : 0);
  size_t N = 1;
  bool sizes_ok = true;
  for (auto& o : ops)
    if (o.vec) N = o.n > N ? o.n : N;
  for (auto& o : ops)
    if (o.vec && o.n != N) sizes_ok = false;

  if constexpr (!is_device_operand<T_y>::value && !is_device_operand<T_dof>::value
                && !is_device_operand<T_loc>::value && !is_device_operand<T_scale>::value) {
    if (N <= heavy_tail_host_max_ref<KIND>())
      return heavy_tail_lpdf_host<KIND, propto>(fn, y, nu, mu, sigma, ops, N, include);
  }

  smg_ctx* c = amd::ctx();
  // pinned staging: [res(9), 7 spare | host values of y, nu, mu, sigma | host partials of the same]
  size_t off = 16, val_off[4], g_off[4];
  for (int i = 0; i < 4; ++i) {
    val_off[i] = off;
    if (ops[i].host && ops[i].vec) off += ops[i].n;
  }
  const bool want_g[4] = {vy, vnu, vmu, vs};
  for (int i = 0; i < 4; ++i) {
    g_off[i] = off;
    if (want_g[i] && ops[i].vec && ops[i].host) off += ops[i].n;
  }
  double* st = static_cast<double*>(smg_pinned_result(c, off * sizeof(double)));
  if (!st) throw std::bad_alloc();
  for (int i = 0; i < 16; ++i) st[i] = 0.0;
  fused_stage(y, st + val_off[0]);
  fused_stage(nu, st + val_off[1]);
  fused_stage(mu, st + val_off[2]);
  fused_stage(sigma, st + val_off[3]);
  const double* vals[4];  // vector operands; NULL: the scalar value (a kernel argument)
  for (int i = 0; i < 4; ++i) vals[i] = !ops[i].vec ? nullptr : (ops[i].host ? st + val_off[i] : ops[i].dev);
  operands_and_partials<T_y, T_dof, T_loc, T_scale> ops_partials(y, nu, mu, sigma);
  // partial outputs: host vectors -> staging, device vars -> the device edge,
  // scalars -> reduced into res[5 + i]
  double* g[4] = {heavy_tail_partial_ptr<T_y>(ops_partials.edge1_, ops[0], st + g_off[0], st + 9),
                  heavy_tail_partial_ptr<T_dof>(ops_partials.edge2_, ops[1], st + g_off[1], st + 9),
                  heavy_tail_partial_ptr<T_loc>(ops_partials.edge3_, ops[2], st + g_off[2], st + 9),
                  heavy_tail_partial_ptr<T_scale>(ops_partials.edge4_, ops[3], st + g_off[3], st + 9)};
  if (sizes_ok) {
    if (KIND == 0)
      amd::check(smg_student_t_lpdf_fused(c, vals[0], vals[1], vals[2], vals[3], ops[0].scalar, ops[1].scalar,
                                          ops[2].scalar, ops[3].scalar, (long long)N, include, st, g[0], g[1], g[2],
                                          g[3]),
                 fn);
    else
      amd::check(smg_cauchy_lpdf_fused(c, vals[0], vals[2], vals[3], ops[0].scalar, ops[2].scalar, ops[3].scalar,
                                       (long long)N, include, st, g[0], g[2], g[3]),
                 fn);
  } else {
    // error path: the domain checks over each operand's own length, in order
    static const int kinds[4] = {0, 3, 1, 3};  // smg_check_domain's
    for (int i = 0; i < 4; ++i) {
      if (KIND == 1 && i == 1) continue;
      if (vals[i]) amd::check(smg_check_domain(c, vals[i], (long long)ops[i].n, kinds[i], st + 1 + i), fn);
      else st[1 + i] = heavy_tail_fails(i, ops[i].scalar) ? 1.0 : 0.0;
    }
    amd::check(smg_sync(c), fn);
    for (int i = 0; i < 4; ++i)
      if (st[1 + i] != 0.0) st[1 + i] = 3.0;  // which of check_positive_finite's two failures: not known here
  }
  for (int i = 0; i < 4; ++i) {
    if (st[1 + i] == 0.0) continue;
    // error path: the operand's values on the host, the first offending one reported
    std::vector<double> hv(ops[i].vec ? ops[i].n : 1);
    if (!ops[i].vec) hv[0] = ops[i].scalar;
    else if (ops[i].host) std::memcpy(hv.data(), st + val_off[i], ops[i].n * sizeof(double));
    else amd::to_host(hv.data(), ops[i].dev, ops[i].n);
    heavy_tail_throw_first(fn, i, int(st[1 + i]), hv.data(), hv.size(), ops[i].vec);
  }
  heavy_tail_check_sizes(fn, ops);
  const double logp = st[0];
  if constexpr (vy || vnu || vmu || vs) {
    heavy_tail_partial_take<T_y>(ops_partials.edge1_, ops[0], st + g_off[0], st[5]);
    heavy_tail_partial_take<T_dof>(ops_partials.edge2_, ops[1], st + g_off[1], st[6]);
    heavy_tail_partial_take<T_loc>(ops_partials.edge3_, ops[2], st + g_off[2], st[7]);
    heavy_tail_partial_take<T_scale>(ops_partials.edge4_, ops[3], st + g_off[3], st[8]);
    return ops_partials.build(logp);
  } else {
    return propto ? 0.0 : logp;
  }
}

}  // namespace internal

namespace amd {
/** Set the student_t_lpdf host gate (elements); 0 sends every call to the device. */
inline void set_student_t_host_max(size_t n) { internal::heavy_tail_host_max_ref<0>() = n; }
/** Set the cauchy_lpdf host gate (elements); 0 sends every call to the device. */
inline void set_cauchy_host_max(size_t n) { internal::heavy_tail_host_max_ref<1>() = n; }
}  // namespace amd

template <bool propto, typename T_y, typename T_dof, typename T_loc, typename T_scale>
inline typename internal::ops_return<T_y, T_dof, T_loc, T_scale>::type student_t_lpdf(const T_y& y, const T_dof& nu,
                                                                                      const T_loc& mu,
                                                                                      const T_scale& sigma) {
  return internal::heavy_tail_lpdf<0, propto>(y, nu, mu, sigma);
}

template <typename T_y, typename T_dof, typename T_loc, typename T_scale>
inline auto student_t_lpdf(const T_y& y, const T_dof& nu, const T_loc& mu, const T_scale& sigma) {
  return student_t_lpdf<false>(y, nu, mu, sigma);
}

template <bool propto, typename T_y, typename T_loc, typename T_scale>
inline typename internal::ops_return<T_y, T_loc, T_scale>::type cauchy_lpdf(const T_y& y, const T_loc& mu,
                                                                            const T_scale& sigma) {
  return internal::heavy_tail_lpdf<1, propto>(y, 1.0, mu, sigma);
}

template <typename T_y, typename T_loc, typename T_scale>
inline auto cauchy_lpdf(const T_y& y, const T_loc& mu, const T_scale& sigma) {
  return cauchy_lpdf<false>(y, mu, sigma);
}

}  // namespace math
}  // namespace stan
#endif
