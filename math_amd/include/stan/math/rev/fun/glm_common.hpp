#ifndef STAN_MATH_REV_FUN_GLM_COMMON_HPP
#define STAN_MATH_REV_FUN_GLM_COMMON_HPP

// What the GLM log-density headers (bernoulli_logit, poisson_log, normal_id,
// neg_binomial_2_log, categorical_logit, ordered_logistic) share on the host:
// the row shard and its partition, the operands (alpha a scalar or one
// intercept per row, beta on the host or the device), the reference's size and
// finiteness messages, the error-path scan of a device y, and the tape nodes.
// Each likelihood's header keeps what is its own: buffer layout, entry call,
// propto rules, the composition of lp and the packing of the gradient.

#include <stan/math/amd/comm.hpp>
#include <stan/math/amd/matrix.hpp>
#include <stan/math/rev/core.hpp>
#include <stan/math/rev/fun/normal_lpdf.hpp>

#include <cmath>
#include <limits>
#include <new>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace stan {
namespace math {

/** Device-resident GLM data: a row block [row0, row0 + rows) of y and x.
 * x: rows x M column-major with leading dimension ldx (ldx >= rows). */
struct glm_shard {
  const int* y = nullptr;
  const double* yd = nullptr;  // real-valued y (normal_id_glm_lpdf)
  const double* x = nullptr;
  long long rows = 0;
  int M = 0;
  long long ldx = 0;
  long long row0 = 0;      // first global row (bookkeeping)
  long long total_rows = 0;
  bool distributed = false;  // all-reduce across the communicator
};

/** Contiguous row partition used by every sharded reducer: rank r of W owns
 * rows [r*R/W, (r+1)*R/W) (integer division), so the blocks tile [0, R). */
inline void row_partition(long long R, int world, int rank, long long* begin, long long* end) {
  *begin = R * rank / world;
  *end = R * (rank + 1) / world;
}

namespace internal {

// ---- sizes, and the device / host forms of (y, x)
// check_consistent_size's message (prim/scal/err/check_consistent_size.hpp)
[[noreturn]] inline void glm_size_mismatch(const char* fn, const char* name, long long got, long long want) {
  std::ostringstream m;
  m << fn << ": " << name << " has dimension = " << got << ", expecting dimension = " << want
    << "; a function was called with arguments of different scalar, array, vector, or matrix "
       "types, and they were not consistently sized;  all arguments must be scalars or "
       "multidimensional values of the same shape.";
  throw std::invalid_argument(m.str());
}

/** The whole of device-resident (y, x) as one shard, y of int or of double,
 * after the consistent-size check of y. */
template <typename T_y>
inline glm_shard glm_shard_of(const char* fn, const dev_data<T_y>& y, const dev_data<double>& x) {
  if ((long long)y.size() != (long long)x.rows())
    glm_size_mismatch(fn, "Vector of dependent variables", (long long)y.size(), x.rows());
  glm_shard s;
  if constexpr (std::is_same<T_y, int>::value) s.y = y.data();
  else s.yd = y.data();
  s.x = x.data();
  s.rows = x.rows();
  s.M = x.cols();
  s.ldx = x.rows();
  s.total_rows = s.rows;
  return s;
}

/** Host (y, x column-major with M columns) uploaded for one call, y first. */
template <typename T_y>
struct glm_uploaded {
  dev_data<T_y> y;
  dev_data<double> x;
};
template <typename T_y>
inline glm_uploaded<T_y> glm_upload(const char* fn, const std::vector<T_y>& y, const std::vector<double>& x_colmajor,
                                    int M) {
  const int R = int(y.size());
  if ((long long)x_colmajor.size() != (long long)R * M)
    throw std::invalid_argument(std::string(fn) + ": x must hold y.size() * M values");
  return {to_dev_data(y), to_dev_data(x_colmajor.data(), x_colmajor.size(), R, M)};
}

// ---- the first offending y, for check_bounded / check_nonnegative's messages
struct glm_int_hit {
  long long index = -1;  // within y; -1: none
  int value = 0;
};
/** The first of the device ints y[0, n) outside [lo, hi].  Error path only:
 * host copies in chunks through the context's scratch, one sync each. */
inline glm_int_hit glm_first_int_outside(const char* fn, const int* y, long long n, int lo, int hi) {
  smg_ctx* c = amd::ctx();
  const long long chunk = 1 << 20;
  for (long long i0 = 0; i0 < n; i0 += chunk) {
    const long long k = n - i0 < chunk ? n - i0 : chunk;
    int* stage = static_cast<int*>(smg_host_scratch(c, size_t(k) * sizeof(int)));
    if (!stage) throw std::bad_alloc();
    amd::check(smg_memcpy_d2h(c, stage, y + i0, size_t(k) * sizeof(int)), fn);
    amd::check(smg_sync(c), fn);
    for (long long i = 0; i < k; ++i)
      if (stage[i] < lo || stage[i] > hi) return {i0 + i, stage[i]};
  }
  return {};
}

// The three throwers below name the element by its global index (row0 = the
// shard's first row).  A rank whose own rows are all in range (the flag came
// from another rank's shard) names no element.
// check_bounded(fn, "Vector of dependent variables", y, lo, hi)
// (prim/scal/err/check_bounded.hpp:40-50)
[[noreturn]] inline void glm_throw_y_bounds(const char* fn, const int* y, long long n, int lo, int hi,
                                            long long row0) {
  const glm_int_hit f = glm_first_int_outside(fn, y, n, lo, hi);
  std::ostringstream m;
  if (f.index >= 0)
    m << fn << ": Vector of dependent variables[" << row0 + f.index + 1 << "] is " << f.value
      << ", but must be in the interval [" << lo << ", " << hi << "]";
  else
    m << fn << ": Vector of dependent variables is out of bounds (on another rank's rows), but must be in "
            "the interval [" << lo << ", " << hi << "]";
  throw std::domain_error(m.str());
}

// check_nonnegative(fn, name, y); `name`: the reference's name of y (poisson's by default)
[[noreturn]] inline void glm_throw_negative_y(const char* fn, const int* y, long long n, long long row0 = 0,
                                              const char* name = "Vector of dependent variables") {
  const glm_int_hit f = glm_first_int_outside(fn, y, n, 0, std::numeric_limits<int>::max());
  if (f.index < 0)
    throw std::domain_error(std::string(fn) + ": " + name + " is negative (on another rank's rows), but must be >= 0!");
  std::ostringstream m;
  m << fn << ": " << name << "[" << row0 + f.index + 1 << "] is " << f.value << ", but must be >= 0!";
  throw std::domain_error(m.str());
}

// check_bounded(fn, "categorical outcome out of support", y, lo, hi)
[[noreturn]] inline void glm_throw_out_of_support(const char* fn, const int* y, long long n, int lo, int hi,
                                                  long long row0 = 0) {
  const glm_int_hit f = glm_first_int_outside(fn, y, n, lo, hi);
  std::ostringstream m;
  if (f.index >= 0)
    m << fn << ": categorical outcome out of support[" << row0 + f.index + 1 << "] is " << f.value
      << ", but must be in the interval [" << lo << ", " << hi << "]";
  else
    m << fn << ": categorical outcome out of support (on another rank's rows), but must be in the interval ["
      << lo << ", " << hi << "]";
  throw std::domain_error(m.str());
}

// check_finite on a device matrix (column-major, ld): the first non-finite
// entry by linear index (error path only: host copy column by column)
inline void glm_check_finite_dev(const char* fn, const char* name, const double* d, long long rows,
                                 long long cols, long long ld) {
  std::vector<double> h(size_t(rows > 0 ? rows : 0));
  for (long long j = 0; j < cols; ++j) {
    if (rows > 0) amd::to_host(h.data(), d + j * ld, size_t(rows));
    for (long long i = 0; i < rows; ++i)
      if (!std::isfinite(h[size_t(i)])) {
        std::ostringstream m;
        m << fn << ": " << name << "[" << j * rows + i + 1 << "] is " << h[size_t(i)] << ", but must be finite!";
        throw std::domain_error(m.str());
      }
  }
}

// check_positive_finite(fn, name, v): a scale or a precision
inline void glm_check_positive_finite(const char* fn, const char* name, double v) {
  if (v > 0 && std::isfinite(v)) return;
  std::ostringstream m;
  m << fn << ": " << name << " is " << v << (v > 0 ? ", but must be finite!" : ", but must be > 0!");
  throw std::domain_error(m.str());
}

// ---- the operands
struct glm_params {
  double alpha = 0;
  vari* alpha_vi = nullptr;
  std::vector<double> beta;       // host values (for upload and the finite check)
  vari** beta_vi = nullptr;       // host beta varis
  dev_matrix_vari* beta_dev = nullptr;
  // one intercept per row (T_alpha a vector; alpha and alpha_vi are then unused)
  bool alpha_vec = false;
  long long alpha_n = 0;
  std::vector<double> alpha_h;           // host values (host vectors)
  vari** alpha_vis = nullptr;            // host varis (std::vector<var>)
  dev_matrix_vari* alpha_dev = nullptr;  // device vars (dev_var_matrix, R x 1 or 1 x R)
  const double* alpha_d = nullptr;       // device data (dev_data<double>)
  int alpha_rows = 0, alpha_cols = 1;    // a device vector's shape (a column or a row)
  bool any_var() const { return alpha_vi || alpha_vis || alpha_dev || beta_vi || beta_dev; }
};

inline void glm_alpha(glm_params& p, double a) { p.alpha = a; }
inline void glm_alpha(glm_params& p, const var& a) {
  p.alpha = a.val();
  p.alpha_vi = a.vi_;
}
inline void glm_alpha(glm_params& p, const std::vector<double>& a) {
  p.alpha_vec = true;
  p.alpha_n = (long long)a.size();
  p.alpha_h = a;
}
inline void glm_alpha(glm_params& p, const std::vector<var>& a) {
  p.alpha_vec = true;
  p.alpha_n = (long long)a.size();
  p.alpha_h.resize(a.size());
  p.alpha_vis = ChainableStack::instance_->memalloc_.alloc_array<vari*>(a.size() ? a.size() : 1);
  for (size_t i = 0; i < a.size(); ++i) {
    p.alpha_h[i] = a[i].val();
    p.alpha_vis[i] = a[i].vi_;
  }
}
inline void glm_alpha(glm_params& p, const dev_data<double>& a) {
  p.alpha_vec = true;
  p.alpha_n = (long long)a.size();
  p.alpha_d = a.data();
}
inline void glm_alpha(glm_params& p, const dev_var_matrix& a) {
  p.alpha_vec = true;
  if (!a.vi_) return;  // a default-constructed matrix: the empty vector
  p.alpha_n = (long long)a.size();
  p.alpha_rows = a.rows();
  p.alpha_cols = a.cols();
  p.alpha_dev = a.vi_;
}
inline void glm_beta(glm_params& p, const std::vector<double>& b) { p.beta = b; }
inline void glm_beta(glm_params& p, const std::vector<var>& b) {
  p.beta.resize(b.size());
  p.beta_vi = ChainableStack::instance_->memalloc_.alloc_array<vari*>(b.size() ? b.size() : 1);
  for (size_t j = 0; j < b.size(); ++j) {
    p.beta[j] = b[j].val();
    p.beta_vi[j] = b[j].vi_;
  }
}
inline void glm_beta(glm_params& p, const dev_var_matrix& b) {
  p.beta = b.val();
  p.beta_dev = b.vi_;
}

// a scalar scale or precision
inline double glm_sigma_val(double s) { return s; }
inline double glm_sigma_val(const var& s) { return s.val(); }
inline vari* glm_sigma_vi(double) { return nullptr; }
inline vari* glm_sigma_vi(const var& s) { return s.vi_; }

template <typename T>
struct glm_is_var
    : std::integral_constant<bool, !std::is_same<T, double>::value &&
                                       !std::is_same<T, std::vector<double>>::value &&
                                       !std::is_same<T, dev_data<double>>::value> {};

struct glm_result {
  double lp = 0.0;
  vari* node = nullptr;  // null: constant result
};

/** What an overload returns: a var over the result's node (or its constant)
 * when an operand holds vars, the plain double otherwise. */
template <bool IsVar>
inline typename std::conditional<IsVar, var, double>::type glm_return(const glm_result& r) {
  if constexpr (IsVar) {
    if (r.node) return var(r.node);
    return var(r.lp);
  } else {
    return r.lp;
  }
}

// ---- one intercept per row (smg_glm_vec_intercept), shared by the four GLMs
// check_consistent_size(fn, "Vector of intercepts", alpha, rows): a shard's
// vector is shard-local
inline void glm_check_alpha_size(const char* fn, const glm_params& p, long long rows) {
  if (!p.alpha_vec) return;
  if (p.alpha_dev && p.alpha_rows != 1 && p.alpha_cols != 1) {
    std::ostringstream m;
    m << fn << ": Vector of intercepts must be a column or a row vector, but is " << p.alpha_rows << " x "
      << p.alpha_cols;
    throw std::invalid_argument(m.str());
  }
  if (p.alpha_n != rows) glm_size_mismatch(fn, "Vector of intercepts", p.alpha_n, rows);
}

/** The device side of a vector intercept: av its values (a host vector's are
 * uploaded, a device vector's read in place), thp the rows' theta' when alpha
 * holds vars (null: data).  A scalar intercept gives nulls. */
struct glm_vec_alpha {
  const double* av = nullptr;
  double* thp = nullptr;
};
inline glm_vec_alpha glm_vec_alpha_prepare(const glm_params& p, long long rows) {
  glm_vec_alpha a;
  if (!p.alpha_vec) return a;
  const size_t n = size_t(rows > 0 ? rows : 1);
  if (p.alpha_dev) {
    a.av = p.alpha_dev->val();
  } else if (p.alpha_d) {
    a.av = p.alpha_d;
  } else {
    double* d = amd::alloc_doubles(n);
    if (rows > 0) amd::to_device(d, p.alpha_h.data(), size_t(rows));
    a.av = d;
  }
  if (p.alpha_vis || p.alpha_dev) a.thp = amd::alloc_doubles(n);
  return a;
}

// check_finite(fn, "Intercept", alpha) for a vector alpha: the first offender,
// 1-based (a device vector is downloaded here, on the error path only)
inline void glm_throw_nonfinite_alpha_vec(const char* fn, const glm_params& p, const glm_vec_alpha& a) {
  if (!p.alpha_vec) return;
  std::vector<double> h = p.alpha_h;
  if (h.empty() && p.alpha_n > 0) {
    h.resize(size_t(p.alpha_n));
    amd::to_host(h.data(), a.av, h.size());
  }
  for (size_t i = 0; i < h.size(); ++i)
    if (!std::isfinite(h[i])) {
      std::ostringstream m;
      m << fn << ": Intercept[" << i + 1 << "] is " << h[i] << ", but must be finite!";
      throw std::domain_error(m.str());
    }
}

// ---- a non-finite result: check_finite on beta ("Weight vector"), then on
// alpha ("Intercept", scalar or per row); returns when all are finite (a
// likelihood without an intercept leaves p's at its default 0)
inline void glm_throw_nonfinite_operands(const char* fn, const glm_params& p, const glm_vec_alpha& va) {
  for (size_t j = 0; j < p.beta.size(); ++j)
    if (!std::isfinite(p.beta[j])) {
      std::ostringstream m;
      m << fn << ": Weight vector[" << j + 1 << "] is " << p.beta[j] << ", but must be finite!";
      throw std::domain_error(m.str());
    }
  if (!std::isfinite(p.alpha)) {
    std::ostringstream m;
    m << fn << ": Intercept is " << p.alpha << ", but must be finite!";
    throw std::domain_error(m.str());
  }
  glm_throw_nonfinite_alpha_vec(fn, p, va);
}
// ... then the linear predictor, under the name of x
[[noreturn]] inline void glm_throw_nonfinite_x(const char* fn) {
  throw std::domain_error(std::string(fn) + ": Matrix of independent variables is not finite, but must be finite!");
}

// ---- the tape nodes
/** One node over (alpha, beta, [sigma | phi]), alpha a scalar: partials
 * g = [alpha', beta'(M), extra'] on the host (arena), beta' also on the device
 * for device-resident beta. */
class glm_dev_vari : public local_adjoint_vari {
 public:
  vari* alpha_vi_;
  vari** beta_vi_;             // host varis of beta (null when beta is data / on device)
  dev_matrix_vari* beta_dev_;  // device beta vars
  vari* extra_vi_;             // sigma or phi (null: none, or data)
  double* g_;
  const double* g_dev_;        // beta' on device
  int M_;
  const char* fn_;
  glm_dev_vari(double lp, vari* a, vari** b, dev_matrix_vari* bd, vari* ex, double* g, const double* gd, int M,
               const char* fn)
      : local_adjoint_vari(lp), alpha_vi_(a), beta_vi_(b), beta_dev_(bd), extra_vi_(ex), g_(g), g_dev_(gd), M_(M),
        fn_(fn) {}
  bool touches_adjoints_in(const vari* lo, const vari* hi) const override {
    auto in = [&](const vari* v) { return v && v >= lo && v < hi; };
    if (in(alpha_vi_) || in(extra_vi_)) return true;
    if (beta_vi_)
      for (int j = 0; j < M_; ++j)
        if (in(beta_vi_[j])) return true;
    return false;
  }
  void chain() override {
    if (alpha_vi_) alpha_vi_->adj_ += adj_ * g_[0];
    if (beta_vi_)
      for (int j = 0; j < M_; ++j) beta_vi_[j]->adj_ += adj_ * g_[1 + j];
    if (beta_dev_) amd::check(smg_axpy(amd::ctx(), M_, adj_, g_dev_, 1, beta_dev_->adj(), 1), fn_);
    if (extra_vi_) extra_vi_->adj_ += adj_ * g_[M_ + 1];
  }
};

/** One node over (alpha(R), beta, [sigma | phi]): alpha' = theta' per row, on
 * the host (arena) for host vars or on the device for a device vector (one
 * axpy into its adjoint); g = [-, beta'(M), extra'] on the host, beta' also on
 * the device for device-resident beta. */
class glm_vec_dev_vari : public local_adjoint_vari {
 public:
  vari** alpha_vis_;
  dev_matrix_vari* alpha_dev_;
  long long R_;
  const double* th_;      // theta' on the host (alpha_vis_)
  const double* th_dev_;  // theta' on the device (alpha_dev_)
  const vari* alo_;       // the address range of alpha's host varis
  const vari* ahi_;
  vari** beta_vi_;
  dev_matrix_vari* beta_dev_;
  vari* extra_vi_;
  double* g_;
  const double* g_dev_;
  int M_;
  const char* fn_;
  glm_vec_dev_vari(double lp, vari** av, dev_matrix_vari* ad, long long R, const double* th, const double* thd,
                   vari** b, dev_matrix_vari* bd, vari* ex, double* g, const double* gd, int M, const char* fn)
      : local_adjoint_vari(lp), alpha_vis_(av), alpha_dev_(ad), R_(R), th_(th), th_dev_(thd), alo_(nullptr),
        ahi_(nullptr), beta_vi_(b), beta_dev_(bd), extra_vi_(ex), g_(g), g_dev_(gd), M_(M), fn_(fn) {
    if (alpha_vis_)
      for (long long i = 0; i < R_; ++i) {
        if (!alo_ || alpha_vis_[i] < alo_) alo_ = alpha_vis_[i];
        if (!ahi_ || alpha_vis_[i] > ahi_) ahi_ = alpha_vis_[i];
      }
  }
  bool touches_adjoints_in(const vari* lo, const vari* hi) const override {
    auto in = [&](const vari* v) { return v && v >= lo && v < hi; };
    if (in(extra_vi_)) return true;
    if (beta_vi_)
      for (int j = 0; j < M_; ++j)
        if (in(beta_vi_[j])) return true;
    if (alpha_vis_ && alo_ && alo_ < hi && ahi_ >= lo)
      for (long long i = 0; i < R_; ++i)
        if (in(alpha_vis_[i])) return true;
    return false;
  }
  void chain() override {
    if (alpha_vis_)
      for (long long i = 0; i < R_; ++i) alpha_vis_[i]->adj_ += adj_ * th_[i];
    if (alpha_dev_ && R_ > 0)
      amd::check(smg_axpy(amd::ctx(), R_, adj_, th_dev_, 1, alpha_dev_->adj(), 1), fn_);
    if (beta_vi_)
      for (int j = 0; j < M_; ++j) beta_vi_[j]->adj_ += adj_ * g_[1 + j];
    if (beta_dev_) amd::check(smg_axpy(amd::ctx(), M_, adj_, g_dev_, 1, beta_dev_->adj(), 1), fn_);
    if (extra_vi_) extra_vi_->adj_ += adj_ * g_[M_ + 1];
  }
};

// the node of a vector-intercept GLM: theta' of host vars is copied into the
// arena here, a device vector's stays on the device; g = [-, beta'(M), extra']
inline vari* glm_vec_node(const char* fn, double lp, const glm_params& p, const glm_vec_alpha& a, long long rows,
                          vari* extra_vi, double* g, const double* g_dev, int M) {
  double* th = nullptr;
  if (p.alpha_vis) {
    th = ChainableStack::instance_->memalloc_.alloc_array<double>(size_t(rows > 0 ? rows : 1));
    if (rows > 0) amd::to_host(th, a.thp, size_t(rows));
  }
  return new glm_vec_dev_vari(lp, p.alpha_vis, p.alpha_dev, rows, th, a.thp, p.beta_vi, p.beta_dev, extra_vi, g,
                              g_dev, M, fn);
}

}  // namespace internal
}  // namespace math
}  // namespace stan
#endif
