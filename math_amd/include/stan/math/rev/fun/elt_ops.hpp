#ifndef STAN_MATH_REV_FUN_ELT_OPS_HPP
#define STAN_MATH_REV_FUN_ELT_OPS_HPP

// Element-wise arithmetic and transforms on device matrices of vars: what
// sits between the producers of a dev_var_matrix (cholesky_decompose,
// multiply, mdivide_left_tri, the GP covariances) and the reducers that take
// one (normal_lpdf, student_t_lpdf, cauchy_lpdf, multi_normal_cholesky_lpdf,
// the GLMs' per-row intercept).
//
//   unary   exp, log, sqrt, square, inv, inv_logit, log_inv_logit, log1p_exp,
//           tanh of a dev_var_matrix (apply_scalar_unary over
//           prim/scal/fun/*.hpp, rev/scal/fun/*.hpp): one node, value and
//           adjoint by the streaming kernels smg_elt_unary_* (math_amd/csrc/elt.hip)
//   binary  add, subtract, elt_multiply, elt_divide of a dev_var_matrix with a
//           dev_var_matrix or dev_data<double> of the same shape (add of two
//           dev_var_matrix stays mix/fvar_functors.hpp's), and add, subtract,
//           divide, elt_divide with a scalar var or double
//           (prim/mat/fun/{add,subtract,elt_multiply,elt_divide,divide}.hpp);
//           a scalar var's adjoint is reduced on the device and lands through
//           add_pending_adjoint, as multiply(var, dev_var_matrix)'s does.
//   scalar  inv, inv_logit, log_inv_logit, log1p_exp, tanh of a var: host tape
//           nodes with the kernels' formulas, so one name serves a scalar and
//           a device vector.
// With e = exp(-|x|):  inv_logit = x >= 0 ? 1/(1+e) : e/(1+e),
//   log1p_exp = max(x, 0) + log1p(e),  log_inv_logit = min(x, 0) - log1p(e);
//   inv_logit' = e/(1+e)^2,  log1p_exp' = inv_logit(x),
//   log_inv_logit' = inv_logit(-x),  tanh' = 4t/(1+t)^2 with t = exp(-2|x|).
// A size-zero operand gives an empty matrix and no node.

#include <stan/math/amd/matrix.hpp>
#include <stan/math/rev/core.hpp>

#include <cmath>
#include <sstream>
#include <stdexcept>

namespace stan {
namespace math {

// ------------------------------------------------------------ scalars
inline double inv(double x) { return 1.0 / x; }
inline double inv_logit(double x) {
  const double e = std::exp(-std::fabs(x));
  return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}
inline double log_inv_logit(double x) {
  return (x < 0.0 ? x : (x == x ? 0.0 : x)) - std::log1p(std::exp(-std::fabs(x)));
}

inline var inv(const var& a) {
  const double y = 1.0 / a.val();
  return var(new internal::unary_vari(y, a.vi_, -(y * y)));
}
inline var inv_logit(const var& a) {
  const double x = a.val(), e = std::exp(-std::fabs(x)), d = 1.0 + e;
  return var(new internal::unary_vari(x >= 0.0 ? 1.0 / d : e / d, a.vi_, e / (d * d)));
}
inline var log_inv_logit(const var& a) {
  return var(new internal::unary_vari(log_inv_logit(a.val()), a.vi_, inv_logit(-a.val())));
}
inline var log1p_exp(const var& a) {
  const double x = a.val();
  return var(new internal::unary_vari((x > 0.0 ? x : (x == x ? 0.0 : x)) + std::log1p(std::exp(-std::fabs(x))), a.vi_,
                                      inv_logit(x)));
}
inline var tanh(const var& a) {
  const double x = a.val(), t = std::exp(-2.0 * std::fabs(x)), d = 1.0 + t;
  return var(new internal::unary_vari(std::tanh(x), a.vi_, 4.0 * t / (d * d)));
}

namespace internal {

// ------------------------------------------------------------ unary nodes
class elt_unary_dev_vari : public device_vari {
 public:
  int op_;
  const char* fn_;
  dev_matrix_vari* x_;
  dev_matrix_vari* y_;
  elt_unary_dev_vari(int op, const char* fn, dev_matrix_vari* x)
      : device_vari(0.0), op_(op), fn_(fn), x_(x), y_(new dev_matrix_vari(x->rows_, x->cols_)) {
    x->want_adjoint();
    amd::check(smg_elt_unary_fwd(amd::ctx(), op_, x_->val(), (long long)x_->size(), y_->raw_val()), fn_);
  }
  void chain() override {
    amd::check(smg_elt_unary_rev(amd::ctx(), op_, x_->val(), y_->raw_val(), (long long)x_->size(), y_->adj(),
                                 x_->adj()),
               fn_);
  }
};

inline dev_var_matrix elt_unary(int op, const char* fn, const dev_var_matrix& x) {
  if (x.size() == 0) return dev_var_matrix(new dev_matrix_vari(x.rows(), x.cols()));
  return dev_var_matrix((new elt_unary_dev_vari(op, fn, x.vi_))->y_);
}

// ------------------------------------------------------------ binary nodes
/** One operand of an element-wise binary node: a device var matrix, constant
 * device data, or a scalar (var or double) broadcast over the other's shape. */
struct elt_operand {
  dev_matrix_vari* vi = nullptr;  // a var matrix
  const double* data = nullptr;   // a data matrix
  double s = 0.0;                 // the scalar's value
  vari* svi = nullptr;            // the scalar's vari (null: double)
  bool is_vector() const { return vi || data; }
  const double* val() const { return vi ? vi->val() : data; }
  double* adj() const { return vi ? vi->adj() : nullptr; }
};
inline elt_operand elt_op(const dev_var_matrix& m) {
  elt_operand o;
  o.vi = m.vi_;
  return o;
}
inline elt_operand elt_op(const dev_data<double>& d) {
  elt_operand o;
  o.data = d.data();
  return o;
}
inline elt_operand elt_op(const var& c) {
  elt_operand o;
  o.s = c.val();
  o.svi = c.vi_;
  return o;
}
inline elt_operand elt_op(double c) {
  elt_operand o;
  o.s = c;
  return o;
}

class elt_binary_dev_vari : public device_vari {
 public:
  int op_;
  const char* fn_;
  elt_operand a_, b_;
  dev_matrix_vari* c_;
  int want_;     // scalar var operands: bit 1 = a, bit 2 = b
  double* red_;  // their reduced adjoints (device, 2 doubles)
  elt_binary_dev_vari(int op, const char* fn, const elt_operand& a, const elt_operand& b, int rows, int cols)
      : device_vari(0.0), op_(op), fn_(fn), a_(a), b_(b), c_(new dev_matrix_vari(rows, cols)),
        want_((a.svi ? 1 : 0) | (b.svi ? 2 : 0)), red_(want_ ? amd::alloc_doubles(2) : nullptr) {
    if (a_.vi) a_.vi->want_adjoint();
    if (b_.vi) b_.vi->want_adjoint();
    amd::check(smg_elt_binary_fwd(amd::ctx(), op_, a_.val(), b_.val(), a_.s, b_.s, (long long)c_->size(),
                                  c_->raw_val()),
               fn_);
  }
  void chain() override {
    amd::check(smg_elt_binary_rev(amd::ctx(), op_, a_.val(), b_.val(), a_.s, b_.s, (long long)c_->size(), c_->adj(),
                                  a_.adj(), b_.adj(), want_, red_),
               fn_);
    if (a_.svi) add_pending_adjoint(a_.svi, red_);
    if (b_.svi) add_pending_adjoint(b_.svi, red_ + 1);
  }
};

inline dev_var_matrix elt_binary(int op, const char* fn, const elt_operand& a, const elt_operand& b, int rows,
                                 int cols) {
  if (size_t(rows) * size_t(cols) == 0) return dev_var_matrix(new dev_matrix_vari(rows, cols));
  return dev_var_matrix((new elt_binary_dev_vari(op, fn, a, b, rows, cols))->c_);
}

template <typename TA, typename TB>
inline dev_var_matrix elt_binary_mm(int op, const char* fn, const TA& A, const TB& B) {
  if (A.rows() != B.rows() || A.cols() != B.cols()) {
    std::ostringstream m;
    m << fn << ": the shapes of A (" << A.rows() << " x " << A.cols() << ") and B (" << B.rows() << " x " << B.cols()
      << ") must match";
    throw std::invalid_argument(m.str());
  }
  return elt_binary(op, fn, elt_op(A), elt_op(B), A.rows(), A.cols());
}

}  // namespace internal

// ------------------------------------------------------------ unary, device
#define SMG_ELT_UNARY_DEV(NAME, OP) \
  inline dev_var_matrix NAME(const dev_var_matrix& x) { return internal::elt_unary(OP, #NAME, x); }
SMG_ELT_UNARY_DEV(exp, SMG_ELT_EXP)
SMG_ELT_UNARY_DEV(log, SMG_ELT_LOG)
SMG_ELT_UNARY_DEV(sqrt, SMG_ELT_SQRT)
SMG_ELT_UNARY_DEV(square, SMG_ELT_SQUARE)
SMG_ELT_UNARY_DEV(inv, SMG_ELT_INV)
SMG_ELT_UNARY_DEV(inv_logit, SMG_ELT_INV_LOGIT)
SMG_ELT_UNARY_DEV(log_inv_logit, SMG_ELT_LOG_INV_LOGIT)
SMG_ELT_UNARY_DEV(log1p_exp, SMG_ELT_LOG1P_EXP)
SMG_ELT_UNARY_DEV(tanh, SMG_ELT_TANH)
#undef SMG_ELT_UNARY_DEV

// ------------------------------------------------------------ binary, matrix with matrix
#define SMG_ELT_BINARY_MM(NAME, OP, TA, TB) \
  inline dev_var_matrix NAME(const TA& A, const TB& B) { return internal::elt_binary_mm(OP, #NAME, A, B); }
SMG_ELT_BINARY_MM(add, SMG_ELT_ADD, dev_var_matrix, dev_data<double>)
SMG_ELT_BINARY_MM(add, SMG_ELT_ADD, dev_data<double>, dev_var_matrix)
SMG_ELT_BINARY_MM(subtract, SMG_ELT_SUBTRACT, dev_var_matrix, dev_var_matrix)
SMG_ELT_BINARY_MM(subtract, SMG_ELT_SUBTRACT, dev_var_matrix, dev_data<double>)
SMG_ELT_BINARY_MM(subtract, SMG_ELT_SUBTRACT, dev_data<double>, dev_var_matrix)
SMG_ELT_BINARY_MM(elt_multiply, SMG_ELT_MULTIPLY, dev_var_matrix, dev_var_matrix)
SMG_ELT_BINARY_MM(elt_multiply, SMG_ELT_MULTIPLY, dev_var_matrix, dev_data<double>)
SMG_ELT_BINARY_MM(elt_multiply, SMG_ELT_MULTIPLY, dev_data<double>, dev_var_matrix)
SMG_ELT_BINARY_MM(elt_divide, SMG_ELT_DIVIDE, dev_var_matrix, dev_var_matrix)
SMG_ELT_BINARY_MM(elt_divide, SMG_ELT_DIVIDE, dev_var_matrix, dev_data<double>)
SMG_ELT_BINARY_MM(elt_divide, SMG_ELT_DIVIDE, dev_data<double>, dev_var_matrix)
#undef SMG_ELT_BINARY_MM

// ------------------------------------------------------------ binary, matrix with scalar (var or double)
#define SMG_ELT_BINARY_MS(NAME, OP, TS)                                                          \
  inline dev_var_matrix NAME(const dev_var_matrix& A, TS c) {                                    \
    return internal::elt_binary(OP, #NAME, internal::elt_op(A), internal::elt_op(c), A.rows(), A.cols()); \
  }
#define SMG_ELT_BINARY_SM(NAME, OP, TS)                                                          \
  inline dev_var_matrix NAME(TS c, const dev_var_matrix& A) {                                    \
    return internal::elt_binary(OP, #NAME, internal::elt_op(c), internal::elt_op(A), A.rows(), A.cols()); \
  }
SMG_ELT_BINARY_MS(add, SMG_ELT_ADD, const var&)
SMG_ELT_BINARY_MS(add, SMG_ELT_ADD, double)
SMG_ELT_BINARY_SM(add, SMG_ELT_ADD, const var&)
SMG_ELT_BINARY_SM(add, SMG_ELT_ADD, double)
SMG_ELT_BINARY_MS(subtract, SMG_ELT_SUBTRACT, const var&)
SMG_ELT_BINARY_MS(subtract, SMG_ELT_SUBTRACT, double)
SMG_ELT_BINARY_SM(subtract, SMG_ELT_SUBTRACT, const var&)
SMG_ELT_BINARY_SM(subtract, SMG_ELT_SUBTRACT, double)
SMG_ELT_BINARY_MS(divide, SMG_ELT_DIVIDE, const var&)
SMG_ELT_BINARY_MS(divide, SMG_ELT_DIVIDE, double)
SMG_ELT_BINARY_SM(elt_divide, SMG_ELT_DIVIDE, const var&)
SMG_ELT_BINARY_SM(elt_divide, SMG_ELT_DIVIDE, double)
#undef SMG_ELT_BINARY_MS
#undef SMG_ELT_BINARY_SM

}  // namespace math
}  // namespace stan
#endif
