#ifndef STAN_MATH_REV_FUN_INDEX_OPS_HPP
#define STAN_MATH_REV_FUN_INDEX_OPS_HPP

// Indexing a device vector of vars by group: the Stan language's u[g]
// (stan::model::rvalue(u, index_multi(g))) and its mirror image, the
// per-group sums.  What a hierarchical model needs between its group-level
// parameters and a row-level likelihood, without leaving the device:
//
//   dev_index idx = to_dev_index(group, J);      // once, outside gradient()
//   ... poisson_log_glm_lpmf(y, x, gather(u, idx), beta) + normal_lpdf(u, 0, tau)
//
//   dev_index      g and its inverted index on the device: perm, the rows
//                  sorted by group (stably, so each group's rows ascend), and
//                  offs, each group's range of perm.  to_dev_index builds it
//                  on the host by a counting sort, O(R + J), and uploads it
//                  once; it is arena-owned like dev_data, so build it before
//                  gradient() / start_nested() and it outlives the evaluations.
//   gather         u[g]: R x 1 from u (J x 1 or 1 x J).  One node: the value
//                  by smg_gather, the adjoint by smg_segment_sum into u's
//                  adjoint (math_amd/csrc/index.hip: no atomics, a fixed
//                  order of summation, bitwise repeatable).
//   segment_sum    out[j] = the sum of v over the rows of group j: J x 1 from
//                  v (R x 1 or 1 x R); the same two kernels the other way round.
// Indices are 1-based.  to_dev_index checks every index before it touches the
// device and throws std::out_of_range with check_range's message
// (prim/mat/err/check_range.hpp, prim/scal/err/out_of_range.hpp).  R == 0
// gives an empty matrix and no node.

#include <stan/math/amd/matrix.hpp>
#include <stan/math/rev/core.hpp>

#include <sstream>
#include <stdexcept>
#include <vector>

namespace stan {
namespace math {

/** A multi-index g (R indices into a container of J elements) on the device
 * with its inverted index.  Arena-owned, trivially destructible. */
class dev_index {
 public:
  const int* g_ = nullptr;           // R, 1-based
  const int* perm_ = nullptr;        // R rows (0-based) sorted by group, stably
  const long long* offs_ = nullptr;  // J + 1: group j's rows are perm[offs[j] .. offs[j+1])
  double* ws_ = nullptr;             // smg_segment_sum's partials
  long long R_ = 0;
  int J_ = 0;
  /** the size of the container it indexes (J) */
  int size() const { return J_; }
  /** how many indices it holds (R): the rows of u[g] */
  long long rows() const { return R_; }
};

inline dev_index to_dev_index(const std::vector<int>& g, int size) {
  if (size < 0) throw std::invalid_argument("to_dev_index: size must not be negative, but is " + std::to_string(size));
  for (size_t i = 0; i < g.size(); ++i)
    if (g[i] < 1 || g[i] > size) {
      std::ostringstream m;
      m << "to_dev_index: accessing element out of range. index " << g[i] << " out of range; ";
      if (size == 0) m << "container is empty and cannot be indexed";
      else m << "expecting index to be between 1 and " << size;
      m << "; position = " << i + 1;
      throw std::out_of_range(m.str());
    }
  const size_t R = g.size(), J = size_t(size);
  std::vector<long long> offs(J + 1, 0);
  for (size_t i = 0; i < R; ++i) ++offs[size_t(g[i])];
  for (size_t j = 0; j < J; ++j) offs[j + 1] += offs[j];
  std::vector<int> perm(R);
  {
    std::vector<long long> at(offs.begin(), offs.end() - 1);
    for (size_t i = 0; i < R; ++i) perm[size_t(at[size_t(g[i]) - 1]++)] = int(i);
  }
  dev_index idx;
  idx.R_ = (long long)R;
  idx.J_ = size;
  int* gd = amd::alloc_ints(R);
  int* pd = amd::alloc_ints(R);
  // (the offsets travel as 8-byte words)
  double* od = amd::alloc_doubles(J + 1);
  amd::to_device_int(gd, g.data(), R);
  amd::to_device_int(pd, perm.data(), R);
  amd::to_device(od, reinterpret_cast<const double*>(offs.data()), J + 1);
  idx.g_ = gd;
  idx.perm_ = pd;
  idx.offs_ = reinterpret_cast<const long long*>(od);
  idx.ws_ = amd::alloc_doubles(size_t(smg_segment_sum_ws_doubles(idx.R_, idx.J_)));
  return idx;
}

namespace internal {

// u (J x 1 or 1 x J) against the index's container size
inline void index_check_container(const char* fn, int rows, int cols, size_t n, const dev_index& idx) {
  if ((rows == 1 || cols == 1 || n == 0) && n == size_t(idx.size())) return;
  std::ostringstream m;
  m << fn << ": u must be a vector of the size the index was built for, " << idx.size() << ", but is " << rows
    << " x " << cols << " (size " << n << ")";
  throw std::invalid_argument(m.str());
}

class gather_dev_vari : public device_vari {
 public:
  dev_matrix_vari* u_;
  dev_matrix_vari* y_;
  dev_index idx_;
  gather_dev_vari(dev_matrix_vari* u, const dev_index& idx)
      : device_vari(0.0), u_(u), y_(new dev_matrix_vari(int(idx.rows()), 1)), idx_(idx) {
    u_->want_adjoint();
    amd::check(smg_gather(amd::ctx(), u_->val(), idx_.g_, idx_.R_, 0, y_->raw_val()), "gather");
  }
  void chain() override {
    amd::check(smg_segment_sum(amd::ctx(), y_->adj(), idx_.perm_, idx_.offs_, idx_.R_, idx_.J_, 1, idx_.ws_,
                               u_->adj()),
               "gather");
  }
};

class segment_sum_dev_vari : public device_vari {
 public:
  dev_matrix_vari* v_;
  dev_matrix_vari* y_;
  dev_index idx_;
  segment_sum_dev_vari(dev_matrix_vari* v, const dev_index& idx)
      : device_vari(0.0), v_(v), y_(new dev_matrix_vari(idx.size(), 1)), idx_(idx) {
    v_->want_adjoint();
    amd::check(smg_segment_sum(amd::ctx(), v_->val(), idx_.perm_, idx_.offs_, idx_.R_, idx_.J_, 0, idx_.ws_,
                               y_->raw_val()),
               "segment_sum");
  }
  void chain() override {
    amd::check(smg_gather(amd::ctx(), y_->adj(), idx_.g_, idx_.R_, 1, v_->adj()), "segment_sum");
  }
};

}  // namespace internal

/** u[g]: R x 1. */
inline dev_var_matrix gather(const dev_var_matrix& u, const dev_index& idx) {
  internal::index_check_container("gather", u.rows(), u.cols(), u.size(), idx);
  if (idx.rows() == 0) return dev_var_matrix(new dev_matrix_vari(0, 1));
  return dev_var_matrix((new internal::gather_dev_vari(u.vi_, idx))->y_);
}
inline dev_var_matrix gather(const std::vector<var>& u, const dev_index& idx) {
  internal::index_check_container("gather", int(u.size()), 1, u.size(), idx);
  if (idx.rows() == 0) return dev_var_matrix(new dev_matrix_vari(0, 1));
  return gather(to_dev(u), idx);
}
/** u[g] of constant data: no node. */
inline dev_data<double> gather(const dev_data<double>& u, const dev_index& idx) {
  internal::index_check_container("gather", u.rows(), u.cols(), u.size(), idx);
  const size_t R = size_t(idx.rows());
  if (R == 0) return dev_data<double>(nullptr, 0, 0, 1);
  double* d = amd::alloc_doubles(R);
  amd::check(smg_gather(amd::ctx(), u.data(), idx.g_, idx.R_, 0, d), "gather");
  return dev_data<double>(d, R, int(R), 1);
}

/** out[j] = the sum of v[i] over the rows i with g[i] == j + 1: J x 1 from v
 * (R x 1 or 1 x R); a group without rows gets 0. */
inline dev_var_matrix segment_sum(const dev_var_matrix& v, const dev_index& idx) {
  if (!(v.rows() == 1 || v.cols() == 1 || v.size() == 0) || (long long)v.size() != idx.rows()) {
    std::ostringstream m;
    m << "segment_sum: v must be a vector with one element per index, " << idx.rows() << ", but is " << v.rows()
      << " x " << v.cols() << " (size " << v.size() << ")";
    throw std::invalid_argument(m.str());
  }
  if (idx.rows() == 0) {  // every group is empty: zeros, and nothing to differentiate
    auto* y = new dev_matrix_vari(idx.size(), 1);
    amd::zero(y->raw_val(), y->size());
    return dev_var_matrix(y);
  }
  return dev_var_matrix((new internal::segment_sum_dev_vari(v.vi_, idx))->y_);
}

}  // namespace math
}  // namespace stan
#endif
