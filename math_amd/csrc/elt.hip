// Element-wise maps over device vectors, forward and reverse: the unary
// transforms (exp, log, sqrt, square, inv, inv_logit, log_inv_logit,
// log1p_exp, tanh) and the binary arithmetic (add, subtract, elt_multiply,
// elt_divide) of the tape's device-resident matrices (rev/fun/elt_ops.hpp).
// One kernel template per direction, the operation a template parameter, a
// grid-stride loop over n; nothing synchronises with the host.
//
// Access width W: 1 = one 8-byte element per lane and trip, 2 = two adjacent
// elements (16 bytes) per lane and trip with the odd last element by one lane.
// The 16-byte form needs every vector pointer on a 16-byte boundary; a call
// with one that is not takes the 8-byte form.  By default the forward maps
// and the unary reverse take the 16-byte form and the binary reverse the
// 8-byte form: what each measured faster (DESIGN.md "Element-wise device
// nodes" has the timings); smg_elt_set_width forces one form for all.
#include <cmath>

#include "smg_internal.h"

namespace {

constexpr int ELT_THREADS = 256;        // threads of a block of the maps
constexpr int ELT_MAX_BLOCKS = 8192;    // grid cap of the maps (grid-stride beyond)
constexpr int ELT_RED_THREADS = 1024;   // the reducing reverse: k_normal_fused's launch rule
constexpr int ELT_RED_PER_BLOCK = 4096;
constexpr int ELT_RED_MAX_BLOCKS = 512;
constexpr int ELT_MAP_WIDTH = 2;         // forward maps and the unary reverse: 16 bytes per lane
constexpr int ELT_BINARY_REV_WIDTH = 1;  // the binary reverse (up to five streams read, two written): 8 bytes

// elements per lane and trip of aligned calls: the defaults above unless the context forces 1 or 2
inline int map_width(const smg_ctx* ctx) { return ctx->elt_width ? ctx->elt_width : ELT_MAP_WIDTH; }
inline int binary_rev_width(const smg_ctx* ctx) { return ctx->elt_width ? ctx->elt_width : ELT_BINARY_REV_WIDTH; }

// With e = exp(-|x|) (prim/scal/fun/inv_logit.hpp, log1p_exp.hpp,
// log_inv_logit.hpp in forms that neither overflow nor cancel):
//   inv_logit     = x >= 0 ? 1 / (1 + e) : e / (1 + e)
//   log1p_exp     = max(x, 0) + log1p(e)
//   log_inv_logit = min(x, 0) - log1p(e)
// log1p(e) for e = exp(-|x|) in [0, 1]: below 2^-54 it is e to the last bit
// (e^2 / 2 is under half an ulp of e), and the device library's log1p gives 0
// for the smallest subnormal, which is what e is at |x| = 745
__device__ __forceinline__ double dev_log1p_e(double e) { return e < 0x1p-54 ? e : log1p(e); }

__device__ __forceinline__ double dev_inv_logit(double x) {
  const double e = exp(-fabs(x));
  return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

template <int OP>
__device__ __forceinline__ double elt_value(double x) {
  switch (OP) {
    case SMG_ELT_EXP: return exp(x);
    case SMG_ELT_LOG: return log(x);
    case SMG_ELT_SQRT: return sqrt(x);
    case SMG_ELT_SQUARE: return x * x;
    case SMG_ELT_INV: return 1.0 / x;
    case SMG_ELT_INV_LOGIT: return dev_inv_logit(x);
    case SMG_ELT_LOG_INV_LOGIT: return (x < 0.0 ? x : (x == x ? 0.0 : x)) - dev_log1p_e(exp(-fabs(x)));
    case SMG_ELT_LOG1P_EXP: return (x > 0.0 ? x : (x == x ? 0.0 : x)) + dev_log1p_e(exp(-fabs(x)));
    default: return tanh(x);
  }
}

// f'(x), evaluated from x (y: the stored value, read by exp, sqrt and inv
// alone) in forms without cancellation: every element is accurate relative
// to its own size, the tails included (y (1 - y) and 1 - y^2 are not).
//   inv_logit' = e / (1 + e)^2;   tanh' = 4 t / (1 + t)^2, t = exp(-2 |x|)
//   log1p_exp' = inv_logit(x);    log_inv_logit' = inv_logit(-x)
template <int OP>
__device__ __forceinline__ double elt_partial(double x, double y) {
  switch (OP) {
    case SMG_ELT_EXP: return y;
    case SMG_ELT_LOG: return 1.0 / x;
    case SMG_ELT_SQRT: return 0.5 / y;
    case SMG_ELT_SQUARE: return 2.0 * x;
    case SMG_ELT_INV: return -(y * y);
    case SMG_ELT_INV_LOGIT: {
      const double e = exp(-fabs(x)), d = 1.0 + e;
      return e / (d * d);
    }
    case SMG_ELT_LOG_INV_LOGIT: return dev_inv_logit(-x);
    case SMG_ELT_LOG1P_EXP: return dev_inv_logit(x);
    default: {
      const double t = exp(-2.0 * fabs(x)), d = 1.0 + t;
      return 4.0 * t / (d * d);
    }
  }
}

constexpr bool elt_reads_y(int op) { return op == SMG_ELT_EXP || op == SMG_ELT_SQRT || op == SMG_ELT_INV; }

template <int OP>
__device__ __forceinline__ double bin_value(double a, double b) {
  switch (OP) {
    case SMG_ELT_ADD: return a + b;
    case SMG_ELT_SUBTRACT: return a - b;
    case SMG_ELT_MULTIPLY: return a * b;
    default: return a / b;
  }
}

// c' times dc/da and dc/db
template <int OP>
__device__ __forceinline__ void bin_partials(double a, double b, double ca, double& da, double& db) {
  switch (OP) {
    case SMG_ELT_ADD: da = ca; db = ca; break;
    case SMG_ELT_SUBTRACT: da = ca; db = -ca; break;
    case SMG_ELT_MULTIPLY: da = ca * b; db = ca * a; break;
    default: {
      const double ib = 1.0 / b;
      da = ca * ib;
      db = -(da * (a * ib));
    }
  }
}

// the grid-stride walk: W elements per lane and trip; with W = 2 the odd last
// element belongs to the lane that would take the next pair
struct elt_walk {
  long long i, stride, end;
  __device__ __forceinline__ elt_walk(long long n, int W) {
    i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * W;
    stride = (long long)gridDim.x * blockDim.x * W;
    end = W == 2 ? (n & ~1LL) : n;
  }
};

template <int OP, int W>
__global__ void __launch_bounds__(ELT_THREADS) k_elt_unary_fwd(const double* __restrict__ x, long long n,
                                                               double* __restrict__ y) {
  elt_walk w(n, W);
  for (long long i = w.i; i < w.end; i += w.stride) {
    if (W == 2) {
      const d2v v = *reinterpret_cast<const d2v*>(x + i);
      d2v r;
      r.x = elt_value<OP>(v.x);
      r.y = elt_value<OP>(v.y);
      *reinterpret_cast<d2v*>(y + i) = r;
    } else {
      y[i] = elt_value<OP>(x[i]);
    }
  }
  if (W == 2 && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0) y[n - 1] = elt_value<OP>(x[n - 1]);
}

// xadj[i] += yadj[i] f'(x[i])
template <int OP, int W>
__global__ void __launch_bounds__(ELT_THREADS) k_elt_unary_rev(const double* __restrict__ x,
                                                               const double* __restrict__ y, long long n,
                                                               const double* __restrict__ ya,
                                                               double* __restrict__ xa) {
  constexpr bool RY = elt_reads_y(OP);
  elt_walk w(n, W);
  for (long long i = w.i; i < w.end; i += w.stride) {
    if (W == 2) {
      const d2v xv = *reinterpret_cast<const d2v*>(x + i);
      const d2v yv = RY ? *reinterpret_cast<const d2v*>(y + i) : xv;
      const d2v av = *reinterpret_cast<const d2v*>(ya + i);
      d2v r = *reinterpret_cast<const d2v*>(xa + i);
      r.x += av.x * elt_partial<OP>(xv.x, yv.x);
      r.y += av.y * elt_partial<OP>(xv.y, yv.y);
      *reinterpret_cast<d2v*>(xa + i) = r;
    } else {
      const double xv = x[i];
      xa[i] += ya[i] * elt_partial<OP>(xv, RY ? y[i] : xv);
    }
  }
  if (W == 2 && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double xv = x[n - 1];
    xa[n - 1] += ya[n - 1] * elt_partial<OP>(xv, RY ? y[n - 1] : xv);
  }
}

// c = a op b; a null operand pointer selects the scalar a0 / b0
template <int OP, int W>
__global__ void __launch_bounds__(ELT_THREADS) k_elt_binary_fwd(const double* __restrict__ a,
                                                                const double* __restrict__ b, double a0, double b0,
                                                                long long n, double* __restrict__ c) {
  elt_walk w(n, W);
  for (long long i = w.i; i < w.end; i += w.stride) {
    if (W == 2) {
      d2v av, bv, r;
      if (a) av = *reinterpret_cast<const d2v*>(a + i); else av.x = av.y = a0;
      if (b) bv = *reinterpret_cast<const d2v*>(b + i); else bv.x = bv.y = b0;
      r.x = bin_value<OP>(av.x, bv.x);
      r.y = bin_value<OP>(av.y, bv.y);
      *reinterpret_cast<d2v*>(c + i) = r;
    } else {
      c[i] = bin_value<OP>(a ? a[i] : a0, b ? b[i] : b0);
    }
  }
  if (W == 2 && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    c[n - 1] = bin_value<OP>(a ? a[n - 1] : a0, b ? b[n - 1] : b0);
}

// one element of the reverse: aadj and badj may be the same buffer (the same
// node as both operands), so b's read-modify-write follows a's store and the
// two pointers are not declared __restrict__
template <int OP>
__device__ __forceinline__ void bin_rev_one(double av, double bv, double ca, double* aadj, double* badj,
                                            long long i, double& sa, double& sb) {
  double da, db;
  bin_partials<OP>(av, bv, ca, da, db);
  if (aadj) aadj[i] += da;
  if (badj) badj[i] += db;
  sa += da;
  sb += db;
}

// aadj += cadj dc/da, badj += cadj dc/db where the pointers are non-null.
// RED: the sums of cadj dc/da (want & 1) and cadj dc/db (want & 2) over the
// elements are WRITTEN to red[0] / red[1]: per-block partials, the
// self-resetting ticket, a final sum in block order (k_normal_fused's
// protocol without the completion word: the consumer reads red on the
// stream).  Bitwise repeatable.
template <int OP, int W, bool RED>
__global__ void __launch_bounds__(RED ? ELT_RED_THREADS : ELT_THREADS) k_elt_binary_rev(
    const double* __restrict__ a, const double* __restrict__ b, double a0, double b0, long long n,
    const double* __restrict__ cadj, double* aadj, double* badj, int want, double* part, unsigned int* counter,
    double* red) {
  __shared__ double lds[2][16];
  __shared__ double fin[2][RED ? ELT_RED_MAX_BLOCKS : 1];
  __shared__ int last;
  double sa = 0.0, sb = 0.0;
  elt_walk w(n, W);
  for (long long i = w.i; i < w.end; i += w.stride) {
    if (W == 2) {
      d2v av, bv;
      if (a) av = *reinterpret_cast<const d2v*>(a + i); else av.x = av.y = a0;
      if (b) bv = *reinterpret_cast<const d2v*>(b + i); else bv.x = bv.y = b0;
      const d2v cv = *reinterpret_cast<const d2v*>(cadj + i);
      double dax, day, dbx, dby;
      bin_partials<OP>(av.x, bv.x, cv.x, dax, dbx);
      bin_partials<OP>(av.y, bv.y, cv.y, day, dby);
      if (aadj) {
        d2v r = *reinterpret_cast<const d2v*>(aadj + i);
        r.x += dax;
        r.y += day;
        *reinterpret_cast<d2v*>(aadj + i) = r;
      }
      if (badj) {
        d2v r = *reinterpret_cast<const d2v*>(badj + i);
        r.x += dbx;
        r.y += dby;
        *reinterpret_cast<d2v*>(badj + i) = r;
      }
      sa += dax;
      sa += day;
      sb += dbx;
      sb += dby;
    } else {
      bin_rev_one<OP>(a ? a[i] : a0, b ? b[i] : b0, cadj[i], aadj, badj, i, sa, sb);
    }
  }
  if (W == 2 && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    bin_rev_one<OP>(a ? a[n - 1] : a0, b ? b[n - 1] : b0, cadj[n - 1], aadj, badj, n - 1, sa, sb);
  if (!RED) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const double ta = (want & 1) ? wave_sum(sa) : 0.0;
  const double tb = (want & 2) ? wave_sum(sb) : 0.0;
  if (lane == 0) {
    lds[0][wv] = ta;
    lds[1][wv] = tb;
  }
  __syncthreads();
  const int col = threadIdx.x;
  double tot = 0.0;  // thread c < 2: column c summed over the block's waves in order
  if (col < 2)
    for (int k = 0; k < nw; ++k) tot += lds[col][k];
  if (gridDim.x > 1) {
    if (col < 2) __hip_atomic_store(part + 2 * blockIdx.x + col, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every wave's stores have left it before the barrier; then one release
    // by thread 0 ahead of the ticket, whose acquire orders the last block's
    // reads of every part (k_normal_fused)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    // the last block: every part into LDS by all threads at once (one thread
    // loading them one after the other spent 90 us on 512 blocks), then each
    // column summed in block order
    for (unsigned int k = threadIdx.x; k < 2 * gridDim.x; k += blockDim.x)
      fin[k & 1][k >> 1] = __hip_atomic_load(part + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (col < 2) {
      tot = 0.0;
      for (unsigned int k = 0; k < gridDim.x; ++k) tot += fin[col][k];
    }
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (col < 2 && ((want >> col) & 1)) red[col] = tot;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int map_grid(long long n, int W) {
  long long g = (n / W + ELT_THREADS - 1) / ELT_THREADS;
  if (g > ELT_MAX_BLOCKS) g = ELT_MAX_BLOCKS;
  if (g < 1) g = 1;
  return (int)g;
}

#define ELT_UNARY_CASES(LAUNCH)                   \
  switch (op) {                                   \
    case SMG_ELT_EXP: LAUNCH(SMG_ELT_EXP); break; \
    case SMG_ELT_LOG: LAUNCH(SMG_ELT_LOG); break; \
    case SMG_ELT_SQRT: LAUNCH(SMG_ELT_SQRT); break; \
    case SMG_ELT_SQUARE: LAUNCH(SMG_ELT_SQUARE); break; \
    case SMG_ELT_INV: LAUNCH(SMG_ELT_INV); break; \
    case SMG_ELT_INV_LOGIT: LAUNCH(SMG_ELT_INV_LOGIT); break; \
    case SMG_ELT_LOG_INV_LOGIT: LAUNCH(SMG_ELT_LOG_INV_LOGIT); break; \
    case SMG_ELT_LOG1P_EXP: LAUNCH(SMG_ELT_LOG1P_EXP); break; \
    default: LAUNCH(SMG_ELT_TANH); break;         \
  }

#define ELT_BINARY_CASES(LAUNCH)                  \
  switch (op) {                                   \
    case SMG_ELT_ADD: LAUNCH(SMG_ELT_ADD); break; \
    case SMG_ELT_SUBTRACT: LAUNCH(SMG_ELT_SUBTRACT); break; \
    case SMG_ELT_MULTIPLY: LAUNCH(SMG_ELT_MULTIPLY); break; \
    default: LAUNCH(SMG_ELT_DIVIDE); break;       \
  }

inline bool unary_op_ok(int op) { return op >= SMG_ELT_EXP && op <= SMG_ELT_TANH; }
inline bool binary_op_ok(int op) { return op >= SMG_ELT_ADD && op <= SMG_ELT_DIVIDE; }

}  // namespace

extern "C" {

int smg_elt_set_width(smg_ctx* ctx, int elements) {
  if (!ctx) return 0;
  const int prev = ctx->elt_width;
  if (elements >= 0 && elements <= 2) ctx->elt_width = elements;
  return prev;
}

int smg_elt_launch_shape(smg_ctx* ctx, int* shape) {
  if (!ctx || !shape) return SMG_ERR_ARG;
  shape[0] = ELT_THREADS;
  shape[1] = ELT_MAX_BLOCKS;
  shape[2] = map_width(ctx);
  shape[3] = ELT_RED_THREADS;
  shape[4] = ELT_RED_PER_BLOCK;
  shape[5] = ELT_RED_MAX_BLOCKS;
  shape[6] = binary_rev_width(ctx);
  return SMG_OK;
}

int smg_elt_unary_fwd(smg_ctx* ctx, int op, const double* x, long long n, double* y) {
  if (!ctx || n < 0 || !unary_op_ok(op)) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  if (!x || !y) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_ELEMWISE);
  const bool wide = map_width(ctx) == 2 && aligned16(x) && aligned16(y);
#define LAUNCH(OP)                                                                                            \
  if (wide)                                                                                                   \
    hipLaunchKernelGGL((k_elt_unary_fwd<OP, 2>), dim3(map_grid(n, 2)), dim3(ELT_THREADS), 0, ctx->stream, x, n, y); \
  else                                                                                                        \
    hipLaunchKernelGGL((k_elt_unary_fwd<OP, 1>), dim3(map_grid(n, 1)), dim3(ELT_THREADS), 0, ctx->stream, x, n, y)
  ELT_UNARY_CASES(LAUNCH)
#undef LAUNCH
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_elt_unary_rev(smg_ctx* ctx, int op, const double* x, const double* y, long long n, const double* yadj,
                      double* xadj) {
  if (!ctx || n < 0 || !unary_op_ok(op)) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  if (!x || !yadj || !xadj || (elt_reads_y(op) && !y)) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_ELEMWISE);
  const bool wide = map_width(ctx) == 2 && aligned16(x) && aligned16(y) && aligned16(yadj) && aligned16(xadj);
#define LAUNCH(OP)                                                                                              \
  if (wide)                                                                                                     \
    hipLaunchKernelGGL((k_elt_unary_rev<OP, 2>), dim3(map_grid(n, 2)), dim3(ELT_THREADS), 0, ctx->stream, x, y, n, \
                       yadj, xadj);                                                                             \
  else                                                                                                          \
    hipLaunchKernelGGL((k_elt_unary_rev<OP, 1>), dim3(map_grid(n, 1)), dim3(ELT_THREADS), 0, ctx->stream, x, y, n, \
                       yadj, xadj)
  ELT_UNARY_CASES(LAUNCH)
#undef LAUNCH
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_elt_binary_fwd(smg_ctx* ctx, int op, const double* a, const double* b, double a0, double b0, long long n,
                       double* c) {
  if (!ctx || n < 0 || !binary_op_ok(op)) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  if (!c) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_ELEMWISE);
  const bool wide = map_width(ctx) == 2 && aligned16(a) && aligned16(b) && aligned16(c);
#define LAUNCH(OP)                                                                                               \
  if (wide)                                                                                                      \
    hipLaunchKernelGGL((k_elt_binary_fwd<OP, 2>), dim3(map_grid(n, 2)), dim3(ELT_THREADS), 0, ctx->stream, a, b, a0, \
                       b0, n, c);                                                                                \
  else                                                                                                           \
    hipLaunchKernelGGL((k_elt_binary_fwd<OP, 1>), dim3(map_grid(n, 1)), dim3(ELT_THREADS), 0, ctx->stream, a, b, a0, \
                       b0, n, c)
  ELT_BINARY_CASES(LAUNCH)
#undef LAUNCH
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_elt_binary_rev(smg_ctx* ctx, int op, const double* a, const double* b, double a0, double b0, long long n,
                       const double* cadj, double* aadj, double* badj, int want_scalar, double* red) {
  if (!ctx || n < 0 || !binary_op_ok(op)) return SMG_ERR_ARG;
  // a scalar operand's sum where its bit is set; a vector operand's bit asks for nothing
  const int want = want_scalar & ((a ? 0 : 1) | (b ? 0 : 2));
  if (want && !red) return SMG_ERR_ARG;
  if (n == 0) return SMG_OK;
  if (!cadj) return SMG_ERR_ARG;
  // a scalar operand has no vector adjoint
  if (!a) aadj = nullptr;
  if (!b) badj = nullptr;
  if (!want && !aadj && !badj) return SMG_OK;
  smg_prof_scope prof(ctx, SMG_FAM_ELEMWISE);
  const bool wide =
      binary_rev_width(ctx) == 2 && aligned16(a) && aligned16(b) && aligned16(cadj) && aligned16(aadj) && aligned16(badj);
  if (!want) {
#define LAUNCH(OP)                                                                                                 \
  if (wide)                                                                                                        \
    hipLaunchKernelGGL((k_elt_binary_rev<OP, 2, false>), dim3(map_grid(n, 2)), dim3(ELT_THREADS), 0, ctx->stream, a, \
                       b, a0, b0, n, cadj, aadj, badj, 0, nullptr, nullptr, nullptr);                              \
  else                                                                                                             \
    hipLaunchKernelGGL((k_elt_binary_rev<OP, 1, false>), dim3(map_grid(n, 1)), dim3(ELT_THREADS), 0, ctx->stream, a, \
                       b, a0, b0, n, cadj, aadj, badj, 0, nullptr, nullptr, nullptr)
    ELT_BINARY_CASES(LAUNCH)
#undef LAUNCH
    SMG_LAUNCH_CHECK();
    return SMG_OK;
  }
  const int nb = n <= ELT_RED_PER_BLOCK
                     ? 1
                     : (int)(n / ELT_RED_PER_BLOCK < ELT_RED_MAX_BLOCKS ? (n + ELT_RED_PER_BLOCK - 1) / ELT_RED_PER_BLOCK
                                                                        : ELT_RED_MAX_BLOCKS);
  double* part = nb > 1 ? smg_ws(ctx, SMG_WS_RED, 2 * (size_t)nb) : nullptr;
  if (nb > 1 && !part) return SMG_ERR_OOM;
#define LAUNCH(OP)                                                                                                  \
  if (wide)                                                                                                         \
    hipLaunchKernelGGL((k_elt_binary_rev<OP, 2, true>), dim3(nb), dim3(ELT_RED_THREADS), 0, ctx->stream, a, b, a0, b0, \
                       n, cadj, aadj, badj, want, part, ctx->red_counter_d, red);                                   \
  else                                                                                                              \
    hipLaunchKernelGGL((k_elt_binary_rev<OP, 1, true>), dim3(nb), dim3(ELT_RED_THREADS), 0, ctx->stream, a, b, a0, b0, \
                       n, cadj, aadj, badj, want, part, ctx->red_counter_d, red)
  ELT_BINARY_CASES(LAUNCH)
#undef LAUNCH
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

}  // extern "C"
