// The GLM reducers over rows, each in ONE pass over x (KIND 0-3: scalar
// intercept, or one intercept per row -- AV below):
//   KIND 0  bernoulli_logit_glm_lpmf  (y int in {0,1})
//   KIND 1  normal_id_glm_lpdf        (y double, scalar sigma)
//   KIND 2  poisson_log_glm_lpmf      (y int >= 0)
//   KIND 3  neg_binomial_2_log_glm_lpmf (y int >= 0, scalar precision phi)
//   KIND 4  ordered_logistic_glm_lpmf   (y int in 1..C, C - 1 cut-points, no intercept)
// They differ only in the per-row function of the linear predictor; the
// x-streaming, the x^T theta' product and the deterministic reductions are
// shared.
//
// KIND 1: prim/mat/prob/normal_id_glm_lpdf.hpp:84-150
//   y_scaled = (y - x beta - alpha) / sigma;  mu' = y_scaled / sigma
//   partials: beta' = x^T mu', alpha' = sum mu', sigma' = (sum y_scaled^2 - N)/sigma
//   logp = -N log sqrt(2 pi) - N log sigma - sum y_scaled^2 / 2
//   (device: out = [sum y_scaled^2, sum mu', x^T mu'])
// KIND 2: prim/mat/prob/poisson_log_glm_lpmf.hpp:81-123
//   theta = x beta + alpha;  theta' = y - exp(theta)
//   logp = -sum lgamma(y + 1) + sum(y theta - exp(theta))
//   (device: out = [sum(y theta - exp theta), sum theta', x^T theta', sum lgamma(y + 1)])
// KIND 3: neg_binomial_2_log_glm_lpmf of Stan Math 3.0.0, restated so that no
// term forms exp(theta): with d = theta - log phi and e = exp(-|d|) in (0, 1],
//   lse = log(exp theta + phi) = max(theta, log phi) + log1p(e)
//   s = exp theta / (exp theta + phi) = d >= 0 ? 1 / (1 + e) : e / (1 + e)
//   1 - s = the same with the sign of d flipped
//   theta' = y - (y + phi) s
//   phi'   = sum (1 - (y + phi)(1 - s) / phi) + (log phi - lse)
//                + (digamma(y + phi) - digamma(phi))
//   logp = -C + N (phi log phi - lgamma phi) - A + B + D  (composed by the host)
//   (device: out = [A = sum (y + phi) lse, sum theta', x^T theta', B = sum y theta,
//                   C = sum lgamma(y + 1), D = sum lgamma(y + phi), phi'])
// Every sum is finite for finite theta of any size (the reference's own
// exp(theta) / (exp(theta) + phi) is inf / inf beyond theta = 709).
// KIND 4: ordered_logistic_glm_lpmf, cut-points c_1 < ... < c_{C-1}, c_0 = -inf,
// c_C = +inf; per row k = y, a = c_k - eta, b = c_{k-1} - eta,
// P = logistic(a) - logistic(b), every term from exp(-|.|):
//   ll(z) = min(z, 0) - log1p(exp(-|z|))                  (log logistic(z))
//   lg(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e), e = exp(-|z|)  (logistic(z))
//   gap = c_k - c_{k-1} (from the cut-points, not through eta), and per class
//   lm = log1m_exp(-gap), r = 1 / expm1(gap)              (both 0 for k = 1 and k = C)
//   log P  = [k < C] ll(a) + [k > 1] ll(-b) + lm
//   d_hi   = dlogP/dc_k     = [k < C] (lg(-a) + r)
//   d_lo   = dlogP/dc_{k-1} = [k > 1] (-lg(b) - r)
//   theta' = dlogP/deta     = [k > 1] lg(b) - [k < C] lg(-a)   (the r terms cancel exactly)
//   beta' = x^T theta',  cuts'_j = sum_{y = j} d_hi + sum_{y = j + 1} d_lo
//   (device: ab = [beta(M), cuts(C - 1)], out = [logp, beta'(M), cuts'(C - 1)])
// Every thread evaluates one side of its row: lanes l and l + 32 of a wave
// hold the same row, the lower half takes z = a, the upper z = -b, and one
// lane exchange gives both theta' (one exp and one division per thread;
// both sides on every thread measured 1.39x Poisson's time at 1e6 x 256 and
// 1.99x at 1e6 x 8).
// The cut-point gradient is a per-class binning of row terms.  Each of the 64
// lanes of wave 0 (32 rows x 2 sides) owns one LDS slot per cut-point,
// ol_bin[j][lane], and adds its row's d_hi (lower half, j = k) or d_lo (upper
// half, j = k - 1) to its own slot: a private read-add-write indexed by the
// clamped class, so there is no race, no atomic, no barrier beyond the
// loop's one per tile, and a lane's slot sees its tiles in tile order.  After
// the loop thread j sums slot row j over the 64 lanes in lane order.  The
// same inputs on the same grid give the same bits.  (Measured before this:
// the row terms left in a double-buffered LDS array and bin j summed over the
// 32 rows by one thread after the next tile's barrier -- 1.63x Poisson's time
// at 1e6 x 256 and 2.4x at 1e6 x 8 with the row loop rolled: one wave's serial
// LDS reads sit on every tile's critical path.)
//
// KIND 0:
// Reference: prim/mat/prob/bernoulli_logit_glm_lpmf.hpp:46-138
//   ytheta = sign .* (x beta + alpha), sign = 2y - 1            (:92-94)
//   logp   = sum( ytheta > 20 ? -exp(-ytheta)
//               : ytheta < -20 ? ytheta : -log1p(exp(-ytheta)) )  (:99-104)
//   theta' = ytheta > 20 ? -exp(-ytheta) : ytheta < -20 ? sign
//               : sign exp(-ytheta) / (exp(-ytheta) + 1)         (:115-121)
//   d/dbeta = x^T theta',  d/dalpha = sum theta'                  (:123, :133)
// The reference makes two GEMV passes over x (HBM-bound).  Here persistent
// workgroups stream 32-row tiles of x (column-major) once: the tile yields
// eta for its rows, then theta', then its contribution to x^T theta' while it
// is still on chip.  Each workgroup keeps per-column accumulators in
// registers and writes one [logp, alpha', beta'(M)] partial; a fixed-order
// second pass sums the partials (deterministic).  The default kernel is
// k_glm_reg (the tile stays in registers); the LDS-staged form measured
// slower (below) and lives in git history.
//
// Measured at 1e7 x 256 on MI355X (bench.py --workload glm, same box):
//   k_glm_fused 32 rows x 256 threads, 512 WGs   5.08 TB/s
//   k_glm_reg   32 rows x 512 threads            5.67-5.74 TB/s (256 or 512 WGs)
//   k_glm_reg   16 rows x 256 threads            4.75 TB/s (128-byte column segments)
//   k_glm_reg   16 rows x 512 threads            4.04 TB/s
//   k_glm_reg   32 x 512 with two tiles in flight (3 register buffers): no gain
//   k_glm_reg   32 x 512, x read with nontemporal loads (x is streamed once,
//               it should not displace other lines): 5.61-5.73 -> 5.81 TB/s
// The first k_glm_reg build ran at 1.7 TB/s: a branch or a select next to a
// load, a loop-carried register copy and a y load issued after x each made
// the compiler wait for the loads within the tile that issued them.
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "smg_internal.h"
#include "special_dev.h"  // dev_lgamma, dev_digamma (KIND 3)

namespace {

constexpr int MMAX = 256;         // fused path: M <= 256
constexpr int OL_CMAX = 16;       // ordered_logistic: C <= 16 classes (CAT_CMAX's value)

// zero page (global address space) for out-of-range loads: the address is
// redirected, no select on the loaded value
__device__ double g_glm_zero[2] = {0.0, 0.0};


// Register-resident variant: the tile never goes through LDS.  512 threads:
// thread t holds row r = t & 31 of the tile and the 16 columns c = g + 16q
// (g = t >> 5, q = 0..15): eta_r is 16 FMAs per thread plus one 16-way sum through a small
// LDS array (double-buffered: one barrier per tile), every thread forms
// theta'_r for its own row, and x^T theta' accumulates in 16 registers per
// thread (summed over the 32 rows of a column group once, at the end, by
// lane shuffles).  A load instruction still covers two 256-byte column
// segments per wave.
// check_y (KIND 0): also count the rows whose y is outside {0, 1} (the
// reference's check_bounded(y, 0, 1), prim/mat/prob/bernoulli_logit_glm_lpmf.hpp:75)
// into partial slot M + 2 -- the pass reads y anyway, so the check costs no
// extra launch and no extra pass over y.
// KIND 4 takes its number of classes C in the check_y argument.
// AV (KIND 0-3): one intercept per row, av[R], in place of ab[0] (not read);
// the row's value is loaded with its y and carried with it, and the row's
// theta' -- the partial of its intercept -- is stored to thp[R] unless thp is
// null.  Everything of this mode sits under `if (AV)`: the scalar
// instantiations are the code they were.
template <int KIND, int RB, int NT, bool NTL, bool AV = false>
__device__ __forceinline__ void glm_reg_body(const void* __restrict__ yv, const double* __restrict__ x, long long R,
                                             int M, long long ldx, const double* __restrict__ ab,
                                             double* __restrict__ part, int check_y,
                                             const double* __restrict__ av = nullptr,
                                             double* __restrict__ thp = nullptr) {
  static_assert(!AV || KIND < 4, "KIND 4 has no intercept");
  constexpr int G = NT / RB, Q = MMAX / G;
  const int* __restrict__ y = static_cast<const int*>(yv);
  const double* __restrict__ yd = static_cast<const double*>(yv);
  __shared__ double beta[MMAX];
  __shared__ double red[2][G][RB];
  __shared__ double lds[16];
  // KIND 4: cut[k] = c_k (k = 0..C), lm / r of class k, and wave 0's private
  // bins ol_bin[j][lane] (j = 0 and j = C take the masked-out sides' zeros)
  constexpr int OLC = KIND == 4 ? OL_CMAX + 1 : 1, OLW = KIND == 4 ? 64 : 1;
  static_assert(KIND != 4 || RB == 32, "KIND 4 pairs lanes l and l + 32 of a 64-lane wave on one row");
  __shared__ double ol_cut[OLC], ol_lm[OLC], ol_r[OLC];
  __shared__ double ol_bin[OLC][OLW];
  const int t = threadIdx.x, r = t % RB, g = t / RB;
  for (int c = t; c < MMAX; c += NT) beta[c] = c < M ? ab[(KIND == 4 ? 0 : 1) + c] : 0.0;
  const double alpha = (KIND == 4 || AV) ? 0.0 : ab[0];
  const int C = KIND == 4 ? (check_y < 1 ? 1 : (check_y > OL_CMAX ? OL_CMAX : check_y)) : 0;
  if (KIND == 4) {
    if (t <= C) {  // class t's constants (t = 0: only c_0)
      const double clo = t >= 2 ? ab[M + t - 2] : -INFINITY;
      const double chi = t == 0 ? -INFINITY : (t < C ? ab[M + t - 1] : INFINITY);
      const bool mid = t >= 2 && t < C;
      const double gap = mid ? chi - clo : 1.0;
      const double lm = gap < 0.693147180559945309417 ? log(-expm1(-gap)) : log1p(-exp(-gap));
      ol_cut[t] = chi;
      ol_lm[t] = mid ? lm : 0.0;
      ol_r[t] = mid ? 1.0 / expm1(gap) : 0.0;
    }
    for (int i = t; i < OLC * OLW; i += NT) ol_bin[i / OLW][i % OLW] = 0.0;
  }
  const double inv_sigma = KIND == 1 ? 1.0 / ab[1 + M] : 0.0;
  const double phi = KIND == 3 ? ab[1 + M] : 0.0;
  const double log_phi = KIND == 3 ? log(phi) : 0.0;
  // no columns (M == 0, x may be null; the column clamp below would give -1):
  // every x load reads the zero page, for every kind
  const bool nox = M == 0;
  const double* __restrict__ xb = nox ? g_glm_zero : x;
  const long long ldc = nox ? 0 : ldx, rend = nox ? 1 : R;
  const long long ntiles = (R + RB - 1) / RB;
  double gacc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) gacc[q] = 0.0;
  double lp_acc = 0.0, ga_acc = 0.0, c_acc = 0.0;
  double b_acc = 0.0, d_acc = 0.0, f_acc = 0.0;  // KIND 3: B, D and phi'
  double xc[Q], xn[Q];
  double yc = 0.0, yn = 0.0;  // the row's y (as double), loaded one tile ahead with x
  double ac = 0.0, an = 0.0;  // AV: the row's intercept, loaded and carried with its y
  // Loads are straight-line code: addresses are clamped into x and the
  // values masked where they are consumed (a branch or a select next to a
  // load makes the compiler wait for it there), and y is issued before x so
  // that waiting for it leaves the x loads in flight (vmcnt counts in order);
  // so is the row's intercept (AV), at y's clamped row.
  auto load = [&](double (&v)[Q], double& yv_, double& av_, long long tile) {
    const long long gr = tile * RB + r;
    const size_t ry = (size_t)(gr < R ? gr : R - 1);
    const size_t rc = (size_t)(gr < rend ? gr : rend - 1);
    yv_ = KIND == 1 ? yd[ry] : (double)y[ry];
    if (AV) av_ = av[ry];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int c = g + G * q;
      const int cc = c < M ? c : M - 1;
      const double* px = xb + rc + (size_t)cc * ldc;
      v[q] = NTL ? __builtin_nontemporal_load(px) : *px;
    }
  };
  // one tile's work on the registers cur / cy (the other buffer's loads
  // stay in flight meanwhile); ping-pong buffers instead of a copy, which
  // would wait for the loads
  auto work = [&](double (&cur)[Q], double cy, double ca, long long tile, int buf) {
    const long long gr = tile * RB + r;
    const double al = AV ? ca : alpha;  // the row's intercept
#pragma unroll
    for (int q = 0; q < Q; ++q) cur[q] = (gr < R && g + G * q < M) ? cur[q] : 0.0;
    double e = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) e += cur[q] * beta[g + G * q];
    red[buf][g][r] = e;
    __syncthreads();
    double th = 0.0;
    if (gr < R) {
      double eta = 0.0;
#pragma unroll
      for (int k = 0; k < G; ++k) eta += red[buf][k][r];
      double lp;
      if (KIND == 0) {
        const double sgn = 2.0 * cy - 1.0;
        const double yt = sgn * (eta + al);
        const double ex = exp(-yt);
        lp = yt > 20.0 ? -ex : (yt < -20.0 ? yt : -log1p(ex));
        th = yt > 20.0 ? -ex : (yt < -20.0 ? sgn : sgn * ex / (ex + 1));
      } else if (KIND == 1) {
        const double ys = (cy - eta - al) * inv_sigma;
        lp = ys * ys;
        th = ys * inv_sigma;
      } else if (KIND == 2) {
        const double yi = cy;
        const double theta = eta + al;
        const double ex = exp(theta);
        lp = yi * theta - ex;
        th = yi - ex;
      } else if (KIND == 3) {
        const double yi = cy;
        const double theta = eta + al;
        const double d = theta - log_phi;
        const double e = exp(-fabs(d));  // in [0, 1]: never exp(theta) itself
        const double lse = fmax(theta, log_phi) + log1p(e);
        const double inv = 1.0 / (1.0 + e);
        const double s = d >= 0.0 ? inv : e * inv;
        const double s1 = d >= 0.0 ? e * inv : inv;  // 1 - s
        const double yp = yi + phi;
        lp = yp * lse;
        th = yi - yp * s;
        if (g == 0) {
          b_acc += yi * theta;
          f_acc += (1.0 - yp * s1 / phi) + (log_phi - lse);
        }
      } else {
        // the class, clamped into 1..C for the lookups (a y outside is the
        // caller's check; that row's result is unspecified)
        // Lanes l and l + 32 of a wave hold the same row (column groups 2w and
        // 2w + 1): the even group evaluates the upper cut-point's side, z = a,
        // the odd group the lower one's, z = -b, by the same code -- one exp
        // and one division per thread -- and a lane exchange brings the two
        // together, without a barrier.
        const int yk = (int)cy;
        const int k = yk < 1 ? 1 : (yk > C ? C : yk);
        const int side = g & 1;
        const bool on = side ? k > 1 : k < C;
        const double ck = ol_cut[k - side];
        const double z = side ? eta - ck : ck - eta;
        const double ez = exp(-fabs(z));  // in [0, 1]
        const double inv = 1.0 / (1.0 + ez);
        const double s = on ? (z <= 0.0 ? inv : ez * inv) : 0.0;  // [k < C] logistic(-a) / [k > 1] logistic(b)
        const double o = __shfl_xor(s, 32);
        th = side ? s - o : o - s;  // the same two operands on both lanes: the same bits
        lp = 0.0;
        if (g < 2) {  // wave 0: group 0 keeps ll(a) + lm and d_hi, group 1 ll(-b) and d_lo
          const double ll = on ? (z < 0.0 ? z : 0.0) - log1p(ez) : 0.0;
          lp_acc += side ? ll : ll + ol_lm[k];
          const double d = on ? s + ol_r[k] : 0.0;
          ol_bin[k - side][t] += side ? -d : d;  // this lane's own slot
        }
      }
      if (g == 0) {  // one thread per row accumulates the row's terms
        lp_acc += lp;
        ga_acc += th;
        if (KIND == 0) c_acc += (cy != 0.0 && cy != 1.0) ? 1.0 : 0.0;
        // lanes 0-31 of wave 0: one 256-byte segment per tile, rows >= R never.
        // Measured at 1e6 x 256: 1.06-1.09x the scalar kernel's time with the
        // store, 1.00-1.06x without.  Stored one tile late instead (behind the
        // next tile's loads, th and gr carried in registers): 1.07-1.10x, and
        // 1.01-1.09x without the store -- not kept.
        if (AV)
          if (thp) thp[gr] = th;
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) gacc[q] += th * cur[q];
  };
  __syncthreads();  // beta
  long long tile = blockIdx.x;
  const long long gs = gridDim.x;
  auto clampt = [&](long long tt) { return tt < ntiles ? tt : tile; };
  {
    if (tile < ntiles) load(xc, yc, ac, tile);
    for (;;) {
      if (tile >= ntiles) break;
      load(xn, yn, an, clampt(tile + gs));
      work(xc, yc, ac, tile, 0);
      tile += gs;
      if (tile >= ntiles) break;
      load(xc, yc, ac, clampt(tile + gs));
      work(xn, yn, an, tile, 1);
      tile += gs;
    }
  }
  if (KIND == 2)  // sum of lgamma(y + 1) over this workgroup's rows, off the streaming loop
    for (long long k = t / RB;; k += NT / RB) {
      const long long tl2 = blockIdx.x + k * gridDim.x;
      if (tl2 >= ntiles) break;
      const long long gr = tl2 * RB + r;
      if (gr < R) c_acc += lgamma((double)y[gr] + 1.0);
    }
  if (KIND == 3) {  // the terms of y and phi alone, off the streaming loop, over all threads
    const double dg_phi = dev_digamma(phi);
    for (long long k = t / RB;; k += NT / RB) {
      const long long tl2 = blockIdx.x + k * gridDim.x;
      if (tl2 >= ntiles) break;
      const long long gr = tl2 * RB + r;
      if (gr < R) {
        const double yi = (double)y[gr];
        c_acc += dev_lgamma(yi + 1.0);
        d_acc += dev_lgamma(yi + phi);
        f_acc += dev_digamma(yi + phi) - dg_phi;
      }
    }
  }
  // column sums over the RB rows of each column group: RB adjacent lanes
#pragma unroll
  for (int q = 0; q < Q; ++q)
    for (int off = RB / 2; off > 0; off >>= 1) gacc[q] += __shfl_xor(gacc[q], off, RB);
  const bool extra = KIND == 2 || (KIND == 0 && check_y);
  const int W = KIND == 4 ? M + C : (KIND == 3 ? M + 6 : M + 2 + (extra ? 1 : 0));
  double* p = part + (size_t)blockIdx.x * W;
  __syncthreads();
  const double lp = block_sum(lp_acc, lds);
  if (KIND == 4) {  // [logp, beta'(M), cuts'(C - 1)]: no intercept slot
    if (t == 0) p[0] = lp;
    if (t >= NT - 64 && t - (NT - 64) < C - 1) {  // cuts'[j]: wave 0's 64 slots of bin j + 1, in lane order
      const int j = t - (NT - 64);
      double cs = 0.0;
      for (int l = 0; l < OLW; ++l) cs += ol_bin[j + 1][l];
      p[1 + M + j] = cs;
    }
    if (r == 0)
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int c = g + G * q;
        if (c < M) p[1 + c] = gacc[q];
      }
    return;
  }
  __syncthreads();
  const double ga = block_sum(ga_acc, lds);
  double cs = 0.0;
  if (extra) {
    __syncthreads();
    cs = block_sum(c_acc, lds);
  }
  if (t == 0) {
    p[0] = lp;
    p[1] = ga;
    if (extra) p[M + 2] = cs;
  }
  if (KIND == 3) {  // [.., B, C, D, phi'] behind beta'
    __syncthreads();
    const double bs = block_sum(b_acc, lds);
    __syncthreads();
    const double c3 = block_sum(c_acc, lds);
    __syncthreads();
    const double ds = block_sum(d_acc, lds);
    __syncthreads();
    const double fs = block_sum(f_acc, lds);
    if (t == 0) {
      p[M + 2] = bs;
      p[M + 3] = c3;
      p[M + 4] = ds;
      p[M + 5] = fs;
    }
  }
  if (r == 0)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int c = g + G * q;
      if (c < M) p[2 + c] = gacc[q];
    }
}

template <int KIND, int RB, int NT, bool NTL = false>
__global__ __launch_bounds__(NT) void k_glm_reg(const void* __restrict__ yv, const double* __restrict__ x,
                                                long long R, int M, long long ldx, const double* __restrict__ ab,
                                                double* __restrict__ part, int check_y = 0) {
  glm_reg_body<KIND, RB, NT, NTL>(yv, x, R, M, ldx, ab, part, check_y);
}

// the vector-intercept form (KIND 0-3): av[R] per-row intercepts, thp[R] the
// rows' theta' (null: not stored); ab[0] is not read
template <int KIND, int RB, int NT, bool NTL = false>
__global__ __launch_bounds__(NT) void k_glm_reg_av(const void* __restrict__ yv, const double* __restrict__ x,
                                                   long long R, int M, long long ldx,
                                                   const double* __restrict__ ab, double* __restrict__ part,
                                                   int check_y, const double* __restrict__ av,
                                                   double* __restrict__ thp) {
  glm_reg_body<KIND, RB, NT, NTL, true>(yv, x, R, M, ldx, ab, part, check_y, av, thp);
}

// [alpha, beta(M)] as a kernel argument: the launch carries the parameters,
// no host-to-device copy ahead of it
struct glm_ab_arg {
  double v[MMAX + 1];
};

// The latency-bound form of k_glm_reg (KIND 0, y-bounds count on) takes the
// parameters from the kernel arguments of a one-workgroup copy ahead of it
// (no host-to-device copy).  The kernel arguments live in host memory: the
// streaming kernel reading them directly (every workgroup, 8 B at a time
// over the bus) measured 0.44 -> 0.53 ms at 1.25e6 rows.
__global__ __launch_bounds__(256) void k_glm_params(glm_ab_arg a, int n, double* __restrict__ dst) {
  for (int i = threadIdx.x; i < n; i += 256) dst[i] = a.v[i];
}

// ...and its finish: one workgroup per output column c sums column c of the
// per-workgroup partials (the order of k_reduce_partials: the same bits as
// the staged path), writes out[c] (device) and out_h[c] (pinned host), and
// takes a ticket; the last workgroup publishes seq to the host completion
// word, so the host spins on it instead of a copy back and a stream
// synchronisation.  (One workgroup summing all M + 3 columns measured 84 us
// at M = 256 -- 1 MB of partials through one CU -- against 4.7 us here.)
__global__ __launch_bounds__(256) void k_glm_io_final(const double* __restrict__ part, int nb, int W, double* out,
                                                      double* out_h, unsigned int* counter, long long* done,
                                                      long long seq) {
  __shared__ double lds[16];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) s += part[(size_t)i * W + c];
  s = block_sum(s, lds);
  if (threadIdx.x != 0) return;
  out[c] = s;
  if (!out_h) return;
  // a system-scope store goes to host memory directly; the ticket's
  // system-scope release orders it (and out[c]) before this workgroup's
  // arrival, the last arrival's acquire orders every column before done
  __hip_atomic_store(out_h + c, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM) != gridDim.x - 1) return;
  __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// rows per tile (measured on MI355X: 16 rows 4.3 TB/s, 32 rows 5.1, 64 rows 4.0).
// Also measured and rejected: 16-byte loads (two rows per lane) 4.8 TB/s vs
// 5.0 for 8-byte loads; contiguous per-workgroup tile ranges 3.9 TB/s (the
// interleaved order keeps concurrently running workgroups on adjacent
// segments of every column)
constexpr int GLM_RB = 32;

int glm_blocks(long long R) {
  const long long ntiles = (R + GLM_RB - 1) / GLM_RB;
  // LDS-limited workgroups per CU x 256 CUs (32 rows: 67.6 KB, 2 per CU; 16 rows: 34.8 KB, 4 per CU)
  long long nb = GLM_RB == 16 ? 1024 : (GLM_RB == 32 ? 512 : 256);
  if (nb > ntiles) nb = ntiles;
  if (nb < 1) nb = 1;
  return (int)nb;
}

// check_y: KIND 0's y-bounds count; KIND 4's number of classes
template <int KIND>
int glm_launch(hipStream_t st, const void* y, const double* x, long long R, int M, long long ldx,
               const double* ab, double* ws, int check_y = 0) {
  const int nb = glm_blocks(R);
  hipLaunchKernelGGL((k_glm_reg<KIND, 32, 512, true>), dim3(nb), dim3(512), 0, st, y, x, R, M, ldx, ab, ws, check_y);
  return nb;
}

template <int KIND>
int glm_launch_av(hipStream_t st, const void* y, const double* x, long long R, int M, long long ldx,
                  const double* ab, double* ws, int check_y, const double* av, double* thp) {
  const int nb = glm_blocks(R);
  hipLaunchKernelGGL((k_glm_reg_av<KIND, 32, 512, true>), dim3(nb), dim3(512), 0, st, y, x, R, M, ldx, ab, ws, check_y,
                     av, thp);
  return nb;
}

// ------------------------------------------------ categorical_logit_glm_lpmf
// prim/mat/prob/categorical_logit_glm_lpmf.hpp:38-146 (x an N x M matrix,
// alpha C, beta M x C, y in 1..C), ONE pass over x in 16-row tiles:
//   lin = x beta + alpha;  logp = sum_i lin(i, y_i - 1) - max_i - log sum exp(lin_i - max_i)
//   theta'(i, c) = [c == y_i - 1] - softmax(lin_i)_c
//   alpha' = sum_i theta'(i, :),  beta' = x^T theta'
// (the reference's neg_softmax_lin plus the one-hot terms, :117-143).
// Per-workgroup partial [logp, alpha'(C), beta'(M x C col-major)], reduced in
// fixed order.  M <= 256, C <= CAT_CMAX.
constexpr int CAT_RB = 16;
constexpr int CAT_CMAX = 16;

__global__ __launch_bounds__(256) void k_glm_categorical(const int* __restrict__ y,
                                                         const double* __restrict__ x, long long R,
                                                         int M, long long ldx, int C,
                                                         const double* __restrict__ ab,
                                                         double* __restrict__ part) {
  constexpr int RB = CAT_RB, XS = RB + 1;
  constexpr int PER = RB * MMAX / 256;
  __shared__ double X[MMAX * XS];
  __shared__ double beta[MMAX * CAT_CMAX];  // beta[m * CAT_CMAX + c]
  __shared__ double alpha[CAT_CMAX];
  __shared__ double lin[RB * CAT_CMAX];     // then theta'
  __shared__ double lds[16];
  const int t = threadIdx.x;
  for (int e = t; e < M * C; e += 256) beta[(e % M) * CAT_CMAX + e / M] = ab[C + e];  // ab = [alpha(C), beta(M x C)]
  if (t < C) alpha[t] = ab[t];
  const long long ntiles = (R + RB - 1) / RB;
  double gacc[CAT_CMAX];  // column t of beta': one accumulator per class
#pragma unroll
  for (int c = 0; c < CAT_CMAX; ++c) gacc[c] = 0.0;
  double lp_acc = 0.0, ga_acc = 0.0;  // rows' logp (t < RB) / class t's alpha' (t < C)
  double reg[PER];
  auto load = [&](long long tile) {
    const long long r0 = tile * RB;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = t + 256 * q;
      const int r = e % RB, c = e / RB;
      const long long gr = r0 + r;
      reg[q] = *((c < M && gr < R) ? x + gr + (size_t)c * ldx : g_glm_zero);
    }
  };
  long long tile = blockIdx.x;
  if (tile < ntiles) load(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // previous tile fully consumed
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = t + 256 * q;
      X[(e / RB) * XS + (e % RB)] = reg[q];
    }
    __syncthreads();
    const long long next = tile + gridDim.x;
    if (next < ntiles) load(next);  // in flight during the compute below
    if (t < RB * C) {  // lin(r, c)
      const int r = t % RB, c = t / RB;
      double s = 0.0;
      for (int m = 0; m < M; ++m) s += X[m * XS + r] * beta[m * CAT_CMAX + c];
      lin[r * CAT_CMAX + c] = s + alpha[c];
    }
    __syncthreads();
    if (t < RB) {  // the row's softmax, logp and theta'
      const long long gr = tile * RB + t;
      if (gr < R) {
        double mx = lin[t * CAT_CMAX];
        for (int c = 1; c < C; ++c) mx = fmax(mx, lin[t * CAT_CMAX + c]);
        double se = 0.0;
        for (int c = 0; c < C; ++c) se += exp(lin[t * CAT_CMAX + c] - mx);
        const double inv = 1.0 / se;
        const int yc = y[gr] - 1;
        lp_acc += log(inv) - mx + lin[t * CAT_CMAX + yc];
        for (int c = 0; c < C; ++c)
          lin[t * CAT_CMAX + c] = (c == yc ? 1.0 : 0.0) - exp(lin[t * CAT_CMAX + c] - mx) * inv;
      } else {
        for (int c = 0; c < C; ++c) lin[t * CAT_CMAX + c] = 0.0;
      }
    }
    __syncthreads();
    if (t < C) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < RB; ++r) s += lin[r * CAT_CMAX + t];
      ga_acc += s;
    }
    if (t < M) {
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const double xv = X[t * XS + r];
#pragma unroll
        for (int c = 0; c < CAT_CMAX; ++c)
          if (c < C) gacc[c] += xv * lin[r * CAT_CMAX + c];
      }
    }
  }
  const int W = 1 + C + M * C;
  double* p = part + (size_t)blockIdx.x * W;
  __syncthreads();
  const double lp = block_sum(lp_acc, lds);
  if (t == 0) p[0] = lp;
  if (t < C) p[1 + t] = ga_acc;
  if (t < M)
#pragma unroll
    for (int c = 0; c < CAT_CMAX; ++c)
      if (c < C) p[1 + C + (size_t)c * M + t] = gacc[c];
}

int glm_cat_blocks(long long R) {
  const long long ntiles = (R + CAT_RB - 1) / CAT_RB;
  long long nb = 512;
  if (nb > ntiles) nb = ntiles;
  if (nb < 1) nb = 1;
  return (int)nb;
}

// ------------------------------------------------ generic path (M > 256)
// the intercept of row i: one scalar by value, or av[i], with theta' then also
// stored to thp[i] unless thp is null (th feeds the x^T theta' GEMM)
struct glm_rows_av {
  const double* __restrict__ av;
  double* __restrict__ thp;
};

template <bool AV>
__global__ void k_glm_rows(const int* __restrict__ y, const double* __restrict__ eta, long long R,
                           std::conditional_t<AV, glm_rows_av, double> alpha, double* __restrict__ th, double* part) {
  __shared__ double lds[16];
  double lp = 0.0, ga = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < R;
       i += (long long)gridDim.x * blockDim.x) {
    const double sgn = 2.0 * y[i] - 1.0;
    double a;
    if constexpr (AV) a = alpha.av[i];
    else a = alpha;
    const double yt = sgn * (eta[i] + a);
    const double e = exp(-yt);
    lp += yt > 20.0 ? -e : (yt < -20.0 ? yt : -log1p(e));
    const double d = yt > 20.0 ? -e : (yt < -20.0 ? sgn : sgn * e / (e + 1));
    th[i] = d;
    if constexpr (AV)
      if (alpha.thp) alpha.thp[i] = d;
    ga += d;
  }
  lp = block_sum(lp, lds);
  __syncthreads();
  ga = block_sum(ga, lds);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = lp;
    part[2 * blockIdx.x + 1] = ga;
  }
}

// categorical generic path (M > 256 or C > 16): lin = x beta by GEMM, then one
// thread per row turns lin(i, :) (column-major, ld R) into theta'(i, :) in
// place and accumulates the row's logp; alpha' and beta' by GEMM.
__global__ void k_glm_cat_rows(const int* __restrict__ y, double* __restrict__ lin, long long R, int C,
                               const double* __restrict__ alpha, double* __restrict__ ones,
                               double* __restrict__ part) {
  __shared__ double lds[16];
  double lp = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < R;
       i += (long long)gridDim.x * blockDim.x) {
    double mx = -INFINITY;
    for (int c = 0; c < C; ++c) {
      const double v = lin[i + (size_t)c * R] + alpha[c];
      lin[i + (size_t)c * R] = v;
      mx = fmax(mx, v);
    }
    double se = 0.0;
    for (int c = 0; c < C; ++c) se += exp(lin[i + (size_t)c * R] - mx);
    const double inv = 1.0 / se;
    const int yc = y[i] - 1;
    lp += log(inv) - mx + lin[i + (size_t)yc * R];
    for (int c = 0; c < C; ++c) {
      const double v = lin[i + (size_t)c * R];
      lin[i + (size_t)c * R] = (c == yc ? 1.0 : 0.0) - exp(v - mx) * inv;
    }
    ones[i] = 1.0;
  }
  lp = block_sum(lp, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = lp;
}

// bernoulli_logit at M > 256: eta = x beta (GEMM n = 1), theta' per row, beta'
// = x^T theta'; out = [logp, alpha', beta'(M)].  av null: the scalar intercept
// ab[0], fetched to the host between the GEMM and the row kernel.
int glm_bernoulli_generic(smg_ctx* ctx, const int* y, const double* x, long long R, int M, long long ldx,
                          const double* ab, const double* av, double* thp, double* ws, double* out) {
  double* eta = ws;
  double* th = ws + R;
  double* part = ws + 2 * R;
  int rc = smg_gemm_impl(ctx, 0, 0, 0, (int)R, 1, M, 1.0, x, (int)ldx, ab + 1, M, 0.0, eta, (int)R);
  if (rc) return rc;
  if (av) {
    hipLaunchKernelGGL(k_glm_rows<true>, dim3(1024), dim3(256), 0, ctx->stream, y, eta, R, glm_rows_av{av, thp}, th,
                       part);
  } else {
    double alpha_h;
    rc = smg_memcpy_d2h(ctx, &alpha_h, ab, sizeof(double));
    if (rc) return rc;
    rc = smg_sync(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_glm_rows<false>, dim3(1024), dim3(256), 0, ctx->stream, y, eta, R, alpha_h, th, part);
  }
  smg_reduce_partials(ctx, part, 1024, 2, out, 0);
  rc = smg_gemm_impl(ctx, 1, 0, 0, M, 1, (int)R, 1.0, x, (int)ldx, th, (int)R, 0.0, out + 2, M);
  SMG_LAUNCH_CHECK();
  return rc;
}

// every entry's data arguments: rows need y, columns need x with ldx >= R
bool glm_bad_data(const void* y, const double* x, long long R, int M, long long ldx) {
  return R > 0 && (!y || (M > 0 && (!x || ldx < R)));
}

}  // namespace

extern "C" {

long long smg_glm_ws_doubles(long long R, int M) {
  if (M <= MMAX) return (long long)glm_blocks(R) * (M + 3);
  return 2 * R + 2 * 1024;
}

int smg_bernoulli_logit_glm(smg_ctx* ctx, const int* y, const double* x, long long R, int M,
                            long long ldx, const double* ab, double* ws, double* out) {
  if (!ctx || R < 0 || M < 0 || !ab || !ws || !out) return SMG_ERR_ARG;
  if (glm_bad_data(y, x, R, M, ldx)) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GLM);
  if (M <= MMAX) {
    const int nb = glm_launch<0>(ctx->stream, y, x, R, M, ldx, ab, ws);
    smg_reduce_partials(ctx, ws, nb, M + 2, out, 0);
    SMG_LAUNCH_CHECK();
    return SMG_OK;
  }
  return glm_bernoulli_generic(ctx, y, x, R, M, ldx, ab, nullptr, nullptr, ws, out);
}

int smg_bernoulli_logit_glm_checked(smg_ctx* ctx, const int* y, const double* x, long long R, int M,
                                    long long ldx, const double* ab, double* ws, double* out) {
  if (!ctx || R < 0 || M < 0 || !ab || !ws || !out) return SMG_ERR_ARG;
  if (glm_bad_data(y, x, R, M, ldx)) return SMG_ERR_ARG;
  if (M > MMAX || R == 0) {  // the general path: a separate bound check
    int rc = smg_memset(ctx, out + M + 2, 0, sizeof(double));
    if (!rc) rc = smg_check_bounded_int(ctx, y, R, 0, 1, out + M + 2);
    if (!rc) rc = R > 0 ? smg_bernoulli_logit_glm(ctx, y, x, R, M, ldx, ab, ws, out)
                        : smg_memset(ctx, out, 0, sizeof(double) * (M + 2));
    return rc;
  }
  smg_prof_scope prof(ctx, SMG_FAM_GLM);
  const int nb = glm_launch<0>(ctx->stream, y, x, R, M, ldx, ab, ws, 1);
  smg_reduce_partials(ctx, ws, nb, M + 3, out, 0);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_bernoulli_logit_glm_io(smg_ctx* ctx, const int* y, const double* x, long long R, int M, long long ldx,
                               double alpha, const double* beta, double* ws, double* out, double* out_h) {
  if (!ctx || R < 0 || M < 0 || !ws || !out || (M > 0 && !beta)) return SMG_ERR_ARG;
  if (glm_bad_data(y, x, R, M, ldx)) return SMG_ERR_ARG;
  if (M > MMAX || R == 0) {  // the general path, then one copy back and a synchronisation
    double* ab = smg_ws(ctx, SMG_WS_GLM, (size_t)M + 1);
    double* h = (double*)smg_host_scratch(ctx, sizeof(double) * (M + 1));
    if (!ab || !h) return SMG_ERR_OOM;
    h[0] = alpha;
    for (int j = 0; j < M; ++j) h[1 + j] = beta[j];
    int rc = smg_memcpy_h2d(ctx, ab, h, sizeof(double) * (M + 1));
    if (!rc) rc = smg_bernoulli_logit_glm_checked(ctx, y, x, R, M, ldx, ab, ws, out);
    if (!rc && out_h) rc = smg_memcpy_d2h(ctx, out_h, out, sizeof(double) * (M + 3));
    if (!rc) rc = smg_sync(ctx);  // the scratch upload has been read
    return rc;
  }
  glm_ab_arg a;
  a.v[0] = alpha;
  for (int j = 0; j < M; ++j) a.v[1 + j] = beta[j];
  const int nb = glm_blocks(R);
  const long long seq = out_h ? ++ctx->done_seq : 0;
  {  // (the profiling scope closes before the host waits)
    smg_prof_scope prof(ctx, SMG_FAM_GLM);
    double* ab = smg_ws(ctx, SMG_WS_GLM, MMAX + 1);
    if (!ab) return SMG_ERR_OOM;
    hipLaunchKernelGGL(k_glm_params, dim3(1), dim3(256), 0, ctx->stream, a, M + 1, ab);
    hipLaunchKernelGGL((k_glm_reg<0, GLM_RB, 512, true>), dim3(nb), dim3(512), 0, ctx->stream, y, x, R, M, ldx, ab, ws, 1);
    hipLaunchKernelGGL(k_glm_io_final, dim3(M + 3), dim3(256), 0, ctx->stream, ws, nb, M + 3, out, out_h,
                       ctx->red_counter_d + 1, out_h ? ctx->done_h : nullptr, seq);
    SMG_LAUNCH_CHECK();
  }
  return out_h ? smg_wait_done(ctx, seq) : SMG_OK;
}

long long smg_glm_categorical_ws_doubles(long long R, int M, int C) {
  if (M <= MMAX && C <= CAT_CMAX) return (long long)glm_cat_blocks(R) * (1 + C + (long long)M * C);
  return R * ((long long)C + 1) + 1024;
}

int smg_categorical_logit_glm(smg_ctx* ctx, const int* y, const double* x, long long R, int M,
                              long long ldx, int C, const double* alpha_beta, double* ws,
                              double* out) {
  if (!ctx || R < 0 || M < 0 || C < 1 || !alpha_beta || !ws || !out) return SMG_ERR_ARG;
  if (glm_bad_data(y, x, R, M, ldx)) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GLM);
  if (M <= MMAX && C <= CAT_CMAX) {
    const int nb = glm_cat_blocks(R);
    hipLaunchKernelGGL(k_glm_categorical, dim3(nb), dim3(256), 0, ctx->stream, y, x, R, M, ldx, C,
                       alpha_beta, ws);
    smg_reduce_partials(ctx, ws, nb, 1 + C + M * C, out, 0);
    SMG_LAUNCH_CHECK();
    return SMG_OK;
  }
  if (R > INT_MAX || (long long)M * C > INT_MAX) return SMG_ERR_ARG;  // GEMM dimensions
  if (R == 0) return smg_memset(ctx, out, 0, sizeof(double) * (1 + C + (size_t)M * C));
  double* lin = ws;                         // R x C
  double* ones = ws + R * (long long)C;     // R
  double* part = ones + R;                  // 1024
  int rc = smg_gemm_impl(ctx, 0, 0, 0, (int)R, C, M, 1.0, x, (int)ldx, alpha_beta + C, M > 0 ? M : 1,
                         0.0, lin, (int)R);
  if (rc) return rc;
  hipLaunchKernelGGL(k_glm_cat_rows, dim3(1024), dim3(256), 0, ctx->stream, y, lin, R, C, alpha_beta,
                     ones, part);
  smg_reduce_partials(ctx, part, 1024, 1, out, 0);
  rc = smg_gemm_impl(ctx, 1, 0, 0, C, 1, (int)R, 1.0, lin, (int)R, ones, (int)R, 0.0, out + 1, C);
  if (rc) return rc;
  if (M > 0) rc = smg_gemm_impl(ctx, 1, 0, 0, M, C, (int)R, 1.0, x, (int)ldx, lin, (int)R, 0.0, out + 1 + C, M);
  SMG_LAUNCH_CHECK();
  return rc;
}

// normal_id_glm_lpdf / poisson_log_glm_lpmf: the fused pass (M <= 256)
int smg_normal_id_glm(smg_ctx* ctx, const double* y, const double* x, long long R, int M,
                      long long ldx, const double* abs, double* ws, double* out) {
  if (!ctx || R < 0 || M < 0 || M > MMAX || !abs || !ws || !out) return SMG_ERR_ARG;
  if (glm_bad_data(y, x, R, M, ldx)) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GLM);
  const int nb = glm_launch<1>(ctx->stream, y, x, R, M, ldx, abs, ws);
  smg_reduce_partials(ctx, ws, nb, M + 2, out, 0);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

int smg_poisson_log_glm(smg_ctx* ctx, const int* y, const double* x, long long R, int M,
                        long long ldx, const double* ab, double* ws, double* out) {
  if (!ctx || R < 0 || M < 0 || M > MMAX || !ab || !ws || !out) return SMG_ERR_ARG;
  if (glm_bad_data(y, x, R, M, ldx)) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GLM);
  const int nb = glm_launch<2>(ctx->stream, y, x, R, M, ldx, ab, ws);
  smg_reduce_partials(ctx, ws, nb, M + 3, out, 0);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

// neg_binomial_2_log_glm_lpmf: the fused pass (M <= 256), partial width M + 6
long long smg_neg_binomial_2_log_glm_ws_doubles(long long R, int M) {
  return (long long)glm_blocks(R) * ((M > 0 ? M : 0) + 6);
}

int smg_neg_binomial_2_log_glm(smg_ctx* ctx, const int* y, const double* x, long long R, int M,
                               long long ldx, const double* abp, double* ws, double* out) {
  if (!ctx || R < 0 || M < 0 || M > MMAX || !abp || !ws || !out) return SMG_ERR_ARG;
  if (glm_bad_data(y, x, R, M, ldx)) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GLM);
  const int nb = glm_launch<3>(ctx->stream, y, x, R, M, ldx, abp, ws);
  smg_reduce_partials(ctx, ws, nb, M + 6, out, 0);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

// One intercept per row (kinds 0-3): the same fused pass with alpha_vec[R] in
// place of ab[0]; theta_adj[R] (may be null) receives the rows' theta', the
// partials of their intercepts.  `out` as the kind's scalar entry lays it out
// (kind 0: the _checked form).
int smg_glm_vec_intercept(smg_ctx* ctx, int kind, const void* y, const double* x, long long R, int M,
                          long long ldx, const double* alpha_vec, const double* ab, double* ws, double* out,
                          double* theta_adj) {
  if (!ctx || kind < 0 || kind > 3 || R < 0 || M < 0 || !ab || !ws || !out) return SMG_ERR_ARG;
  if (kind != 0 && M > MMAX) return SMG_ERR_ARG;
  if (glm_bad_data(y, x, R, M, ldx) || (R > 0 && !alpha_vec)) return SMG_ERR_ARG;
  const int W = kind == 3 ? M + 6 : (kind == 1 ? M + 2 : M + 3);
  if (R == 0) return smg_memset(ctx, out, 0, sizeof(double) * W);
  if (M > MMAX) {  // kind 0's generic path
    if (R > INT_MAX) return SMG_ERR_ARG;  // GEMM dimensions
    int rc = smg_memset(ctx, out + M + 2, 0, sizeof(double));
    if (!rc) rc = smg_check_bounded_int(ctx, static_cast<const int*>(y), R, 0, 1, out + M + 2);
    if (rc) return rc;
    smg_prof_scope prof(ctx, SMG_FAM_GLM);
    return glm_bernoulli_generic(ctx, static_cast<const int*>(y), x, R, M, ldx, ab, alpha_vec, theta_adj, ws, out);
  }
  smg_prof_scope prof(ctx, SMG_FAM_GLM);
  int nb;
  switch (kind) {
    case 0: nb = glm_launch_av<0>(ctx->stream, y, x, R, M, ldx, ab, ws, 1, alpha_vec, theta_adj); break;
    case 1: nb = glm_launch_av<1>(ctx->stream, y, x, R, M, ldx, ab, ws, 0, alpha_vec, theta_adj); break;
    case 2: nb = glm_launch_av<2>(ctx->stream, y, x, R, M, ldx, ab, ws, 0, alpha_vec, theta_adj); break;
    default: nb = glm_launch_av<3>(ctx->stream, y, x, R, M, ldx, ab, ws, 0, alpha_vec, theta_adj); break;
  }
  smg_reduce_partials(ctx, ws, nb, W, out, 0);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

// ordered_logistic_glm_lpmf: the fused pass (M <= 256, C <= 16), partial width M + C
long long smg_ordered_logistic_glm_ws_doubles(long long R, int M, int C) {
  return (long long)glm_blocks(R) * ((M > 0 ? M : 0) + (C > 1 ? C : 1));
}

int smg_ordered_logistic_glm(smg_ctx* ctx, const int* y, const double* x, long long R, int M,
                             long long ldx, int C, const double* bc, double* ws, double* out) {
  if (!ctx || R < 0 || M < 0 || M > MMAX || C < 1 || C > OL_CMAX || !bc || !ws || !out) return SMG_ERR_ARG;
  if (glm_bad_data(y, x, R, M, ldx)) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GLM);
  const int nb = glm_launch<4>(ctx->stream, y, x, R, M, ldx, bc, ws, C);
  smg_reduce_partials(ctx, ws, nb, M + C, out, 0);
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

}  // extern "C"
