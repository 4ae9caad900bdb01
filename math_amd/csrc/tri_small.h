// Dense kernels on ONE 64 x 64 diagonal block held in LDS by one 512-thread
// workgroup (8 waves).  Everything here is instantiated by a kernel of the
// library; variants that were measured and dropped live in
// tools/ubench_variants.h, beside the microbenchmarks that timed them.
//
//   LDS products        lds_mma64_8w            k_chol_panel (owners, inverter), k_symbolic_rev
//                       lds_mma32_8w(_acc)      k_chol_panel (the 32-row tiles below a panel)
//                       lds_syrk64_8w_next      k_chol_panel (chain: the next diagonal block)
//   factor, per pivot   lds_potrf64_lookahead   k_potrf_diag (through lds_potrf_inv64_blk)
//   factor, pivot pairs lds_potrf64_chain       k_chol_panel (chain_factor)
//   inverse             lds_trtri64_mfma        k_chol_panel and lds_potrf_inv64_blk; its pieces
//                       trtri_leaf16 / trtri_t_acc / trtri_t_store / trtri_x_tile and
//                       leaf16_store also singly in k_chol_panel's chain
//   row solve           lds_trsm64_rt           k_chol_panel (chain and tiles)
//   factor + inverse    lds_potrf_inv64_blk     k_potrf_diag, k_trtri_diag (cholesky.hip),
//                                               k_trtri_blocks (tri.hip), k_lu_unit_inv (lu.hip)
//   block loads         lds_load_block(0)       k_potrf_diag, k_trtri_diag, k_symbolic_rev
//
// Layout: row-major [r][c] with stride SMG_NBP = 65 doubles.
// Latency structure (the block is on the critical path of every blocked
// algorithm, so latency, not throughput, is what matters here):
//   * 8-column panels and 16 x 16 leaves live in the registers of ONE wave
//     (lane i = row i or column i); broadcasts are v_readlane_b32 pairs, no
//     LDS round trips;
//   * everything between them is a 64 x 64 (or smaller) product on the fp64
//     matrix cores (v_mfma_f64_16x16x4_f64).
#pragma once
#include "blk_sizes.h"
#include "smg_internal.h"

__device__ __forceinline__ double bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// ---------------------------------------------------------------------------
// Products of 64 x 64 (and 32 x 64) LDS blocks on the matrix cores, 8 waves.
// Every thread of the workgroup must call them.

// C (64x64) = alpha op(A) op(B) + beta C, all LDS [r][c] stride 65: wave w
// owns row stripe w & 3 and column tiles 2 (w >> 2) .. +1.  Safe when C
// aliases A or B (barrier between the MFMA loop and the store).
template <bool TA, bool TB, typename P = double*, typename CP = const double*>
__device__ inline void lds_mma64_8w(P C, CP A, CP B, double alpha = 1.0, double beta = 0.0) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = l & 15, fk = l >> 4;
  const int i = 16 * (w & 3) + fr, t0 = 2 * (w >> 2);
  d4 acc[2];
  acc[0] = d4{0.0, 0.0, 0.0, 0.0};
  acc[1] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int k0 = 0; k0 < SMG_NB; k0 += 4) {
    const int kk = k0 + fk;
    const double a = TA ? A[kk * SMG_NBP + i] : A[i * SMG_NBP + kk];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = 16 * (t0 + t) + fr;
      const double b = TB ? B[j * SMG_NBP + kk] : B[kk * SMG_NBP + j];
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      auto c = &C[(16 * (w & 3) + fk + 4 * r) * SMG_NBP + 16 * (t0 + t) + fr];
      *c = beta == 0.0 ? alpha * acc[t][r] : alpha * acc[t][r] + beta * *c;
    }
  __syncthreads();
}

// The 32-row tiles below a panel: C = alpha A B^T + beta C with A, C 32 x 64
// (rows 0 .. 31 of the 64-row LDS layout), B 64 x 64.  8 waves: wave w owns
// row stripe w & 1 and column tile w >> 1 (one accumulator; the SIMD's two
// waves interleave).  Each element's k order is lds_mma64_8w's.  Safe when C
// aliases A.
template <typename P, typename CP>
__device__ inline void lds_mma32_8w(P C, CP A, CP B, double alpha = 1.0, double beta = 0.0) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = l & 15, fk = l >> 4;
  const int i = 16 * (w & 1) + fr, j = 16 * (w >> 1) + fr;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int k0 = 0; k0 < SMG_NB; k0 += 4) {
    const int kk = k0 + fk;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[i * SMG_NBP + kk], B[j * SMG_NBP + kk], acc, 0, 0, 0);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    auto c = &C[(16 * (w & 1) + fk + 4 * r) * SMG_NBP + 16 * (w >> 1) + fr];
    *c = beta == 0.0 ? alpha * acc[r] : alpha * acc[r] + beta * *c;
  }
  __syncthreads();
}

// This wave's 16 x 16 tile of the 32 x 64 product A B^T (A: 32 x 64, B:
// 64 x 64 in LDS), returned in the accumulator layout lds_mma32_8w stores:
// lane l of wave w holds rows 16 (w & 1) + (l >> 4) + 4 r, column
// 16 (w >> 1) + (l & 15).  No barrier: the caller owns the ordering.
template <typename CP>
__device__ inline d4 lds_mma32_8w_acc(CP A, CP B) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = l & 15, fk = l >> 4;
  const int i = 16 * (w & 1) + fr, j = 16 * (w >> 1) + fr;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int k0 = 0; k0 < SMG_NB; k0 += 4) {
    const int kk = k0 + fk;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[i * SMG_NBP + kk], B[j * SMG_NBP + kk], acc, 0, 0, 0);
  }
  return acc;
}

// The panel chain's next diagonal block: C = C - A A^T (A, C: 64 x 64 in
// LDS), written straight in the factorisation's input form -- lower triangle,
// zero strict upper, identity padding beyond row / column b -- so no separate
// pass over C follows
template <typename P, typename CP>
__device__ inline void lds_syrk64_8w_next(P C, CP A, int b) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = l & 15, fk = l >> 4;
  const int i = 16 * (w & 3) + fr, t0 = 2 * (w >> 2);
  d4 acc[2];
  acc[0] = d4{0.0, 0.0, 0.0, 0.0};
  acc[1] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int k0 = 0; k0 < SMG_NB; k0 += 4) {
    const int kk = k0 + fk;
    const double a = A[i * SMG_NBP + kk];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = 16 * (t0 + t) + fr;
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, A[j * SMG_NBP + kk], acc[t], 0, 0, 0);
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * (w & 3) + fk + 4 * r, col = 16 * (t0 + t) + fr;
      auto c = &C[row * SMG_NBP + col];
      *c = col > row ? 0.0 : (row == col && row >= b ? 1.0 : *c - acc[t][r]);
    }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// Blocked 64x64 Cholesky in LDS (512 threads = 8 waves), 8-wide panels, with
// look-ahead.  Two walks share this structure and differ in how wave 0
// factors a panel: lds_potrf64_lookahead one pivot at a time (k_potrf_diag),
// lds_potrf64_chain below two at a time (the panel chain).
//   panel p (columns j0 = 8p .. j0+7): wave 0, lane i = row i holds the 8
//     panel values in registers; the pivot steps broadcast with v_readlane;
//     the column is scaled by the pivot's reciprocal root (Eigen LLT divides
//     by the root; same to ~1 ulp).
//   look-ahead: in iteration p, wave 0 applies panel p's rank-8 update to
//     panel p+1 and factors it, WHILE waves 1..7 apply panel p's update to
//     the columns right of panel p+1.  The serial pivot chain (wave 0)
//     overlaps the bulk of the trailing work; one barrier per panel.
// D: LDS [64][SMG_NBP], lower triangle holds A (identity padded); on exit the
// lower triangle holds L (strict upper untouched).  A pivot that is not
// positive and finite latches SMG_ERR_NOT_PD (check_pos_definite,
// prim/mat/err/check_pos_definite.hpp:77-81).

// wave 0: factor the 8 columns held in a[] (lane i = row i, rows < j0 hold
// 0), one pivot per step: l_jj = sqrt(pivot) via v_rsq_f64 + 2 Newton steps
// (~1 ulp).  The column's entries of rows j0+c are broadcast BEFORE the
// pivot's reciprocal root and scaled by it on every lane (the same product
// lane j0+c forms, so the same bits as broadcasting l_{j0+c}): one readlane
// less on the pivot chain
__device__ __forceinline__ void wave_factor8_reg(double (&a)[8], int j0, bool& bad) {
  const int i = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    double sc[8];
#pragma unroll
    for (int c = t + 1; c < 8; ++c) sc[c] = bcast(a[t], j0 + c);
    const double piv = bcast(a[t], j0 + t);
    bad |= !(piv > 0.0 && piv < INFINITY);
    double r = __builtin_amdgcn_rsq(piv);
    r = r * (1.5 - 0.5 * piv * r * r);
    r = r * (1.5 - 0.5 * piv * r * r);
    const double li = (i == j0 + t) ? piv * r : a[t] * r;
    a[t] = li;
#pragma unroll
    for (int c = t + 1; c < 8; ++c) a[c] -= li * (sc[c] * r);
  }
}

template <typename P>
__device__ __forceinline__ void wave_store8(P D, const double (&a)[8], int j0) {
  const int i = threadIdx.x & 63;
  if (i >= j0)
#pragma unroll
    for (int t = 0; t < 8; ++t)
      if (i >= j0 + t) D[i * SMG_NBP + j0 + t] = a[t];
}

// wave 0: load, factor (v_readlane broadcasts), store panel j0..j0+7
template <typename P>
__device__ __forceinline__ void wave_panel8_rl(P D, int j0, bool& bad) {
  const int i = threadIdx.x & 63;
  double a[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) a[t] = (i >= j0) ? D[i * SMG_NBP + j0 + t] : 0.0;
  wave_factor8_reg(a, j0, bad);
  wave_store8(D, a, j0);
}

// (templated on the pointer type: double* when inlined into a kernel, an
// address_space(3) pointer when called out of line)
template <typename P>
__device__ inline void lds_potrf64_lookahead(P D, int* status) {
  const int i = threadIdx.x & 63;
  const int g = threadIdx.x >> 6;
  bool bad = false;
  if (g == 0) wave_panel8_rl(D, 0, bad);
  __syncthreads();
  for (int p = 0; p < 7; ++p) {
    const int j0 = 8 * p, c1 = j0 + 8, c2 = j0 + 16;
    // (A) waves 1..7: panel p+1 (rows >= c1, 8 columns) -= panel p's rank-8
    //     update, one element per thread
    if (g > 0) {
      const int e = threadIdx.x - 64;
      const int r = c1 + (e >> 3), c = c1 + (e & 7);
      if (r < 64 && r >= c) {
        double v = D[r * SMG_NBP + c];
#pragma unroll
        for (int t = 0; t < 8; ++t) v -= D[r * SMG_NBP + j0 + t] * D[c * SMG_NBP + j0 + t];
        D[r * SMG_NBP + c] = v;
      }
    }
    __syncthreads();
    // (B) wave 0 factors panel p+1 while waves 1..7 update columns >= c2
    if (g == 0) {
      wave_panel8_rl(D, c1, bad);
    } else if (c2 < 64) {
      // rank-8 trailing update of rows/cols >= c2 on the matrix cores: 16x16
      // tiles (ti >= tj) from 16-tile t0 = c2/16, 2 MFMAs each (K = 8); only
      // entries with col >= c2 and row >= col are written back
      const int t0 = c2 >> 4, nt = 4 - t0, ntiles = nt * (nt + 1) / 2;
      const int fr = i & 15, fk = i >> 4;
      for (int q = g - 1; q < ntiles; q += 7) {
        int ti = 0, rem = q;
        while (rem > ti) {
          rem -= ti + 1;
          ++ti;
        }
        const int tj = rem + t0;
        ti += t0;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k0 = 0; k0 < 8; k0 += 4) {
          const double av = D[(16 * ti + fr) * SMG_NBP + j0 + k0 + fk];
          const double bv = D[(16 * tj + fr) * SMG_NBP + j0 + k0 + fk];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
        const int col = 16 * tj + fr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * ti + fk + 4 * r;
          if (col >= c2 && row >= col) D[row * SMG_NBP + col] -= acc[r];
        }
      }
    }
    __syncthreads();
  }
  if (bad) atomicOr(status, (int)SMG_ERR_NOT_PD);
}

// ---------------------------------------------------------------------------
// x^{-1/2} to ~1 ulp: v_rsq_f64 (about 2^-22 relative) and ONE third-order
// (Halley-type) correction r (1 + e/2 + 3 e^2 / 8), e = 1 - x r^2 -- four
// dependent operations instead of two Newton steps' eight
__device__ __forceinline__ double rsq_h(double x) {
  const double r = __builtin_amdgcn_rsq(x);
  const double t = x * r;
  const double e = __builtin_fma(-t, r, 1.0);
  const double s = r * e;
  const double p = __builtin_fma(0.375, e, 0.5);
  return __builtin_fma(s, p, r);
}

// wave 0: the 8 columns held in a[] two pivots at a time: for the 2x2
// diagonal block [[A, B], [B, C]] both reciprocal roots come from values
// known before either is taken -- r1 = A^{-1/2} and rp = (AC - B^2)^{-1/2},
// the second pivot's l22^{-1} = sqrt(A) rp = A r1 rp -- so the two rsq_h
// chains run side by side and the pivot chain is one root deep per PAIR of
// columns.  The later columns are updated with the factor's own entries
// broadcast from the lanes that form them (li0 / li1 of lane j0 + c are
// L[c][t] / L[c][t+1]): two FMAs per column and pair.  Not bit-identical to
// wave_factor8_reg (l22 from det / A instead of C - l21^2), same accuracy
// class.  PRE: the next pair's two columns' entries are broadcast first, the
// rest after their update.
template <bool PRE = true>
__device__ __forceinline__ void wave_factor8_pair2(double (&a)[8], int j0, bool& bad) {
#pragma unroll
  for (int t = 0; t < 8; t += 2) {
    const double A = bcast(a[t], j0 + t);
    const double B = bcast(a[t], j0 + t + 1);
    const double C = bcast(a[t + 1], j0 + t + 1);
    const double det = __builtin_fma(A, C, -(B * B));
    bad |= !(A > 0.0 && A < INFINITY) || !(det > 0.0 && det < INFINITY);
    const double r1 = rsq_h(A);
    const double rp = rsq_h(det);
    const double r2 = (A * r1) * rp;
    const double l21 = B * r1;
    const double li0 = a[t] * r1;
    const double li1 = (a[t + 1] - li0 * l21) * r2;
    a[t] = li0;
    a[t + 1] = li1;
    if (PRE && t + 2 < 8) {  // the next pair's columns first (its pivots' chain)
#pragma unroll
      for (int c = t + 2; c < t + 4; ++c) a[c] = a[c] - li0 * bcast(li0, j0 + c) - li1 * bcast(li1, j0 + c);
#pragma unroll
      for (int c = t + 4; c < 8; ++c) a[c] = a[c] - li0 * bcast(li0, j0 + c) - li1 * bcast(li1, j0 + c);
    } else {
#pragma unroll
      for (int c = t + 2; c < 8; ++c) a[c] = a[c] - li0 * bcast(li0, j0 + c) - li1 * bcast(li1, j0 + c);
    }
  }
}

// The panel chain's factor (chain_factor, cholesky.hip): the look-ahead walk
// with wave_factor8_pair2 panels.  Templated on the pointer type as
// lds_potrf64_lookahead is; the chain calls it out of line with
// address_space(3) pointers.
template <typename P>
__device__ inline void lds_potrf64_chain(P D, int* status) {
  const int i = threadIdx.x & 63;
  const int g = threadIdx.x >> 6;
  bool bad = false;
  auto panel = [&](int j0) {
    double a[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = (i >= j0) ? D[i * SMG_NBP + j0 + t] : 0.0;
    wave_factor8_pair2(a, j0, bad);
    wave_store8(D, a, j0);
  };
  if (g == 0) panel(0);
  __syncthreads();
  for (int p = 0; p < 7; ++p) {
    const int j0 = 8 * p, c1 = j0 + 8, c2 = j0 + 16;
    // (A) waves 1..7: panel p+1 (rows >= c1, 8 columns) -= panel p's rank-8
    //     update, one element per thread
    if (g > 0) {
      const int e = threadIdx.x - 64;
      const int r = c1 + (e >> 3), c = c1 + (e & 7);
      if (r < 64 && r >= c) {
        double v = D[r * SMG_NBP + c];
#pragma unroll
        for (int t = 0; t < 8; ++t) v -= D[r * SMG_NBP + j0 + t] * D[c * SMG_NBP + j0 + t];
        D[r * SMG_NBP + c] = v;
      }
    }
    __syncthreads();
    // (B) wave 0 factors panel p+1 while waves 1..7 update columns >= c2
    if (g == 0) {
      panel(c1);
    } else if (c2 < 64) {
      const int t0 = c2 >> 4, nt = 4 - t0, ntiles = nt * (nt + 1) / 2;
      const int fr = i & 15, fk = i >> 4;
      for (int q = g - 1; q < ntiles; q += 7) {
        int ti = 0, rem = q;
        while (rem > ti) {
          rem -= ti + 1;
          ++ti;
        }
        const int tj = rem + t0;
        ti += t0;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k0 = 0; k0 < 8; k0 += 4) {
          const double av = D[(16 * ti + fr) * SMG_NBP + j0 + k0 + fk];
          const double bv = D[(16 * tj + fr) * SMG_NBP + j0 + k0 + fk];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
        const int col = 16 * tj + fr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * ti + fk + 4 * r;
          if (col >= c2 && row >= col) D[row * SMG_NBP + col] -= acc[r];
        }
      }
    }
    __syncthreads();
  }
  if (bad) atomicOr(status, (int)SMG_ERR_NOT_PD);
}

// ---------------------------------------------------------------------------
// Pieces of X = L^{-1} (64x64) on 16x16 blocks, shared by lds_trtri64_mfma
// and the panel chain, which runs the leaves and the block rows as separate
// phases (chain_leaves_pub, chain_last_inverse in cholesky.hip: same
// arithmetic, same order: same bits).
// Leaf k (one wave, lane c < 16 owns column c): X_kk = L_kk^{-1} by
// right-looking elimination -- each x[q] still accumulates its terms in
// ascending order, but only one FMA per row sits on the dependency chain.
template <typename CP, typename P>
__device__ __forceinline__ void trtri_leaf16(CP D, P X, int k) {
  const int l = threadIdx.x & 63;
  const int r0 = 16 * k;
  double x[16], rv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    x[r] = (l == r) ? 1.0 : 0.0;
    const double dd = D[(r0 + r) * SMG_NBP + r0 + r];
    double rr = __builtin_amdgcn_rcp(dd);
    rr = rr * (2.0 - dd * rr);
    rv[r] = rr * (2.0 - dd * rr);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    x[r] = x[r] * rv[r];
#pragma unroll
    for (int q = r + 1; q < 16; ++q) x[q] -= D[(r0 + q) * SMG_NBP + r0 + r] * x[r];
  }
  if (l < 16)
#pragma unroll
    for (int r = 0; r < 16; ++r) X[(r0 + r) * SMG_NBP + r0 + l] = x[r];
}
// T_q = -L[p, q:p] X[q:p, q] accumulated over k in [kb, ke) (multiples of 8,
// from 16q): two MFMA chains (even / odd k-steps of 4), summed at the store
template <typename CP, typename XP>
__device__ __forceinline__ void trtri_t_acc(CP D, XP X, int p, int q, int kb, int ke, d4& acc,
                                            d4& acc2) {
  const int l = threadIdx.x & 63;
  const int fr = l & 15, fk = l >> 4;
  for (int k0 = kb; k0 < ke; k0 += 8) {
    const double a = D[(16 * p + fr) * SMG_NBP + k0 + fk];
    const double b = X[(k0 + fk) * SMG_NBP + 16 * q + fr];
    const double a2 = D[(16 * p + fr) * SMG_NBP + k0 + 4 + fk];
    const double b2 = X[(k0 + 4 + fk) * SMG_NBP + 16 * q + fr];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, acc2, 0, 0, 0);
  }
}
template <typename P>
__device__ __forceinline__ void trtri_t_store(P T, int q, const d4& acc, const d4& acc2) {
  const int l = threadIdx.x & 63;
  const int fr = l & 15, fk = l >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) T[q * 256 + (fk + 4 * r) * 16 + fr] = -(acc[r] + acc2[r]);
}
// X[p, q] = X_pp T_q
template <typename P>
__device__ __forceinline__ void trtri_x_tile(P X, P T, int p, int q) {
  const int l = threadIdx.x & 63;
  const int fr = l & 15, fk = l >> 4;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k0 = 0; k0 < 16; k0 += 4) {
    const double a = X[(16 * p + fr) * SMG_NBP + 16 * p + k0 + fk];
    const double b = T[q * 256 + (k0 + fk) * 16 + fr];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) X[(16 * p + fk + 4 * r) * SMG_NBP + 16 * q + fr] = acc[r];
}

// X = L^{-1} (64x64) with 16x16 blocks on the fp64 matrix cores:
//   leaves: wave w < 4 inverts diagonal block w (trtri_leaf16)
//   block rows p = 1..3:  T = -L[p, 0:p] X[0:p, 0:p]  (wave q < p: tile (p, q)),
//                         X[p, 0:p] = X_pp T          (wave q < p)
// X: LDS [64][SMG_NBP], fully written (upper zeros); T: LDS >= 3 * 256 doubles.
template <typename CP, typename P>
__device__ inline void lds_trtri64_mfma(CP D, P X, P T) {
  const int w = threadIdx.x >> 6;
  for (int e = threadIdx.x; e < 64 * SMG_NBP; e += blockDim.x) X[e] = 0.0;
  __syncthreads();
  if (w < 4) trtri_leaf16(D, X, w);
  __syncthreads();
  for (int p = 1; p < 4; ++p) {
    if (w < p) {
      d4 acc = d4{0.0, 0.0, 0.0, 0.0}, acc2 = acc;
      trtri_t_acc(D, X, p, w, 16 * w, 16 * p, acc, acc2);
      trtri_t_store(T, w, acc, acc2);
    }
    __syncthreads();
    if (w < p) trtri_x_tile(X, T, p, w);
    __syncthreads();
  }
}

// A wave's 16 x 16 leaf inverse k (the diagonal block of X written by
// trtri_leaf16) stored (sc1) into G (ld ldg; rows / columns < b): 4 values
// per lane, rows fastest (128-byte column runs), read back from LDS after the
// wave's own writes
template <typename P>
__device__ __forceinline__ void leaf16_store(const P X, double* G, int ldg, int b, int k) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = l + 64 * q, r = 16 * k + (e & 15), c = 16 * k + (e >> 4);
    if (r < b && c < b)
      __hip_atomic_store(&G[r + (size_t)c * ldg], (double)X[r * SMG_NBP + c], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------
// Y <- Y L^{-T} in place (Y: 64 x 64, L: 64 x 64 lower, both LDS [r][c]
// stride SMG_NBP), given the 16 x 16 leaf inverses Li_pp = L_pp^{-1} on the
// diagonal blocks of Li (trtri_leaf16).  Wave w < 4 solves row tile w alone,
// column blocks p = 0..3 in order:
//   Z = Y[w, p] - sum_{q < p} X[w, q] L[p, q]^T,   X[w, p] = Z Li_pp^T
// (40 MFMAs on one dependency chain per wave; no barrier inside: a wave's
// LDS accesses complete in order).  Waves >= row_tiles return at once (Y's
// first 16 row_tiles rows are solved).
template <typename P, typename CP>
__device__ inline void lds_trsm64_rt(P Y, CP L, CP Li, int row_tiles = 4) {
  const int w = threadIdx.x >> 6;
  if (w >= row_tiles) return;
  const int l = threadIdx.x & 63, fr = l & 15, fk = l >> 4;
  const int r0 = 16 * w;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < p; ++q)
#pragma unroll
      for (int k0 = 0; k0 < 16; k0 += 4) {
        const double a = Y[(r0 + fr) * SMG_NBP + 16 * q + k0 + fk];  // X[w, q](fr, k)
        const double b = L[(16 * p + fr) * SMG_NBP + 16 * q + k0 + fk];  // L[p, q]^T(k, fr)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      auto y = &Y[(r0 + fk + 4 * r) * SMG_NBP + 16 * p + fr];
      *y = *y - acc[r];
    }
    d4 x = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k0 = 0; k0 < 16; k0 += 4) {
      const double a = Y[(r0 + fr) * SMG_NBP + 16 * p + k0 + fk];        // Z(fr, k)
      const double b = Li[(16 * p + fr) * SMG_NBP + 16 * p + k0 + fk];   // Li_pp^T(k, fr)
      x = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, x, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Y[(r0 + fk + 4 * r) * SMG_NBP + 16 * p + fr] = x[r];
  }
}

// ---------------------------------------------------------------------------
// The fused diagonal-block kernels' body (SMG_DIAG_THREADS threads): factor D
// in place (if asked; otherwise D already holds L), X = L^{-1}, then one
// coalesced write of L (lower, upper zeroed) and X (dense, upper zeros).
// D, X: LDS [64][SMG_NBP], D identity padded beyond b.  Lout / Xout:
// col-major global destinations (b x b; either may be null).
__device__ __forceinline__ void lds_potrf_inv64_blk(double* D, double* X, int b, double* Lout, int ldl,
                                           double* Xout, int ldx, int* status, bool factor) {
  __shared__ double T[3 * 256];
  if (factor) lds_potrf64_lookahead(D, status);
  lds_trtri64_mfma(D, X, T);
  for (int e = threadIdx.x; e < b * b; e += blockDim.x) {
    const int c = e / b, r = e % b;
    if (Lout) Lout[r + (size_t)c * ldl] = (r >= c) ? D[r * SMG_NBP + c] : 0.0;
    if (Xout) Xout[r + (size_t)c * ldx] = (r >= c) ? X[r * SMG_NBP + c] : 0.0;
  }
}

// load a b x b block (col-major, ld) into LDS [r][c]; lower_only zeroes the
// strict upper triangle; rows/cols >= b are identity padding
__device__ inline void lds_load_block(double* D, const double* A, int ld, int b, bool lower_only) {
  constexpr int PER = SMG_NB * SMG_NB / SMG_DIAG_THREADS;
  if (blockDim.x == SMG_DIAG_THREADS) {  // all global loads in flight at once
    double v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = threadIdx.x + q * SMG_DIAG_THREADS;
      const int c = e / SMG_NB, r = e % SMG_NB;
      v[q] = (r < b && c < b && (!lower_only || r >= c)) ? A[r + (size_t)c * ld] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = threadIdx.x + q * SMG_DIAG_THREADS;
      const int c = e / SMG_NB, r = e % SMG_NB;
      D[r * SMG_NBP + c] = (r < b && c < b) ? v[q] : (r == c ? 1.0 : 0.0);
    }
    return;
  }
  for (int e = threadIdx.x; e < SMG_NB * SMG_NB; e += blockDim.x) {
    const int c = e / SMG_NB, r = e % SMG_NB;
    double v;
    if (r < b && c < b)
      v = (!lower_only || r >= c) ? A[r + (size_t)c * ld] : 0.0;
    else
      v = (r == c) ? 1.0 : 0.0;
    D[r * SMG_NBP + c] = v;
  }
}

// zero-padded load (no identity): for adjoint blocks
__device__ inline void lds_load_block0(double* D, const double* A, int ld, int b, bool lower_only) {
  constexpr int PER = SMG_NB * SMG_NB / SMG_DIAG_THREADS;
  if (blockDim.x == SMG_DIAG_THREADS) {  // all global loads in flight at once
    double v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = threadIdx.x + q * SMG_DIAG_THREADS;
      const int c = e / SMG_NB, r = e % SMG_NB;
      v[q] = (r < b && c < b && (!lower_only || r >= c)) ? A[r + (size_t)c * ld] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = threadIdx.x + q * SMG_DIAG_THREADS;
      D[(e % SMG_NB) * SMG_NBP + e / SMG_NB] = v[q];
    }
    return;
  }
  for (int e = threadIdx.x; e < SMG_NB * SMG_NB; e += blockDim.x) {
    const int c = e / SMG_NB, r = e % SMG_NB;
    double v = 0.0;
    if (r < b && c < b && (!lower_only || r >= c)) v = A[r + (size_t)c * ld];
    D[r * SMG_NBP + c] = v;
  }
}
