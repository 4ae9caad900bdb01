// The GEMM's tile map (gemm.hip): which workgroup computes which tile of C
// over which K range, and the grid that launches them.  Pure integer functions
// shared by the host (launch sizes the grid with gemm_plan, cut_flops counts
// with gemm_k_range) and the kernel (k_gemm decodes its blockIdx.x with
// gemm_tile_of), so that one definition serves both and a host program can
// enumerate a whole grid (tests/cpp/gemm_tile_map_check.cpp).  No HIP include:
// it compiles with a plain C++ compiler too.
#ifndef SMG_GEMM_TILES_H
#define SMG_GEMM_TILES_H
#include <cmath>
#include "../../include/smg_hip.h"  // SMG_TRI_*

#ifdef __HIPCC__
#define SMG_HD __host__ __device__ __forceinline__
#else
#include <algorithm>
#define SMG_HD inline
#endif

namespace gemm_tiles {
#ifndef __HIPCC__
using std::max;
using std::min;
#endif

SMG_HD int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// One launch's geometry: the product's extents and K cuts as the kernel takes
// them, and the grid gemm_plan gives it.  MODE (k_gemm's): 0 / 4 = every tile
// of C, 1 / 3 = the lower, 2 = the upper triangle's tiles.
struct gemm_grid {
  int m, n, k;
  int tri;             // SMG_TRI_* bits: whole triangular operands (they also set the tile order)
  int cut_a, cut_b;    // offset triangles (-1: none), see gemm_k_range
  int cut_spread;      // spread the tiles the cuts shorten over the XCDs
  int tm, tn;          // tiles per side
  int ntiles;          // tiles per split: tm x tn, or the triangle's of a square triangle mode
  int px, ntp;         // XCD partition px x (8 / px) (0: linear order) and workgroups per split
  int splits, kchunk;  // split-K: grid.x = ntp * splits, split s takes K in [s kchunk, (s + 1) kchunk)
};

SMG_HD void tri_decode(int t, int& bi, int& bj) {
  // t -> (bi, bj) with bj <= bi, row-major over the lower triangle of tiles
  int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  while (r * (r + 1) / 2 > t) --r;
  bi = r;
  bj = t - r * (r + 1) / 2;
}

// t -> (bi, bj) over the lower triangle of T x T tiles in groups of 8 block
// rows, each group column by column (its rows i >= j within a column): the
// tiles in flight at once share a few A row panels and B column panels, where
// the row-major order swept every B panel of a row before the next row
SMG_HD void tri_decode_grouped(int t, int T, int& bi, int& bj) {
  constexpr int G = 8;
  int r, c;
  tri_decode(t, r, c);
  const int r0 = r / G * G, r1 = min(r0 + G, T), h = r1 - r0;
  int q = t - r0 * (r0 + 1) / 2;
  if (q < r0 * h) {
    bi = r0 + q % h;
    bj = q / h;
    return;
  }
  q -= r0 * h;
  int j = r0;
  while (q >= r1 - j) {
    q -= r1 - j;
    ++j;
  }
  bi = j + q;
  bj = j;
}

// The grid of one product on BM x BN tiles with K stages of BK (NB: k_gemm's,
// nonzero = the DMA-staged kernel).  cut_mode (smg_set_gemm_cut_mode): 0 the
// product ignores its offset cuts, 1 it takes them, 2 it takes them in the
// uncut product's tile placement.
template <int BM, int BN, int BK, int MODE, int NB>
SMG_HD gemm_grid gemm_plan(int m, int n, int k, int tri, int batch, int cut_mode, int cut_a, int cut_b) {
  constexpr bool TRIC = MODE == 1 || MODE == 2 || MODE == 3;
  gemm_grid g;
  g.m = m, g.n = n, g.k = k, g.tri = tri;
  g.cut_a = cut_mode ? cut_a : -1, g.cut_b = cut_mode ? cut_b : -1;
  g.cut_spread = cut_mode == 1;
  const int tm = ceil_div(m, BM), tn = ceil_div(n, BN);
  const int ntiles = (TRIC && m == n && BM == BN) ? tm * (tm + 1) / 2 : tm * tn;
  // split K when the tile grid cannot fill the 256 CUs and K is long
  int splits = 1;
  const int target = 512;
  constexpr int KMIN = 64;  // shortest K chunk of a split
  // (a grid that already covers every CU once keeps K whole while K is short:
  // 512^3 with 32 x 32 tiles, 256 tiles: 12.3 us unsplit vs 15.9 us split
  // in two plus the reduction)
  const bool covers = ntiles >= 256 && k <= 1024;
  // (triangular operands: every tile has its own K range, no split)
  // (MODE 3 / 4 products -- the symbolic step's, with triangular operands --
  // never split)
  // (the DMA-staged kernel never splits: its K ranges are whole stages)
  if (NB == 0 && !tri && MODE != 3 && MODE != 4 && batch == 1 && ntiles < target && !covers &&
      k >= 2 * KMIN) {
    splits = ceil_div(target, ntiles);
    const int maxs = k / KMIN;
    if (splits > maxs) splits = maxs;
    if (splits > 64) splits = 64;
    if (splits < 1) splits = 1;
  }
  int kchunk = ceil_div(ceil_div(k, splits), BK) * BK;
  splits = ceil_div(k, kchunk);
  // XCD partition px x (8 / px) of a full tile grid minimising the per-XCD
  // operand footprint (rows of A + columns of B, in tiles); triangle grids
  // (tri_decode order) and grids too small to split keep the linear order
  // (a triangular operand alone: the linear, longest-K-first order of the
  // kernel's tile decode instead)
  const bool tri_one = !TRIC && tri && (!(tri & 3) || !(tri & 12));
  int px = 0, ntp = ntiles;
  if (!(TRIC && m == n && BM == BN) && ntiles >= 64 && !tri_one) {
    long long best = -1;
    for (int p = 1; p <= 8; p *= 2) {
      const int q = 8 / p;
      if (p > tm || q > tn) continue;
      const long long rr = ceil_div(tm, p), cc = ceil_div(tn, q);
      const long long foot = rr * BM + cc * BN;
      if (best < 0 || foot < best) {
        best = foot;
        px = p;
        ntp = 8 * (int)(rr * cc);
      }
    }
  }
  g.tm = tm, g.tn = tn, g.ntiles = ntiles, g.px = px, g.ntp = ntp, g.splits = splits, g.kchunk = kchunk;
  return g;
}

// The tile (block row bi, block column bj) and K split of workgroup wg (blockIdx.x)
// of the grid; live == false: the workgroup has no tile and exits.
struct gemm_tile {
  int bi, bj, split;
  bool live;
};

template <int BM, int BN, int MODE>
SMG_HD gemm_tile gemm_tile_of(const gemm_grid& g, unsigned wg) {
  constexpr bool LOWT = MODE == 1 || MODE == 3;  // lower-triangle tiles
  constexpr bool UPT = MODE == 2;
  constexpr bool TRIC = LOWT || UPT;
  const int m = g.m, n = g.n, tri = g.tri, cut_a = g.cut_a, cut_b = g.cut_b, cut_spread = g.cut_spread;
  const int tiles_m = g.tm, ntiles = g.ntiles, px = g.px, ntp = g.ntp;
  int bi, bj, tile, split;
  // A triangular operand gives every tile a K range set by its row (op(A))
  // or column (op(B)) block.  The workgroups a CU holds at once are assigned
  // by index, so an order in which that block index varied fastest gave each
  // CU tiles of ONE block: the CUs of the long-K blocks carried ~2x the mean
  // work (N^3 products with a triangular op(A) took 0.88x the full product's
  // time instead of 0.5x).  Such grids run in the linear order (the plan
  // sets px = 0) with that block index varying slowest, longest K first
  // (N = 4096, op(A) upper: 2120 -> 1143 us; op(B) upper 1136 us).
  const bool tri_a_only = !TRIC && (tri & 3) && !(tri & 12);
  const bool tri_b_only = !TRIC && (tri & 12) && !(tri & 3);
  if (px > 0) {
    // XCD-aware placement (full / trapezoidal grids): workgroups b and b + 8
    // share an XCD (round-robin dispatch), so XCD slot x = b % 8 takes one
    // rectangle of a px x (8 / px) partition of the tile grid, column-major
    // inside it; each XCD's L2 then holds 1/px of A's rows and px/8 of B's
    // columns instead of all of both.  Grid: ntp = 8 x the largest rectangle
    // per split; surplus workgroups exit.
    split = wg / ntp;
    const int tb = wg - split * ntp;
    const int x = tb & 7, l = tb >> 3, py = 8 / px;
    const int tiles_n = ntiles / tiles_m;
    const int rx = x % px, ry = x / px;
    const int r0 = rx * tiles_m / px, r1 = (rx + 1) * tiles_m / px;
    const int c0 = ry * tiles_n / py, c1 = (ry + 1) * tiles_n / py;
    const int rm = r1 - r0;
    // cut_b: the tile columns from the cut on run ever shorter K ranges, and
    // they are the last ones: in contiguous column ranges the XCDs of the
    // last range(s) idle while the others set the kernel's time.  The columns
    // are dealt round-robin instead (XCD column slot ry takes ry, ry + py,
    // ...): as many column panels of B per XCD as before, the short ones last.
    const bool deal = cut_spread && cut_b >= 0;
    const int nc = deal ? (tiles_n - ry + py - 1) / py : c1 - c0;
    if (rm <= 0 || l >= rm * nc) return {0, 0, split, false};
    tile = (r0 + l % rm) + (deal ? ry + py * (l / rm) : c0 + l / rm) * tiles_m;
  } else {
    tile = wg % ntiles;
    split = wg / ntiles;
  }
  // triangle modes: square C -> only the tiles of the triangle are launched
  // (tri_decode); trapezoidal C (m != n, the panel updates of the two-level
  // Cholesky) -> the full grid, tiles wholly outside the triangle exit
  const bool tri_sq = TRIC && m == n && BM == BN;
  if (LOWT && tri_sq) {
    // lower-triangle grids in the order of decreasing K range under the
    // triangular operands (see tri_a_only above): by column (op(B) lower:
    // K in [j0, k)), by column from the right (op(B) upper: K below j0 + BN),
    // by diagonal from the corner (both lower: K in [j0, i0 + BM)), by row
    // from the bottom (op(A) lower alone), else by row from the top
    const int T = tiles_m;
    int r, q;
    if (tri == SMG_TRI_B_LOWER) {
      tri_decode(ntiles - 1 - tile, r, q);
      bj = T - 1 - r;
      bi = bj + q;
    } else if (tri == SMG_TRI_B_UPPER || tri == (SMG_TRI_A_LOWER | SMG_TRI_B_UPPER)) {
      tri_decode(tile, r, q);
      bj = T - 1 - r;
      bi = bj + q;
    } else if (tri == (SMG_TRI_A_LOWER | SMG_TRI_B_LOWER)) {
      tri_decode(tile, r, q);
      bj = q;
      bi = q + (T - 1 - r);
    } else if (tri == SMG_TRI_A_LOWER) {
      tri_decode(ntiles - 1 - tile, bi, bj);
    } else if (tri == 0 && ntiles >= 64) {
      // equal-work tiles (no K cut): XCD x (workgroups b = x mod 8, dispatched
      // round-robin) takes one contiguous run of the grouped tile order, so
      // its L2 holds a few row panels of A and column panels of B at a time
      // (row-major over all XCDs, the last K^{-1} share fetched 530 MB
      // against 151 MB algorithmic, r06 PMC)
      // (cut_a: the tile rows from the cut on run ever shorter K ranges and
      // come last in that order, all in the last XCDs' runs, which then idle
      // while the others set the kernel's time.  The order is split at the
      // first row group that reaches the cut -- nu tiles before it, a multiple
      // of 8 -- and every XCD takes a run of each part, the short tiles last.)
      const int b = tile, x = b & 7, l = b >> 3;
      int nu = 0;
      if (cut_spread && cut_a >= 0) {
        const int g0 = min((cut_a + BM - 1) / BM, T) / 8 * 8;
        nu = (g0 * (g0 + 1) / 2) & ~7;
      }
      const int rest = ntiles - nu, per = rest >> 3, extra = rest & 7;
      const int t = l < (nu >> 3) ? x * (nu >> 3) + l : nu + x * per + (x < extra ? x : extra) + l - (nu >> 3);
      tri_decode_grouped(t, tiles_m, bi, bj);
    } else {
      tri_decode(tile, bi, bj);
    }
  } else if (UPT && tri_sq) {
    tri_decode(tile, bj, bi);
  } else if (tri_a_only) {  // rows slowest, longest K first
    const int r = tile / (ntiles / tiles_m);
    bi = (tri & 1) ? tiles_m - 1 - r : r;
    bj = tile % (ntiles / tiles_m);
  } else if (tri_b_only) {  // columns slowest, longest K first
    const int tn = ntiles / tiles_m, c = tile / tiles_m;
    bi = tile % tiles_m;
    bj = (tri & 8) ? tn - 1 - c : c;
  } else {
    bi = tile % tiles_m;
    bj = tile / tiles_m;
  }
  if (LOWT && !tri_sq && bj * BN > bi * BM + BM - 1) return {bi, bj, split, false};
  if (UPT && !tri_sq && bi * BM > bj * BN + BN - 1) return {bi, bj, split, false};
  return {bi, bj, split, true};
}

// The K range [kbeg, kend) of split `split` of the tile at (i0, j0): its
// chunk of K, cut to where the tile's operands can be nonzero.
struct gemm_krange {
  int kbeg, kend;
};

template <int BM, int BN, int BK>
SMG_HD gemm_krange gemm_k_range(const gemm_grid& g, int i0, int j0, int split) {
  const int k = g.k, tri = g.tri, cut_a = g.cut_a, cut_b = g.cut_b, kchunk = g.kchunk;
  int kbeg = split * kchunk;
  int kend = min(k, kbeg + kchunk);
  if (tri || cut_a >= 0 || cut_b >= 0) {
    // triangular operands: only k where both op(A)(i, k) and op(B)(k, j) can
    // be nonzero for some (i, j) of this tile (BK-aligned: the extra
    // elements are stored zeros)
    int lo = 0, hi = k;
    if (tri & 1) hi = min(hi, i0 + BM);  // op(A) lower: zero for k > i
    if (tri & 2) lo = max(lo, i0);       // op(A) upper: zero for k < i
    if (tri & 4) lo = max(lo, j0);       // op(B) lower: zero for k < j
    if (tri & 8) hi = min(hi, j0 + BN);  // op(B) upper: zero for k > j
    // offset triangles (no say in the tile order, unlike tri): op(A)(i, k) = 0
    // for k < i - cut_a in the rows i >= cut_a, op(B)(k, j) = 0 for
    // k < j - cut_b in the columns j >= cut_b (a block row [X | T] of a lower
    // triangular matrix, T its diagonal block: T's tile band starts at the cut)
    if (cut_a >= 0 && i0 >= cut_a) lo = max(lo, i0 - cut_a);
    if (cut_b >= 0 && j0 >= cut_b) lo = max(lo, j0 - cut_b);
    lo = lo / BK * BK;
    kbeg = max(kbeg, lo);
    kend = min(kend, hi);
    if (kend < kbeg) kend = kbeg;
  }
  return {kbeg, kend};
}

}  // namespace gemm_tiles
#endif
