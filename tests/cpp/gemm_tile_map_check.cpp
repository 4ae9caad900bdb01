// Host check of the GEMM's tile map (math_amd/csrc/gemm_tiles.h): for every
// configuration the whole launched grid is enumerated with the functions the
// kernel itself calls, and held against what a product needs:
//   1. every required tile (all of C; in the triangle modes the tiles that
//      intersect the triangle) is produced exactly once per split, and no
//      other tile is live;
//   2. over the splits, a tile's K ranges are disjoint and their union is
//      exactly [lo, hi), lo / hi restated here from the definitions of tri,
//      cut_a and cut_b (lo floored to the K stage);
//   3. that range holds every k at which op(A)(i, k) and op(B)(k, j) can both
//      be nonzero for an element (i, j) of the tile (element by element on
//      grids of up to four tiles, at the tiles' corner elements on larger ones);
//   4. the plan's tile counts and grid size are what the enumeration needs.
// Built and run by tests/test_gemm_tile_map.py; links nothing of the library.
#include "../../math_amd/csrc/gemm_tiles.h"

#include <algorithm>
#include <cstdio>
#include <vector>

using namespace gemm_tiles;

static long long n_configs = 0, n_workgroups = 0;
static int n_failed = 0;

struct config {
  int BM, BN, BK, MODE, NB, m, n, k, tri, cut_mode, cut_a, cut_b;
};

static bool fail(const config& c, const char* what, int x = 0, int y = 0, int z = 0) {
  if (++n_failed <= 20)
    std::printf("FAIL %s (%d, %d, %d): tile %dx%d BK %d MODE %d NB %d, m %d n %d k %d tri %d cut mode %d cut_a %d cut_b %d\n",
                what, x, y, z, c.BM, c.BN, c.BK, c.MODE, c.NB, c.m, c.n, c.k, c.tri, c.cut_mode, c.cut_a, c.cut_b);
  return false;
}

// the k at which op(A)(i, k) (side 0) or op(B)(k, j) (side 1) can be nonzero: [first, last]
static void nonzero_k(int side, int r, int k, int tri, int cut, int& first, int& last) {
  first = 0, last = k - 1;
  if (tri & (side ? 8 : 1)) last = std::min(last, r);    // op(A) lower: zero for k > i; op(B) upper: zero for k > j
  if (tri & (side ? 4 : 2)) first = std::max(first, r);  // op(A) upper: zero for k < i; op(B) lower: zero for k < j
  if (cut >= 0 && r >= cut) first = std::max(first, r - cut);
}

template <int BM, int BN, int BK, int MODE, int NB>
static bool check(int m, int n, int k, int tri, int cut_mode, int cut_a, int cut_b) {
  const config c = {BM, BN, BK, MODE, NB, m, n, k, tri, cut_mode, cut_a, cut_b};
  constexpr bool LOW = MODE == 1 || MODE == 3, UP = MODE == 2;
  ++n_configs;
  const gemm_grid g = gemm_plan<BM, BN, BK, MODE, NB>(m, n, k, tri, 1, cut_mode, cut_a, cut_b);
  const int ea = cut_mode ? cut_a : -1, eb = cut_mode ? cut_b : -1;  // the cuts in effect
  const int tm = (m + BM - 1) / BM, tn = (n + BN - 1) / BN;
  // which tiles the product needs
  std::vector<char> need((size_t)tm * tn);
  int n_need = 0;
  for (int bj = 0; bj < tn; ++bj)
    for (int bi = 0; bi < tm; ++bi) {
      const int ilast = std::min(bi * BM + BM, m) - 1, jlast = std::min(bj * BN + BN, n) - 1;
      const bool r = LOW ? ilast >= bj * BN : UP ? jlast >= bi * BM : true;
      need[bi + (size_t)bj * tm] = r;
      n_need += r;
    }
  // 4. the plan
  const bool tri_sq = (LOW || UP) && m == n && BM == BN;
  if (g.tm != tm || g.tn != tn) return fail(c, "plan: tiles per side", g.tm, g.tn);
  if (g.ntiles != (tri_sq ? tm * (tm + 1) / 2 : tm * tn)) return fail(c, "plan: ntiles", g.ntiles);
  if (tri_sq && g.ntiles != n_need) return fail(c, "plan: triangle tiles", g.ntiles, n_need);
  if (g.splits < 1 || g.splits > 64 || g.kchunk % BK || (long long)g.splits * g.kchunk < k ||
      (long long)(g.splits - 1) * g.kchunk >= k)
    return fail(c, "plan: split", g.splits, g.kchunk);
  if ((NB || tri || MODE >= 3) && g.splits != 1) return fail(c, "plan: split where none may be", g.splits);
  if (g.px == 0 ? g.ntp != g.ntiles
                : (g.px != 1 && g.px != 2 && g.px != 4 && g.px != 8) || g.px > tm || 8 / g.px > tn || g.ntp % 8 ||
                      g.ntp < g.ntiles)
    return fail(c, "plan: grid", g.px, g.ntp, g.ntiles);
  if (g.cut_a != ea || g.cut_b != eb || g.cut_spread != (cut_mode == 1)) return fail(c, "plan: cuts", g.cut_a, g.cut_b);
  // 1. the grid, workgroup by workgroup
  const int S = g.splits;
  std::vector<char> seen((size_t)S * tm * tn);
  std::vector<int> kb((size_t)S * tm * tn), ke((size_t)S * tm * tn);
  for (unsigned wg = 0; wg < (unsigned)(g.ntp * S); ++wg) {
    ++n_workgroups;
    const gemm_tile t = gemm_tile_of<BM, BN, MODE>(g, wg);
    if (!t.live) continue;
    if (t.bi < 0 || t.bi >= tm || t.bj < 0 || t.bj >= tn || t.split < 0 || t.split >= S)
      return fail(c, "tile outside the grid", t.bi, t.bj, t.split);
    const size_t at = t.bi + (size_t)t.bj * tm + (size_t)t.split * tm * tn;
    if (seen[at]++) return fail(c, "tile produced twice", t.bi, t.bj, t.split);
    const gemm_krange kr = gemm_k_range<BM, BN, BK>(g, t.bi * BM, t.bj * BN, t.split);
    kb[at] = kr.kbeg, ke[at] = kr.kend;
  }
  const bool small = tm * tn <= 4;
  for (int bj = 0; bj < tn; ++bj)
    for (int bi = 0; bi < tm; ++bi) {
      const size_t tile = bi + (size_t)bj * tm;
      for (int s = 0; s < S; ++s)
        if (seen[tile + (size_t)s * tm * tn] != need[tile])
          return fail(c, need[tile] ? "tile missing" : "tile live outside the triangle", bi, bj, s);
      if (!need[tile]) continue;
      // 2. lo and hi from the definitions
      const int i0 = bi * BM, j0 = bj * BN;
      int lo = 0, hi = k;
      if (tri & 1) hi = std::min(hi, i0 + BM);  // op(A) lower: the tile's last row is i0 + BM - 1
      if (tri & 2) lo = std::max(lo, i0);       // op(A) upper: its first row is i0
      if (tri & 4) lo = std::max(lo, j0);       // op(B) lower: its first column is j0
      if (tri & 8) hi = std::min(hi, j0 + BN);  // op(B) upper
      if (ea >= 0 && i0 >= ea) lo = std::max(lo, i0 - ea);
      if (eb >= 0 && j0 >= eb) lo = std::max(lo, j0 - eb);
      lo -= lo % BK;
      int at = lo, first = -1;
      for (int s = 0; s < S; ++s) {
        const int b = kb[tile + (size_t)s * tm * tn], e = ke[tile + (size_t)s * tm * tn];
        if (e < b || (e > b && (b < 0 || e > k))) return fail(c, "K range out of order or outside [0, k)", bi, bj, s);
        if (NB && (e - b) % BK) return fail(c, "DMA staging: K range not in whole stages", bi, bj, s);
        if (e == b) continue;
        if (first < 0) first = b;
        if (b != at) return fail(c, "K ranges of the splits overlap or leave a gap", bi, bj, s);
        at = e;
      }
      if (hi > lo ? (first != lo || at != hi) : first >= 0) return fail(c, "K range is not [lo, hi)", bi, bj, first);
      // 3. sufficiency, element by element
      const int i1 = std::min(i0 + BM, m), j1 = std::min(j0 + BN, n);
      const int istep = small ? 1 : std::max(1, i1 - 1 - i0), jstep = small ? 1 : std::max(1, j1 - 1 - j0);
      for (int j = j0; j < j1; j += jstep) {
        int af, al, bf, bl;
        nonzero_k(1, j, k, tri, eb, bf, bl);
        for (int i = i0; i < i1; i += istep) {
          if ((LOW && i < j) || (UP && i > j)) continue;  // (not an element of C)
          nonzero_k(0, i, k, tri, ea, af, al);
          const int f = std::max(af, bf), l = std::min(al, bl);
          if (f <= l && (first < 0 || f < first || l >= at)) return fail(c, "K range misses a nonzero term", i, j, f);
        }
      }
    }
  return true;
}

// cut positions for an extent of `ext` on tiles of `b`: none, 0, tile-aligned,
// unaligned, and up to the extent
static std::vector<int> cut_values(int ext, int b) {
  return {0, ext / 2 / b * b, ext / 3 + 1, ext - 1, ext};
}

// the sides that cross a threshold of the plan or the tile orders: 64 tiles
// (8 x 8; T = 11 for a triangle), the 8-row groups, 256 tiles (16 x 16; T = 22,
// 23) and 512 (T = 31, 32)
static const int SIDES[] = {1, 2, 3, 7, 8, 9, 10, 11, 16, 17, 22, 23, 24, 31, 32, 40};
static const int TRIS[] = {0, 1, 2, 4, 8, 5, 9};
static const int KS[] = {64, 128, 512, 1024, 1536, 4096};

template <int BM, int BN, int BK, int MODE, int NB>
static void sweep_shape(int m, int n, int wide) {  // wide 0: two products, 1: the tile orders, 2: everything
  auto run = [&](int k, int tri, int cut_mode, int cut_a, int cut_b) {
    if (NB && k % 32) return;
    check<BM, BN, BK, MODE, NB>(m, n, k, tri, cut_mode, cut_a, cut_b);
  };
  if (m <= 0 || n <= 0) return;
  // every shape: no cuts, and the columns dealt
  run(64, 0, 1, -1, -1);
  run(64, 0, 1, -1, n / 2 / BN * BN);
  if (wide == 1) {
    for (int tri : TRIS) run(128, tri, 1, -1, -1);
    for (int cut_mode = 1; cut_mode <= 2; ++cut_mode)
      for (int ca : cut_values(m, BM)) run(128, 0, cut_mode, ca, -1);
  }
  if (wide < 2) return;
  for (int tri : TRIS)
    for (int k : KS) {
      const bool two = k == 128 || k == 1536;  // (the cuts at a short and at a split K)
      if (tri) {  // (no split with a triangular operand)
        if (!two) continue;
        run(k, tri, 1, -1, -1);
        run(k, tri, 1, m / 3 + 1, -1);
        run(k, tri, 1, -1, n / 2 / BN * BN);
        continue;
      }
      run(k, 0, 1, -1, -1);
      run(k, 0, 1, m / 2 / BM * BM, n / 3 + 1);
      if (!two) continue;
      for (int cut_mode = 1; cut_mode <= 2; ++cut_mode) {
        for (int ca : cut_values(m, BM)) run(k, 0, cut_mode, ca, -1);
        for (int cb : cut_values(n, BN)) run(k, 0, cut_mode, -1, cb);
      }
      run(k, 0, 0, m / 2 / BM * BM, n / 3 + 1);  // (cut mode 0: ignored)
    }
}

template <int BM, int BN, int BK, int MODE, int NB = 0>
static void sweep() {
  constexpr bool TRIC = MODE >= 1 && MODE <= 3;
  auto wide = [](int t) { return t == 66 ? 1 : std::find(std::begin(SIDES), std::end(SIDES), t) != std::end(SIDES) ? 2 : 0; };
  // (NB: whole tiles; else odd sides end in a partial tile)
  auto ext = [](int t, int b) { return t * b - (NB == 0 && (t & 1) ? 5 : 0); };
  for (int tm = 1; tm <= (TRIC ? 66 : 40); ++tm) {
    if (tm > 40 && tm != 66) continue;
    const int m = ext(tm, BM);
    if (TRIC) {
      sweep_shape<BM, BN, BK, MODE, NB>(m, m, wide(tm));
      if (MODE == 3 || tm == 66) continue;
      // trapezoids: tall, wide, and one with the square's tile counts
      sweep_shape<BM, BN, BK, MODE, NB>(m, ext(std::max(1, tm - 3), BN), wide(tm));
      sweep_shape<BM, BN, BK, MODE, NB>(m, ext(tm + 2, BN), wide(tm));
      sweep_shape<BM, BN, BK, MODE, NB>(tm * BM, tm * BN - (NB ? 64 : 1), wide(tm));
    } else {
      for (int tn = 1; tn <= 40; ++tn)
        sweep_shape<BM, BN, BK, MODE, NB>(m, ext(tn, BN), tn == 1 || tn == 8 || tn == tm || tn == 41 - tm ? wide(tm) : 0);
    }
  }
}

template <int BM, int BN, int BK>
static void sweep_modes() {
  sweep<BM, BN, BK, 0>();
  sweep<BM, BN, BK, 1>();
  sweep<BM, BN, BK, 2>();
  sweep<BM, BN, BK, 3>();
  sweep<BM, BN, BK, 4>();
}

int main() {
  sweep_modes<32, 32, 32>();
  sweep_modes<64, 64, 16>();
  sweep_modes<128, 128, 16>();
  sweep<128, 64, 16, 0>();
  sweep<32, 64, 32, 0>();  // the in-place forms
  sweep<64, 32, 32, 0>();
  sweep<64, 64, 32, 0, 2>();  // the DMA-staged forms
  sweep<64, 64, 32, 1, 2>();
  sweep<64, 64, 16, 0, 3>();
  sweep<64, 64, 16, 1, 3>();
  std::printf("%lld configurations, %lld workgroups, %d failed\n", n_configs, n_workgroups, n_failed);
  return n_failed != 0;
}
