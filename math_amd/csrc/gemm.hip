// fp64 GEMM on the CDNA4 matrix cores (v_mfma_f64_16x16x4_f64).
//
// C = alpha op(A) op(B) + beta C, optionally only the lower triangle of C.
// Used for the dense contractions of multiply (rev/mat/fun/multiply.hpp:65-135)
// and of the blocked Cholesky forward / Murray adjoint
// (rev/mat/fun/cholesky_decompose.hpp:135-158).
//
// Tiling: a 256-thread workgroup (4 waves, 2x2) owns a BM x BN tile of C;
// each wave owns (BM/2) x (BN/2) = TM x TN MFMA tiles of 16x16 held in
// accumulators.  K advances in stages of BK (16 for the 128 x 128 and
// 64 x 64 tiles, 32 for the 32-wide ones) staged through LDS in unpadded,
// XOR-swizzled images (lds_layout): conflict-free ds_read_b64 fragment reads
// (16 consecutive rows/cols x 4 k) and staging stores.
// Global->LDS staging goes through registers (one stage of prefetch for the
// 128 x 128 tile, two for the small tiles) into double-buffered LDS; the
// beta * C operand of the epilogue is fetched before the K loop.
// The 64 x 64 tile has a second staging path for whole-tile, aligned products
// (dma_eligible): 16-byte LDS-DMA loads straight into the same swizzled
// images (the swizzle applied to the source address), no staging registers,
// K stages of 32 in two LDS buffers (8 waves) or of 16 in three (4 waves).
// Split-K writes fixed-order partial slabs reduced by a second kernel, so the
// result is bitwise deterministic run to run.
// Every tile's K range is cut to where its operands can be nonzero: whole
// triangular operands (tri, which also sets the tile order) and offset
// triangles in the last rows of op(A) / columns of op(B) (cut_a / cut_b, which
// leave the order alone and only spread the shortened tiles over the XCDs).
// Which workgroup computes which tile over which K range, and the grid that
// launches them, are host-and-device functions in gemm_tiles.h.
#include "smg_internal.h"
#include "gemm_tiles.h"
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#ifndef SMG_GEMM_TRI128_MIN
#define SMG_GEMM_TRI128_MIN 1024  // fewest 128 x 128 tiles a product with a triangular operand takes them at
#endif
#ifndef SMG_GEMM_KS2_MAX
#define SMG_GEMM_KS2_MAX 1536  // largest 64 x 64 tile count that takes the 8-wave variant
#endif
// The DMA-staged 64 x 64 kernel: K stage depth and LDS buffers of its 4-wave
// (1) and 8-wave (2) forms, the largest tile count that takes the 8-wave one,
// the fewest tiles the policy gives it, and the families it gives it
// (1: NT lower, 2: TN lower, 4: NN full, 8: TN full, 16: NN lower)
#ifndef SMG_GEMM_DMA_BK1
#define SMG_GEMM_DMA_BK1 16
#endif
#ifndef SMG_GEMM_DMA_NB1
#define SMG_GEMM_DMA_NB1 3
#endif
#ifndef SMG_GEMM_DMA_BK2
#define SMG_GEMM_DMA_BK2 32
#endif
#ifndef SMG_GEMM_DMA_NB2
#define SMG_GEMM_DMA_NB2 2
#endif
#ifndef SMG_GEMM_DMA_KS2_MAX
#define SMG_GEMM_DMA_KS2_MAX 512
#endif
#ifndef SMG_GEMM_DMA_MIN_TILES
#define SMG_GEMM_DMA_MIN_TILES 136
#endif
#ifndef SMG_GEMM_DMA_FAMILIES
#define SMG_GEMM_DMA_FAMILIES 31
#endif
#ifndef SMG_GEMM_NR64
#define SMG_GEMM_NR64 2
#endif
#ifndef SMG_GEMM_NR32
#define SMG_GEMM_NR32 2
#endif

namespace {
using namespace gemm_tiles;

// LDS images of the operand tiles, unpadded and XOR-swizzled so that both
// the staging stores (32 consecutive elements along the contiguous dim per
// half-wave) and the MFMA fragment reads (16 consecutive rows x 2 k per
// half-wave, ds_read_b64) hit 32 distinct bank pairs.
template <int BM, int BK, bool KCONTIG>
struct lds_layout;
template <int BM, int BK>
struct lds_layout<BM, BK, false> {  // [k][BM], row index ^ 16 on odd k
  static_assert(BM % 32 == 0, "BM");
  static constexpr int size = BK * BM;
  __device__ static int at(int i, int kk) { return kk * BM + (i ^ ((kk & 1) << 4)); }
  // the element stored at position p (the inverse of at; p even: p + 1 holds (i + 1, kk))
  __device__ static void from(int p, int& i, int& kk) {
    kk = p / BM;
    i = (p % BM) ^ ((kk & 1) << 4);
  }
};
template <int BM, int BK>
struct lds_layout<BM, BK, true> {  // [BM][BK], k index ^ f(row)
  static_assert(BK == 16 || BK == 32, "BK");
  static constexpr int size = BM * BK;
  __device__ static int at(int i, int kk) {
    return i * BK + (kk ^ (BK == 16 ? (i & 14) : ((i & 15) << 1)));
  }
  // (p even: p + 1 holds (i, kk + 1); both swizzles leave bit 0 alone)
  __device__ static void from(int p, int& i, int& kk) {
    i = p / BK;
    kk = (p % BK) ^ (BK == 16 ? (i & 14) : ((i & 15) << 1));
  }
};

// One 16-byte LDS-DMA load per lane: the wave's 64 lanes fill 1 KiB of LDS
// from `lds` (a wave-uniform byte address) on in lane order, each from its own
// global address g (16-byte aligned).  No register destination, and the
// compiler does not count it: the issuing wave waits with dma_wait_barrier.
// (M0 holds the LDS base only inside the statement.)
__device__ __forceinline__ void dma16(const double* g, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(g), "s"(lds)
      : "memory");
}

// Leave at most N of this wave's loads in flight, retire its fragment reads,
// then the workgroup barrier: behind it every wave's DMA issued before its
// last N loads has landed in LDS, and every wave is done reading the buffer
// that is staged next.  A raw barrier: __syncthreads() would drain to vmcnt(0).
template <int N>
__device__ __forceinline__ void dma_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// compile-time unrolled loop: f(std::integral_constant<int, 0>) .. f(<N - 1>)
template <int I, int N, typename F>
__device__ __forceinline__ void smg_static_for_impl(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    smg_static_for_impl<I + 1, N>(f);
  }
}
template <int N, typename F>
__device__ __forceinline__ void smg_static_for(F&& f) {
  smg_static_for_impl<0, N>(f);
}

// every out-of-range operand element is loaded from this zero instead of
// being masked after the load (see load_tile)
__device__ double g_gemm_zero[2] = {0.0, 0.0};  // global (not constant) address space: keeps the operand loads global_load, not flat_load

// Operand X viewed as a (rows x k) matrix in the kernel's orientation:
//   KCONTIG == false : element (i, kk) at X[i + kk*ld]
//   KCONTIG == true  : element (i, kk) at X[kk + i*ld]
// Branch- and select-free on the loaded data: an out-of-range element's
// ADDRESS is redirected to g_gemm_zero, so the loaded register goes straight
// to its LDS store.  (A select on the loaded value lets the scheduler hoist
// the select -- and with it a wait for that load -- ahead of the previous
// stage's MFMAs, which serialises the prefetch.)
template <int BM, int BK, bool KCONTIG, int NT = 256>
__device__ __forceinline__ void load_tile(const double* __restrict__ X, int ld,
                                          int rows, int k, int i0, int k0,
                                          double (&r)[BM * BK / NT]) {
  constexpr int PER = BM * BK / NT;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int e = threadIdx.x + NT * q;
    int i, kk;
    if (KCONTIG) {
      i = e / BK;
      kk = e % BK;
    } else {
      kk = e / BM;
      i = e % BM;
    }
    const int gi = i0 + i, gk = k0 + kk;
    const double* p = KCONTIG ? X + ((size_t)gi * ld + gk) : X + (gi + (size_t)gk * ld);
    r[q] = *((gi < rows && gk < k) ? p : g_gemm_zero);
  }
}

template <int BM, int BK, bool KCONTIG, int NT = 256>
__device__ __forceinline__ void store_tile(double* lds, const double (&r)[BM * BK / NT]) {
  constexpr int PER = BM * BK / NT;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int e = threadIdx.x + NT * q;
    int i, kk;
    if (KCONTIG) {
      i = e / BK;
      kk = e % BK;
    } else {
      kk = e / BM;
      i = e % BM;
    }
    lds[lds_layout<BM, BK, KCONTIG>::at(i, kk)] = r[q];
  }
}

// MODE: 0 = full C, 1 = lower / 2 = upper triangle of C only (BM == BN, m == n),
//   3 = the lower triangle computed and stored mirrored too (a symmetric C
//       from its lower half: no separate sym_from_lower pass),
//   4 = full C plus a second output C2 = tril(C) with halved diagonal (the
//       Murray reverse's D_adj image of its symbolic step: no separate pass).
// Split-K (slab != null): partial tiles into fixed-order slabs, summed by
// k_splitk_reduce (an in-kernel last-workgroup fixup measured slower: the
// tail reduction ran on one CU per tile, 90 -> 172 us for 512 x 2560 x 1536).
// KS: waves per output sub-tile (KS = 2: 8 waves, the two 4-wave groups take
// alternate halves of every K stage and their accumulators are summed in the
// epilogue -- twice the waves per CU for grids that cover the CUs only once
// or twice)
// NB: 0 = operands staged through registers; 2 or 3 = staged by LDS-DMA into
// NB LDS buffers (64 x 64 tile only).  That path has no bounds handling: the
// host takes it only for whole tiles, K ranges in whole stages and 16-byte
// aligned operand pairs (dma_eligible).
// The parameters stay scalars, and the pointers __restrict__ parameters.  As
// one by-value struct the kernel took the same registers but loaded its fields
// one by one where it first used them, a wait each time, and the short NN
// products on 32 x 32 tiles ran 1.2 to 1.5 % longer ((1024,512,512) 19.15 ->
// 19.44 us, 512^3 10.73 -> 10.85 us; profiles/gemm_args_ab.txt); and
// __restrict__ has no effect on a struct's member: without it the in-place
// forms' TN kernels took 222 VGPRs for 166.  The tile map's view of them, a
// gemm_grid (gemm_tiles.h), is put together from the scalars below.
template <int BM, int BN, int BK, bool TA, bool TB, int MODE, int KS = 1, int NB = 0>
__global__ __launch_bounds__(256 * KS) void k_gemm(
    int m, int n, int k, double alpha, const double* __restrict__ A, int lda,
    const double* __restrict__ B, int ldb, double beta, double* __restrict__ C,
    int ldc, int tiles_m, int ntiles, int kchunk, double* __restrict__ slab, long long sA,
    long long sB, long long sC, int px, int ntp, int tri, double* __restrict__ C2, int ldc2, int bz, int cut_a,
    int cut_b, int cut_spread) {
  const gemm_grid g = {m, n, k, tri, cut_a, cut_b, cut_spread, tiles_m, 0, ntiles, px, ntp, 0, kchunk};  // (tn, splits: the host's)
  constexpr bool LOWT = MODE == 1 || MODE == 3;  // lower-triangle tiles
  constexpr bool UPT = MODE == 2;
  // strided batch over blockIdx.y (sA = sB = sC = 0 for a single product)
  A += blockIdx.y * sA;
  B += blockIdx.y * sB;
  C += blockIdx.y * sC;
  // A-side contiguity: no-trans A is m-contiguous; trans A is k-contiguous.
  // B-side as an (n x k) operand: no-trans B is k-contiguous; trans B is n-contiguous.
  constexpr bool AK = TA;
  constexpr bool BKC = !TB;
  using LA = lds_layout<BM, BK, AK>;
  using LB = lds_layout<BN, BK, BKC>;
  // one LDS pool: the K-loop operand tiles, reused by the epilogue to stage
  // the C tile (column chunks of ECH columns, stride BM + 1) so that C is read
  // and written in whole column segments (coalesced 8*BM-byte runs)
  // operand tiles are double-buffered in LDS (one barrier per K stage)
  constexpr int NR = BM == 128 ? 1 : (BM == 64 ? SMG_GEMM_NR64 : SMG_GEMM_NR32);
  constexpr int STAGE = LA::size + LB::size;
  constexpr int OPS = (NB ? NB : 2) * STAGE;
  constexpr int ECH = (BM * BN + BN <= OPS) ? BN : 32;
  constexpr int POOL = (OPS > (BM + 1) * ECH) ? OPS : (BM + 1) * ECH;
  __shared__ double pool[POOL];

  // which tile of C this workgroup computes, over which K range (gemm_tiles.h)
  const gemm_tile t = gemm_tile_of<BM, BN, MODE>(g, blockIdx.x);
  if (!t.live) return;
  const int split = t.split, i0 = t.bi * BM, j0 = t.bj * BN;
  const gemm_krange kr = gemm_k_range<BM, BN, BK>(g, i0, j0, split);
  const int kbeg = kr.kbeg, kend = kr.kend;

  constexpr int TM = BM / 32, TN = BN / 32;
  constexpr int NT = 256 * KS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // (kg a compile-time 0 for KS == 1: the fragment reads' LDS offsets fold
  // into immediates; a run-time kg cost the 128 x 128 tile 15 %)
  const int wr = (wave & 3) >> 1, wc = wave & 1, kg = KS == 1 ? 0 : wave >> 2;
  d4 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};

  // operand tiles in registers between global memory and LDS: NR sets, so
  // that the load of stage s + NR is in flight while stages s .. s + NR - 1
  // are consumed (NR = 2 for the small tiles, whose grids leave only two or
  // three waves per SIMD to hide the load latency behind)
  constexpr int PA = BM * BK / NT, PB = BN * BK / NT;
  double ra[NR][PA], rb[NR][PB];
  const int nst = (kend - kbeg + BK - 1) / BK;  // K stages of this split
  auto gload = [&](int set, int st) {
    load_tile<BM, BK, AK, NT>(A, lda, m, kend, i0, kbeg + st * BK, ra[set]);
    load_tile<BN, BK, BKC, NT>(B, ldb, n, kend, j0, kbeg + st * BK, rb[set]);
  };
  auto lstore = [&](int set, int buf) {
    store_tile<BM, BK, AK, NT>(pool + buf * STAGE, ra[set]);
    store_tile<BN, BK, BKC, NT>(pool + buf * STAGE + LA::size, rb[set]);
  };
  // every stage load is unconditional (addresses are clamped in range and
  // stages past the end are masked to zero): a conditional load would make
  // the waitcnt pass assume the worst on the loop back-edge and wait for ALL
  // outstanding loads at each LDS store, i.e. no prefetch at all
  if constexpr (NB == 0) {
#pragma unroll
    for (int j = 0; j < NR; ++j) gload(j, j);
  }
  // epilogue operand in flight during the K loop (small tiles only: the
  // 128 x 128 tile would double its register count); coalesced mapping
  // e = tid + 256 q -> (i = e % BM, j = e / BM), the same as the store
  constexpr int EPT = BM * BN / NT;
  constexpr bool PREFETCH_C = EPT <= 16;
  // bz: tiles from row bz (bz > 0) or column -bz (bz < 0) on take beta = 0
  // (the first contribution to a region of an accumulated product: C is not read)
  const bool use_c = !slab && beta != 0.0 && !(bz > 0 && i0 >= bz) && !(bz < 0 && j0 >= -bz);
  double cpre[PREFETCH_C ? EPT : 1];
  if (PREFETCH_C) {
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int e = threadIdx.x + NT * q;
      const int i = i0 + e % BM, j = j0 + e / BM;
      cpre[q] = (use_c && i < m && j < n) ? C[i + (size_t)j * ldc] : 0.0;
    }
  }
  const int fr = lane & 15, fk = lane >> 4;
  static_assert(BK / 4 % KS == 0, "K stage split");
  auto mma_stage = [&](const double* Ab, const double* Bb) {
#pragma unroll
    for (int kq = 0; kq < BK / 4 / KS; ++kq) {
      const int ks = kg * (BK / 4 / KS) + kq;
      double af[TM], bf[TN];
#pragma unroll
      for (int a = 0; a < TM; ++a)
        af[a] = Ab[LA::at(wr * (BM / 2) + a * 16 + fr, ks * 4 + fk)];
#pragma unroll
      for (int b = 0; b < TN; ++b)
        bf[b] = Bb[LB::at(wc * (BN / 2) + b * 16 + fr, ks * 4 + fk)];
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
    }
  };
  if constexpr (NB == 0) {
  // stage s computes from LDS buffer s & 1 while stage s + 1 is stored into
  // the other buffer and stage s + 1 + NR is issued into the freed registers
  // (one barrier per stage); the loop is unrolled by two so that every
  // register-set index is a compile-time constant
  // (an odd stage count runs one all-zero stage: the loop body has no
  // conditional memory operations)
  lstore(0, 0);
  gload(0, NR);
  __syncthreads();
  // stage st: MMA from LDS buffer st & 1, store stage st + 1 (register set
  // (st + 1) % NR) into the other buffer, refill that set with stage
  // st + 1 + NR.  Unrolled by U = lcm(2, NR) so every set / buffer index is a
  // compile-time constant; the main loop has no conditional memory operation
  // (the tail's guards only cost precision of its own waits).
  constexpr int U = NR % 2 == 0 ? NR : 2 * NR;
  auto body = [&](int st, auto uc) {
    constexpr int u = decltype(uc)::value;
    mma_stage(pool + (u & 1) * STAGE, pool + (u & 1) * STAGE + LA::size);
    lstore((u + 1) % NR, (u & 1) ^ 1);
    gload((u + 1) % NR, st + 1 + NR);
    __syncthreads();
  };
  int s0 = 0;
  for (; s0 + U <= nst; s0 += U)
    smg_static_for<U>([&](auto uc) { body(s0 + decltype(uc)::value, uc); });
  smg_static_for<U - 1>([&](auto uc) {
    if (s0 + decltype(uc)::value < nst) body(s0 + decltype(uc)::value, uc);
  });
  } else {
    // LDS-DMA staging.  The LDS image of a tile is filled linearly, 1 KiB per
    // wave instruction (dma16); lane l of wave w writes doubles p, p + 1 with
    // p = 128 (q NW + w) + 2 l in its q-th instruction, and fetches the
    // element pair that lds_layout stores there (the swizzle is applied to
    // the source address).  Instruction q + 1 is NW 1-KiB pieces further on:
    // 2 NW k-rows (m-contiguous image: the same k parity, so the same
    // swizzle) or 128 NW / BK tile rows (k-contiguous image: a multiple of
    // 16, so the same swizzle) -- a wave-uniform pointer step.
    constexpr int NW = 4 * KS;         // waves
    constexpr int QA = BK / 2 / NW;    // DMA instructions per wave, operand tile and stage
    constexpr int L = 2 * QA;          // ... per stage
    static_assert(BM == 64 && BN == 64 && BK / 2 % NW == 0 && (NB == 2 || NB == 3), "DMA staging: 64 x 64 tile");
    static_assert(AK ? (128 * NW / BK) % 16 == 0 : true, "DMA staging: swizzle period");
    static_assert(NB * STAGE * 8 <= 65536, "DMA staging: LDS");
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const double *pa, *pb;
    {
      int i, kk;
      LA::from(wv * 128 + 2 * lane, i, kk);
      pa = AK ? A + ((size_t)(i0 + i) * lda + kbeg + kk) : A + ((i0 + i) + (size_t)(kbeg + kk) * lda);
      LB::from(wv * 128 + 2 * lane, i, kk);
      pb = BKC ? B + ((size_t)(j0 + i) * ldb + kbeg + kk) : B + ((j0 + i) + (size_t)(kbeg + kk) * ldb);
    }
    const long long qsa = (long long)(AK ? 128 * NW / BK : 2 * NW) * lda;
    const long long qsb = (long long)(BKC ? 128 * NW / BK : 2 * NW) * ldb;
    const long long ssa = AK ? BK : (long long)BK * lda, ssb = BKC ? BK : (long long)BK * ldb;
    const unsigned ldsw = (unsigned)(size_t)pool + wv * 1024;
    auto issue = [&](auto bc) {  // the next stage into buffer bc
      constexpr int buf = decltype(bc)::value;
#pragma unroll
      for (int q = 0; q < QA; ++q) dma16(pa + q * qsa, ldsw + (buf * STAGE) * 8 + q * NW * 1024);
#pragma unroll
      for (int q = 0; q < QA; ++q) dma16(pb + q * qsb, ldsw + (buf * STAGE + LA::size) * 8 + q * NW * 1024);
      pa += ssa;
      pb += ssb;
    };
    // Stage st is computed from buffer st % NB.  Before it: wait for this
    // wave's loads of stage st (with three buffers stage st + 1 stays in
    // flight across the barrier), barrier, then stage st + NB - 1 into the
    // buffer stage st - 1 was read from -- every wave finished those reads
    // before the barrier.  The fragment reads of stage st come after the
    // barrier that follows the wait for its loads.
    auto step = [&](int st, auto uc, auto full) {
      constexpr int u = decltype(uc)::value;
      constexpr bool FULL = decltype(full)::value;  // stages st + 1 .. st + NB - 1 exist
      if (NB == 3 && (FULL || st + 1 < nst)) dma_wait_barrier<L>();
      else dma_wait_barrier<0>();
      if (FULL || st + NB - 1 < nst) issue(std::integral_constant<int, (u + NB - 1) % NB>{});
      mma_stage(pool + u * STAGE, pool + u * STAGE + LA::size);
    };
    if (nst > 0) {
      issue(std::integral_constant<int, 0>{});
      if (NB == 3 && nst > 1) issue(std::integral_constant<int, 1>{});
      int s0 = 0;
      for (; s0 + 2 * NB - 1 <= nst; s0 += NB)
        smg_static_for<NB>([&](auto uc) { step(s0 + decltype(uc)::value, uc, std::true_type{}); });
      for (; s0 < nst; s0 += NB)
        smg_static_for<NB>([&](auto uc) {
          if (s0 + decltype(uc)::value < nst) step(s0 + decltype(uc)::value, uc, std::false_type{});
        });
    }
  }

  // epilogue: D layout of v_mfma_f64_16x16x4_f64: reg r of lane l holds
  // row (l>>4) + 4r, col l&15 of the 16x16 tile.  Accumulators go to LDS
  // (column-major, stride BM + 1), then every thread stores whole column runs.
  __syncthreads();  // operand tiles no longer needed
#pragma unroll
  for (int c0 = 0; c0 < BN; c0 += ECH) {
    // k-group 0 stores its accumulators, the other groups add theirs in turn
#pragma unroll
    for (int g = 0; g < KS; ++g) {
      if (kg == g) {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int b = 0; b < TN; ++b) {
            const int jl = wc * (BN / 2) + b * 16 + (lane & 15) - c0;
            if (jl < 0 || jl >= ECH) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              double* d = &pool[jl * (BM + 1) + wr * (BM / 2) + a * 16 + (lane >> 4) + 4 * r];
              *d = g == 0 ? acc[a][b][r] : *d + acc[a][b][r];
            }
          }
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < BM * ECH / NT; ++q) {
      const int e = threadIdx.x + NT * q;
      const int il = e % BM, jl = e / BM;
      const int i = i0 + il, j = j0 + c0 + jl;
      if (i >= m || j >= n) continue;
      if (LOWT && i < j) {
        if (MODE == 3 && C2) C2[i + (size_t)j * ldc2] = 0.0;  // (Phi's zero upper inside the diagonal tiles)
        continue;
      }
      if (UPT && i > j) continue;
      const double v = pool[jl * (BM + 1) + il];
      if (slab) {
        slab[(size_t)split * m * n + (size_t)j * m + i] = v;
      } else {
        double out;
        if (!use_c) {
          out = alpha * v;
        } else {
          double cv;
          if (PREFETCH_C) cv = cpre[(c0 / ECH) * (BM * ECH / NT) + q];
          else cv = C[i + (size_t)j * ldc];
          out = alpha * v + beta * cv;
        }
        C[i + (size_t)j * ldc] = out;
        if (MODE == 3 && i > j) C[j + (size_t)i * ldc] = out;
        if ((MODE == 4 || (MODE == 3 && C2)) && i >= j) C2[i + (size_t)j * ldc2] = i == j ? 0.5 * out : out;
        // (Phi's zero upper covers the diagonal 64-blocks whatever the tile: a
        // reader on 64 x 64 tiles cuts K to those.  A smaller tile below the
        // diagonal of such a block clears its mirror, which no tile owns)
        if (MODE == 3 && BM < 64 && C2 && i0 != j0 && (i >> 6) == (j >> 6)) C2[j + (size_t)i * ldc2] = 0.0;
      }
    }
    if (c0 + ECH < BN) __syncthreads();
  }
}

__global__ void k_splitk_reduce(int m, int n, int splits, const double* __restrict__ slab,
                                double alpha, double beta, double* __restrict__ C,
                                int ldc, int lower, int bz) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)m * n) return;
  const int i = (int)(idx % m), j = (int)(idx / m);
  if (lower == 1 && i < j) return;
  if (lower == 2 && i > j) return;
  double s = 0.0;
  for (int t = 0; t < splits; ++t) s += slab[(size_t)t * m * n + idx];
  double* c = C + i + (size_t)j * ldc;
  if ((bz > 0 && i >= bz) || (bz < 0 && j >= -bz)) beta = 0.0;  // (k_gemm's bz)
  *c = (beta == 0.0) ? alpha * s : alpha * s + beta * *c;
}

// the same reduction for an even m: a lane takes two rows of one column
// (16-byte slab loads, every split's load issued before the sum), a 2-D
// grid-stride walk instead of a 64-bit division per element, a bounded grid
// (the per-element form spent most of its time on index arithmetic: 44 us for
// four 512 x 2560 slabs)
__global__ __launch_bounds__(256) void k_splitk_reduce2(int m, int n, int splits, const double* __restrict__ slab,
                                                        double alpha, double beta, double* __restrict__ C, int ldc,
                                                        int lower, int bz) {
  const long long tot = (long long)m * n;
  for (smg_mn w(m >> 1, n); w.ok(); w.next()) {
    const int i = 2 * w.i, j = w.j;
    if (lower == 1 && i + 1 < j) continue;
    if (lower == 2 && i > j) continue;
    const long long e = (long long)j * m + i;
    d2v s = {0.0, 0.0};
    int t = 0;
    for (; t + 4 <= splits; t += 4) {
      const d2v a0 = *reinterpret_cast<const d2v*>(slab + (size_t)t * tot + e);
      const d2v a1 = *reinterpret_cast<const d2v*>(slab + (size_t)(t + 1) * tot + e);
      const d2v a2 = *reinterpret_cast<const d2v*>(slab + (size_t)(t + 2) * tot + e);
      const d2v a3 = *reinterpret_cast<const d2v*>(slab + (size_t)(t + 3) * tot + e);
      s += a0;
      s += a1;
      s += a2;
      s += a3;
    }
    for (; t < splits; ++t) s += *reinterpret_cast<const d2v*>(slab + (size_t)t * tot + e);
    double* c = C + i + (size_t)j * ldc;
    const bool w0 = !(lower == 1 && i < j), w1 = !(lower == 2 && i + 1 > j);
    // (k_gemm's bz; an even row boundary keeps both rows of the pair on one side)
    const double b = ((bz > 0 && i >= bz) || (bz < 0 && j >= -bz)) ? 0.0 : beta;
    if (w0) c[0] = (b == 0.0) ? alpha * s[0] : alpha * s[0] + b * c[0];
    if (w1) c[1] = (b == 0.0) ? alpha * s[1] : alpha * s[1] + b * c[1];
  }
}

// One product as it travels from an entry to launch:
// C = alpha op(A) op(B) + beta C, `batch` of them at strides sA / sB / sC.
struct gemm_args {
  int m, n, k;
  double alpha;
  const double* A;
  int lda;
  const double* B;
  int ldb;
  double beta;
  double* C;
  int ldc, tri = 0;  // (tri: SMG_TRI_* bits)
  int batch = 1;
  long long sA = 0, sB = 0, sC = 0;
  double* C2 = nullptr;  // the second output of MODE 4 and (optional: Phi) of MODE 3; null in every other mode
  int ldc2 = 0;
  int bz = 0;                 // the beta-zero boundary (k_gemm's bz; smg_gemm_bz_impl)
  int cut_a = -1, cut_b = -1;  // the offset triangular K cuts (-1: none; smg_gemm_cut_impl)
};

// Multiply-adds x 2 that the offset cuts take off a product without triangular
// operands, tile by tile as k_gemm skips them (gemm_k_range); a triangle of C
// counted by its elements, as smg_gemm_impl counts the uncut product.
template <int BM, int BN, int BK>
double cut_flops(int mode, const gemm_grid& g) {
  const int m = g.m, n = g.n;
  double f = 0.0;
  for (int j0 = 0; j0 < n; j0 += BN)
    for (int i0 = 0; i0 < m; i0 += BM) {
      int lo = g.k;  // the K this tile skips: what its splits' ranges leave out
      for (int s = 0; s < g.splits; ++s) {
        const gemm_krange kr = gemm_k_range<BM, BN, BK>(g, i0, j0, s);
        lo -= kr.kend - kr.kbeg;
      }
      if (lo == 0) continue;
      const int i1 = i0 + BM < m ? i0 + BM : m, j1 = j0 + BN < n ? j0 + BN : n;
      double el = 0.0;
      for (int j = j0; j < j1; ++j) {
        const int a = (mode == 1 || mode == 3) && j > i0 ? j : i0;  // lower: rows i >= j
        const int b = mode == 2 && j + 1 < i1 ? j + 1 : i1;         // upper: rows i <= j
        if (b > a) el += b - a;
      }
      f += 2.0 * lo * el;
    }
  return f;
}

template <int BM, int BN, int BK, bool TA, bool TB, int MODE, int KS = 1, int NB = 0>
int launch(smg_ctx* ctx, const gemm_args& a) {
  const int m = a.m, n = a.n;
  // (ctx->gemm_cut 0: every product ignores its offset cuts; 2: it takes them
  // in the uncut product's tile placement, smg_set_gemm_cut_mode)
  const gemm_grid g = gemm_plan<BM, BN, BK, MODE, NB>(m, n, a.k, a.tri, a.batch, ctx->gemm_cut, a.cut_a, a.cut_b);
  if (ctx->prof_on && !a.tri && (g.cut_a >= 0 || g.cut_b >= 0))
    ctx->prof_flops[SMG_FAM_GEMM] -= a.batch * cut_flops<BM, BN, BK>(MODE, g);
  const int splits = g.splits;
  double* slab = nullptr;
  if (splits > 1) {
    // the side and zeroing streams have their own slabs so concurrent split-K
    // GEMMs never share one
    const int slot = ctx->stream == ctx->side                                ? SMG_WS_GEMM_SIDE
                     : (ctx->zero_stream && ctx->stream == ctx->zero_stream) ? SMG_WS_GEMM_ZERO
                                                                             : SMG_WS_GEMM;
    slab = smg_ws(ctx, slot, (size_t)splits * m * n);
    if (!slab) return SMG_ERR_OOM;
  }
  hipLaunchKernelGGL((k_gemm<BM, BN, BK, TA, TB, MODE, KS, NB>), dim3(g.ntp * splits, a.batch), dim3(256 * KS), 0,
                     ctx->stream, m, n, a.k, a.alpha, a.A, a.lda, a.B, a.ldb, a.beta, a.C, a.ldc, g.tm, g.ntiles, g.kchunk,
                     slab, a.sA, a.sB, a.sC, g.px, g.ntp, a.tri, a.C2, a.ldc2, a.bz, g.cut_a, g.cut_b, g.cut_spread);
  if (splits > 1) {
    const long long tot = (long long)m * n;
    if ((m & 1) == 0) {
      const long long pairs = tot / 2;
      const int nb = (int)(pairs / 256 < 2048 ? (pairs + 255) / 256 : 2048);
      hipLaunchKernelGGL(k_splitk_reduce2, dim3(nb), dim3(256), 0, ctx->stream, m, n, splits, slab, a.alpha, a.beta,
                         a.C, a.ldc, MODE, a.bz);
    } else {
      hipLaunchKernelGGL(k_splitk_reduce, dim3(smg_ceil_div(tot, 256)), dim3(256), 0,
                         ctx->stream, m, n, splits, slab, a.alpha, a.beta, a.C, a.ldc, MODE, a.bz);
    }
  }
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

// Do two column-major blocks share an element?  Blocks with the same leading
// dimension are treated as rectangles of one matrix (the sub-blocks Murray's
// reverse works on: La[k:, j:k] vs La[j:k, 0:k] are disjoint although their
// address ranges interleave); otherwise the address ranges are compared.
inline bool overlaps(const double* X, int ldx, int rows, int cols, const double* C, int ldc, int m,
                     int n) {
  if (rows <= 0 || cols <= 0 || m <= 0 || n <= 0) return false;
  const double* x1 = X + (size_t)(cols - 1) * ldx + rows;
  const double* c1 = C + (size_t)(n - 1) * ldc + m;
  if (!(X < c1 && C < x1)) return false;
  if (ldx != ldc) return true;
  const double* base = X < C ? X : C;
  const long long ox = X - base, oc = C - base, ld = ldx;
  const long long rx = ox % ld, cx = ox / ld, rc = oc % ld, cc = oc / ld;
  return rx < rc + m && rc < rx + rows && cx < cc + n && cc < cx + cols;
}

// K stage of the 64 x 64 tile: 16 keeps two stages of registers and two LDS
// buffers within 32 KB per workgroup (four or more workgroups per CU)
constexpr int BK64 = 16;

// May the product take the DMA-staged 64 x 64 kernel (k_gemm's NB != 0)?
// Whole tiles, every K range (the triangular cuts are 64-aligned) in whole
// stages, and element pairs that are 16-byte aligned in every operand.
inline bool dma_eligible(int m, int n, int k, const double* A, int lda, const double* B, int ldb,
                         const double* C, int ldc) {
  constexpr int KQ = SMG_GEMM_DMA_BK1 > SMG_GEMM_DMA_BK2 ? SMG_GEMM_DMA_BK1 : SMG_GEMM_DMA_BK2;
  return m % 64 == 0 && n % 64 == 0 && k > 0 && k % KQ == 0 && !((lda | ldb | ldc) & 1) &&
         !(((size_t)A | (size_t)B | (size_t)C) & 15);
}

template <bool TA, bool TB, int MODE>
int dispatch_tile(smg_ctx* ctx, const gemm_args& a, bool aliased = false) {
  constexpr bool FULLC = MODE == 0 || MODE == 4;  // every tile of C computed
  const int m = a.m, n = a.n, k = a.k, tri = a.tri;
  // In-place products (C aliases an operand: the blocked TRSMs C = C Dinv,
  // L21 = A21 Dinv^T, X_p = W_p B_p) are race-free only when every workgroup
  // owns whole rows (C aliases A) or whole columns (C aliases B) of C.
  const bool alias_a = overlaps(a.A, a.lda, TA ? k : m, TA ? m : k, a.C, a.ldc, m, n);
  const bool alias_b = overlaps(a.B, a.ldb, TB ? n : k, TB ? k : n, a.C, a.ldc, m, n);
  if (alias_a || alias_b) {
    // (the symbolic step's products never alias; neither does one with a
    // beta-zero boundary or a second output: both are refused, not dropped)
    if (MODE == 3 || MODE == 4 || a.bz || a.C2) return SMG_ERR_ARG;
    if (MODE == 0 && alias_a && !alias_b && n <= 64) return launch<32, 64, 32, TA, TB, 0>(ctx, a);
    if (MODE == 0 && alias_b && !alias_a && m <= 64) return launch<64, 32, 32, TA, TB, 0>(ctx, a);
    // general aliasing: out of place through a workspace, then C = T (+ beta C).
    // The product into T keeps the triangles and the K cuts (they describe the
    // operands) and has no beta-zero boundary (bz is 0 here, and beta is).
    double* T = smg_ws(ctx, SMG_WS_ALIAS, (size_t)m * n);
    if (!T) return SMG_ERR_OOM;
    gemm_args t = a;
    t.beta = 0.0, t.C = T, t.ldc = m, t.bz = 0;
    int rc = dispatch_tile<TA, TB, MODE>(ctx, t, true);
    if (rc) return rc;
    if (a.beta == 0.0) return smg_copy_impl(ctx, m, n, T, m, a.C, a.ldc, 1.0, 0);
    if (a.beta != 1.0) {
      rc = smg_scale_impl(ctx, m, n, a.beta, a.C, a.ldc, MODE);
      if (rc) return rc;
    }
    return smg_copy_impl(ctx, m, n, T, m, a.C, a.ldc, 1.0, 1);
  }
  // tile size by how many CUs the output grid can occupy (256 CUs): large
  // outputs take 128x128 tiles (operand reuse), mid-size 64x64, and the
  // CU-starved shapes of the blocked Cholesky (one 64-wide block column or
  // row) 32x32, so the grid spreads over 4x more CUs
  const long long big_tiles = (long long)smg_ceil_div(m, 128) * smg_ceil_div(n, 128);
  const long long t64 = smg_ceil_div(m, 64);
  const long long mid_tiles =
      (!FULLC && m == n) ? t64 * (t64 + 1) / 2 : t64 * smg_ceil_div(n, 64);
  // The DMA-staged 64 x 64 kernel (full and lower C) for the eligible products
  // of the families, tile counts and K where it measured faster than what
  // the policy below takes (profiles/gemm_dma_stage_ubench.txt): from
  // SMG_GEMM_DMA_MIN_TILES tiles on, K >= 512, except the dense full products
  // large enough for 128 x 128 tiles (with a triangular operand the 64 x 64
  // grid's longest-K-first order wins there too).  8 waves up to
  // SMG_GEMM_DMA_KS2_MAX tiles, 4 above.  ctx->gemm_stage 1 never takes it,
  // 2 takes it for every eligible product (smg_set_gemm_stage_mode).
  if constexpr (MODE == 0 || MODE == 1) {
    constexpr int fam = MODE == 1 ? (!TA && TB ? 1 : TA && !TB ? 2 : !TA && !TB ? 16 : 0)
                                  : (!TA && !TB ? 4 : TA && !TB ? 8 : 0);
    const bool g128 = FULLC && big_tiles >= (tri ? SMG_GEMM_TRI128_MIN : 256) && k > 128;
    // (a grid below one tile per CU only while K is short: the long-K ones
    // need the split or the 4x finer grid, (512,1024,3072) TN 68 vs 102 us)
    const bool policy = (SMG_GEMM_DMA_FAMILIES & fam) && k >= 512 && !(g128 && !tri) &&
                        (mid_tiles >= 256 || (mid_tiles >= SMG_GEMM_DMA_MIN_TILES && k <= 1024));
    const bool want = ctx->gemm_stage == 2 || (ctx->gemm_stage == 0 && policy);
    if (want && !aliased && dma_eligible(m, n, k, a.A, a.lda, a.B, a.ldb, a.C, a.ldc)) {
      if (mid_tiles <= SMG_GEMM_DMA_KS2_MAX)
        return launch<64, 64, SMG_GEMM_DMA_BK2, TA, TB, MODE, 2, SMG_GEMM_DMA_NB2>(ctx, a);
      return launch<64, 64, SMG_GEMM_DMA_BK1, TA, TB, MODE, 1, SMG_GEMM_DMA_NB1>(ctx, a);
    }
  }
  // (triangle modes keep 64 x 64 tiles: half the 128-tile grid would sit on
  // the diagonal, and the split-K those few tiles need costs a reduction; at
  // N = K = 4096 the 528-tile 128 triangle -- 2.06 waves over the CUs -- ran
  // 1692 vs 1416 us for the 64 grid)
  // (a triangular operand gives the tiles K ranges from 128 to k: with one
  // 128 tile per CU the longest sets the time -- the 2048^3 products of the
  // inverse doubling ran at 27 TF/s -- so those need 4 per CU to balance,
  // else the 64 x 64 grid's longest-K-first order takes them)
  if (FULLC && big_tiles >= (tri ? SMG_GEMM_TRI128_MIN : 256) && k > 128)
    return launch<128, 128, 16, TA, TB, MODE>(ctx, a);
  // long-K transposed-A products with a small output (the Murray reverse's
  // [R_adj | D_adj] -= C_adj^T [B | C]: 512 x K x m, m >= 1536): 128 x 64
  // tiles split over K (tools/ubench_gemm: (512,2048,2048) 87 vs 100 us,
  // (512,1024,3072) 68 vs 81 us with 32 x 32)
  if (MODE == 0 && TA && !TB && k >= 1536 && mid_tiles < 512)
    return launch<128, 64, 16, TA, TB, MODE>(ctx, a);
  // 64 x 64 tiles from 256 tiles on (one per CU), with 8 waves (KS = 2: the
  // two wave groups split every K stage) up to ~6 tiles per CU; 32 x 32
  // below that (4x the workgroups), and for the tall NN products with
  // n <= 512 (C_adj D^{-1}, B_adj -= C_adj R at small J), where the
  // 4-wave 32 x 32 grid measured fastest.  tools/ubench_gemm at N = 4096
  // (us, 32x32 / 64x64 / 64x64 KS=2):
  //   (3584,512,512) NT lower 57.6 / 54.6 / 51.4   (512,3584,512) NN 49.6 / 51.8 / 47.3
  //   (2048,1536,512) NN 80.5 (64x64) / 70.6       (3072,512,512) NN 45.1 / 52.5 / 48.4
  //   (512,512,512) 11.5 (32x32) / 10.2 (32x32 KS=2)
  // (and a 64 x 64 grid below 256 tiles, split over K or not, loses to 32 x 32:
  // (3584,256,256) 18.6 vs 28 us)
  const bool tall_nn = MODE == 0 && !TA && !TB && n <= 512;
  if (mid_tiles >= 512 ? mid_tiles <= SMG_GEMM_KS2_MAX : (mid_tiles >= 256 && !tall_nn))
    return launch<64, 64, BK64, TA, TB, MODE, 2>(ctx, a);
  if (mid_tiles >= 512) return launch<64, 64, BK64, TA, TB, MODE>(ctx, a);
  const long long t32 = smg_ceil_div(m, 32);
  const long long small_tiles = (!FULLC && m == n) ? t32 * (t32 + 1) / 2 : t32 * smg_ceil_div(n, 32);
  if (small_tiles <= 256) return launch<32, 32, 32, TA, TB, MODE, 2>(ctx, a);
  return launch<32, 32, 32, TA, TB, MODE>(ctx, a);
}

// The one map from (ta, tb, mode) to the template arguments.  mode 0 to 4:
// k_gemm's MODE, the tile by dispatch_tile; BATCHED: the batched entry (full
// C, operands that do not alias), 64 x 64 tiles from 192 of them on, else 32 x 32.
constexpr int BATCHED = -1;
int dispatch(smg_ctx* ctx, int ta, int tb, int mode, const gemm_args& a) {
  auto go = [&](auto TA, auto TB) {
    constexpr bool ta_ = decltype(TA)::value, tb_ = decltype(TB)::value;
    switch (mode) {
      case BATCHED:
        if ((long long)smg_ceil_div(a.m, 64) * smg_ceil_div(a.n, 64) * a.batch >= 192)
          return launch<64, 64, BK64, ta_, tb_, 0>(ctx, a);
        return launch<32, 32, 32, ta_, tb_, 0>(ctx, a);
      case 1: return dispatch_tile<ta_, tb_, 1>(ctx, a);
      case 2: return dispatch_tile<ta_, tb_, 2>(ctx, a);
      case 3: return dispatch_tile<ta_, tb_, 3>(ctx, a);
      case 4: return dispatch_tile<ta_, tb_, 4>(ctx, a);
      default: return dispatch_tile<ta_, tb_, 0>(ctx, a);
    }
  };
  if (!ta && !tb) return go(std::false_type{}, std::false_type{});
  if (!ta && tb) return go(std::false_type{}, std::true_type{});
  if (ta && !tb) return go(std::true_type{}, std::false_type{});
  return go(std::true_type{}, std::true_type{});
}

}  // namespace

// batch x (C_i = alpha op(A_i) op(B_i) + beta C_i), operand i at base + i * stride
// (doubles); full C only, no split-K, operands must not alias
int smg_gemm_batched_impl(smg_ctx* ctx, int ta, int tb, int m, int n, int k, double alpha,
                          const double* A, int lda, long long sA, const double* B, int ldb,
                          long long sB, double beta, double* C, int ldc, long long sC, int batch) {
  if (m <= 0 || n <= 0 || batch <= 0) return SMG_OK;
  if (k <= 0 || alpha == 0.0) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GEMM);
  if (ctx->prof_on) ctx->prof_flops[SMG_FAM_GEMM] += 2.0 * m * n * k * batch;
  gemm_args a = {m, n, k, alpha, A, lda, B, ldb, beta, C, ldc};
  a.batch = batch, a.sA = sA, a.sB = sB, a.sC = sC;
  return dispatch(ctx, ta, tb, BATCHED, a);
}

int smg_gemm_impl(smg_ctx* ctx, int ta, int tb, int uplo, int m, int n, int k,
                  double alpha, const double* A, int lda, const double* B, int ldb,
                  double beta, double* C, int ldc, int tri) {
  return smg_gemm_cut_impl(ctx, ta, tb, uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri, 0, -1, -1);
}

// smg_gemm_impl with beta taken as 0 for C's rows from bz on (bz > 0) or its
// columns from -bz on (bz < 0): the first contribution to that region of an
// accumulated product, which then needs no zeroing beforehand.  |bz| must be a
// multiple of 128 (every tile lies on one side of it).
int smg_gemm_bz_impl(smg_ctx* ctx, int ta, int tb, int uplo, int m, int n, int k, double alpha, const double* A,
                     int lda, const double* B, int ldb, double beta, double* C, int ldc, int tri, int bz) {
  return smg_gemm_cut_impl(ctx, ta, tb, uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri, bz, -1, -1);
}

// smg_gemm_bz_impl (bz = 0: none) for operands with an offset triangle of
// stored zeros, whose K range every tile skips (-1: no such triangle):
//   cut_a >= 0: op(A)(i, t) = 0 for t < i - cut_a in the rows i >= cut_a,
//   cut_b >= 0: op(B)(t, j) = 0 for t < j - cut_b in the columns j >= cut_b.
// The tile order, the kernel and its staging are chosen as without the cuts.
int smg_gemm_cut_impl(smg_ctx* ctx, int ta, int tb, int uplo, int m, int n, int k, double alpha, const double* A,
                      int lda, const double* B, int ldb, double beta, double* C, int ldc, int tri, int bz, int cut_a,
                      int cut_b) {
  if (bz % 128 || cut_a < -1 || cut_b < -1) return SMG_ERR_ARG;
  if (m <= 0 || n <= 0) return SMG_OK;
  if (k <= 0 || alpha == 0.0) {
    if (beta == 1.0) return SMG_OK;
    return smg_scale_impl(ctx, m, n, beta, C, ldc, uplo);
  }
  smg_prof_scope prof(ctx, SMG_FAM_GEMM);
  if (ctx->prof_on) {
    // the K cuts of triangular operands execute about half (one) or a third
    // (two, as in V V^T with a triangle output) of the dense count
    const double cut = (tri & 3) && (tri & 12) ? 1.0 / 3.0 : (tri ? 0.5 : 1.0);
    ctx->prof_flops[SMG_FAM_GEMM] +=
        cut * (uplo ? 2.0 * k * ((double)m * n - (double)n * (n - 1) / 2) : 2.0 * m * n * k);
  }
  gemm_args a = {m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri};
  a.bz = bz, a.cut_a = cut_a, a.cut_b = cut_b;
  // uplo 1 / 2: the lower / upper triangle of C; 3: the lower half computed, stored mirrored (symmetric C)
  return dispatch(ctx, ta, tb, uplo >= 1 && uplo <= 3 ? uplo : 0, a);
}

// C = alpha op(A) op(B) + beta C (full) and C2 = tril(C) with halved diagonal
int smg_gemm_dual_impl(smg_ctx* ctx, int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda,
                       const double* B, int ldb, double beta, double* C, int ldc, double* C2, int ldc2, int tri) {
  if (m <= 0 || n <= 0) return SMG_OK;
  if (k <= 0 || alpha == 0.0 || !C2) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GEMM);
  if (ctx->prof_on) ctx->prof_flops[SMG_FAM_GEMM] += 2.0 * m * n * k;
  gemm_args a = {m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri};
  a.C2 = C2, a.ldc2 = ldc2;
  return dispatch(ctx, ta, tb, 4, a);
}

// C = alpha op(A) op(B) + beta C, symmetric: its lower triangle computed and
// stored mirrored (uplo 3), and P = Phi(C) (strict lower, halved diagonal) as
// a second output.  P's strict upper is written (zeros) only inside the
// diagonal 64-blocks: a reader must cut K to P's lower triangle
// (SMG_TRI_B_LOWER / TRI_B_UPPER on P^T), as the Cholesky tangent's do.
int smg_gemm_sym_phi_impl(smg_ctx* ctx, int ta, int tb, int n, int k, double alpha, const double* A, int lda,
                          const double* B, int ldb, double beta, double* C, int ldc, double* P, int ldp, int tri) {
  if (n <= 0) return SMG_OK;
  if (k <= 0 || alpha == 0.0 || !P) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_GEMM);
  if (ctx->prof_on) {
    const double cut = (tri & 3) && (tri & 12) ? 1.0 / 3.0 : (tri ? 0.5 : 1.0);
    ctx->prof_flops[SMG_FAM_GEMM] += cut * 2.0 * k * ((double)n * n - (double)n * (n - 1) / 2);
  }
  gemm_args a = {n, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri};
  a.C2 = P, a.ldc2 = ldp;
  return dispatch(ctx, ta, tb, 3, a);
}

extern "C" int smg_gemm_tri(smg_ctx* ctx, int ta, int tb, int uplo, int tri, int m, int n, int k,
                            double alpha, const double* A, int lda, const double* B, int ldb, double beta,
                            double* C, int ldc) {
  if (!ctx || m < 0 || n < 0 || k < 0 || tri < 0 || tri > 15) return SMG_ERR_ARG;
  if ((m > 0 && n > 0) && (!C || ldc < m)) return SMG_ERR_ARG;
  if (k > 0 && m > 0 && n > 0 && alpha != 0.0) {
    if (!A || !B) return SMG_ERR_ARG;
    if (lda < (ta ? k : m) || ldb < (tb ? n : k)) return SMG_ERR_ARG;
  }
  return smg_gemm_impl(ctx, ta, tb, uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri);
}

extern "C" int smg_gemm_bz(smg_ctx* ctx, int ta, int tb, int uplo, int tri, int m, int n, int k, double alpha,
                           const double* A, int lda, const double* B, int ldb, double beta, double* C, int ldc,
                           int bz) {
  if (!ctx || m <= 0 || n <= 0 || k <= 0 || tri < 0 || tri > 15 || alpha == 0.0) return SMG_ERR_ARG;
  if (!A || !B || !C || ldc < m || lda < (ta ? k : m) || ldb < (tb ? n : k)) return SMG_ERR_ARG;
  return smg_gemm_bz_impl(ctx, ta, tb, uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri, bz);
}

extern "C" int smg_gemm_cut(smg_ctx* ctx, int ta, int tb, int uplo, int tri, int m, int n, int k, double alpha,
                            const double* A, int lda, const double* B, int ldb, double beta, double* C, int ldc,
                            int bz, int cut_a, int cut_b) {
  if (!ctx || m <= 0 || n <= 0 || k <= 0 || tri < 0 || tri > 15 || alpha == 0.0) return SMG_ERR_ARG;
  if (!A || !B || !C || ldc < m || lda < (ta ? k : m) || ldb < (tb ? n : k)) return SMG_ERR_ARG;
  return smg_gemm_cut_impl(ctx, ta, tb, uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri, bz, cut_a, cut_b);
}

extern "C" int smg_gemm(smg_ctx* ctx, int ta, int tb, int uplo, int m, int n, int k,
                        double alpha, const double* A, int lda, const double* B,
                        int ldb, double beta, double* C, int ldc) {
  if (!ctx || m < 0 || n < 0 || k < 0) return SMG_ERR_ARG;
  if ((m > 0 && n > 0) && (!C || ldc < m)) return SMG_ERR_ARG;
  if (k > 0 && m > 0 && n > 0 && alpha != 0.0) {
    if (!A || !B) return SMG_ERR_ARG;
    if (lda < (ta ? k : m) || ldb < (tb ? n : k)) return SMG_ERR_ARG;
  }
  return smg_gemm_impl(ctx, ta, tb, uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc);
}
