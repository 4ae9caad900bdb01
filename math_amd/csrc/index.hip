// Indexing a device vector by group, forward and reverse: the gather
// dst[i] (+)= src[g[i]-1] and its transpose, the per-destination sums
// out[j] (+)= sum of v over the rows of destination j (rev/fun/index_ops.hpp).
// Indices are 1-based.  Nothing synchronises with the host, and no kernel
// uses an atomic: every sum has one owner and a fixed order, so the results
// are bitwise repeatable.
//
// k_gather: a streaming map over i under elt.hip's launch rule (256-thread
// blocks, at most 8192 of them, a grid-stride loop); a lane takes two
// adjacent rows per trip (one 8-byte read of g, one 16-byte access to dst)
// when dst is on a 16-byte and g on an 8-byte boundary, else one row.  The
// reads of src are indexed.
//
// smg_segment_sum works on the inverted index: perm lists the rows sorted by
// destination (stably), offs[j]..offs[j+1] is destination j's range of it.
// The SORTED LIST, not the destinations, is cut into tiles of SEG_TILE
// entries.  k_segment_starts finds the destination of every tile's first
// entry by binary search in offs, one thread per tile, into ws (all searches
// at once: inside the tile kernel the same search, some twenty dependent
// loads at J = 2^20, stood at the head of every block and cost 0.04 ms of a
// 0.15 ms call at R = 2^24).  Then one block per tile (k_segment_tiles):
//   - the block marks in LDS the entry at which each destination of the tile
//     begins (a loop over the destinations from its first entry's to the next
//     tile's; an empty one it meets is zeroed unless accumulating);
//   - the entries' values v[perm[k]] go through LDS (coalesced reads of perm),
//     so that a thread holds SEG_PER_THREAD consecutive entries;
//   - a segmented sum over the tile in a fixed order: per thread, then a
//     segmented scan over the wave's lanes and over the block's waves;
//   - a destination that begins and ends inside the tile is finished there
//     (one owner: load, add, store, in a last pass over the tile in which
//     neighbouring threads take neighbouring destinations: with every thread
//     storing its own finished sums, R = 2^24 singletons took 0.236 ms, this
//     way 0.180 ms); one that crosses a tile edge leaves one
//     partial per tile in ws: slot 2t for the destination that holds tile t's
//     first entry, slot 2t+1 for another one that runs past its last.
//     The tiles' first destinations follow the partials, from ws[2 tiles] on,
//     stored as doubles (exact: J < 2^31).
// k_segment_combine, a further plain launch on the same stream, has one block
// per tile boundary: the block of the FIRST boundary a destination crosses
// sums its partials (threads stride over the tiles in order, then the fixed
// block sum) and stores the total; every other block returns at once.  The order of every sum depends on (R, J, offs) only.
#include "smg_internal.h"

namespace {

constexpr int MAP_THREADS = 256;      // elt.hip's ELT_THREADS / ELT_MAX_BLOCKS (its map_grid)
constexpr int MAP_MAX_BLOCKS = 8192;
constexpr int MAP_WIDTH = 2;          // rows per lane and trip of an aligned gather
constexpr int SEG_THREADS = 256;
constexpr int SEG_PER_THREAD = 8;
constexpr int SEG_TILE = SEG_THREADS * SEG_PER_THREAD;  // T: entries of the sorted list per block
constexpr int SEG_WAVES = SEG_THREADS / 64;
constexpr int COMBINE_THREADS = 256;

inline int map_width(const smg_ctx* ctx) { return ctx->elt_width ? ctx->elt_width : MAP_WIDTH; }
inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline int map_grid(long long n, int W) {
  long long g = (n / W + MAP_THREADS - 1) / MAP_THREADS;
  if (g > MAP_MAX_BLOCKS) g = MAP_MAX_BLOCKS;
  if (g < 1) g = 1;
  return (int)g;
}

template <int W, bool ACC>
__global__ void __launch_bounds__(MAP_THREADS) k_gather(const double* __restrict__ src, const int* __restrict__ g,
                                                        long long n, double* __restrict__ dst) {
  const long long stride = (long long)gridDim.x * blockDim.x * W;
  const long long end = W == 2 ? (n & ~1LL) : n;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * W; i < end; i += stride) {
    if (W == 2) {
      const int2 gi = *reinterpret_cast<const int2*>(g + i);
      d2v r;
      r.x = src[gi.x - 1];
      r.y = src[gi.y - 1];
      if (ACC) {
        const d2v o = *reinterpret_cast<const d2v*>(dst + i);
        r.x = o.x + r.x;
        r.y = o.y + r.y;
      }
      *reinterpret_cast<d2v*>(dst + i) = r;
    } else {
      const double r = src[g[i] - 1];
      dst[i] = ACC ? dst[i] + r : r;
    }
  }
  if (W == 2 && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double r = src[g[n - 1] - 1];
    dst[n - 1] = ACC ? dst[n - 1] + r : r;
  }
}

// the destination that holds entry k of the sorted list (0 <= k < R = offs[J]):
// the j with offs[j] <= k < offs[j+1]
__device__ __forceinline__ long long dest_of(const long long* __restrict__ offs, long long J, long long k) {
  long long lo = 0, hi = J;  // offs[lo] <= k < offs[hi]
  while (hi - lo > 1) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (offs[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}

// the sum that is open at the end of a range of entries: s since the latest
// beginning of a destination in the range (f: there is one; pos: at which
// entry of the tile), else over the whole range
struct seg_run {
  double s;
  int pos;
  int f;
};
__device__ __forceinline__ seg_run seg_join(const seg_run& a, const seg_run& b) {  // a's range, then b's
  if (b.f) return b;
  seg_run r;
  r.s = a.s + b.s;
  r.pos = a.pos;
  r.f = a.f;
  return r;
}
__device__ __forceinline__ seg_run seg_shfl_up(const seg_run& x, int off) {
  seg_run r;
  r.s = __shfl_up(x.s, off, 64);
  r.pos = __shfl_up(x.pos, off, 64);
  r.f = __shfl_up(x.f, off, 64);
  return r;
}

// the LDS slot of the tile's entry p: one pad per SEG_PER_THREAD entries, so
// that the threads' reads of their consecutive entries spread over the banks
__device__ __forceinline__ int seg_slot(int p) { return p + p / SEG_PER_THREAD; }

// starts[t] = the destination of tile t's first entry
__global__ void __launch_bounds__(SEG_THREADS) k_segment_starts(const long long* __restrict__ offs, long long J,
                                                                long long tiles, double* __restrict__ starts) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < tiles) starts[t] = (double)dest_of(offs, J, t * SEG_TILE);
}

template <bool ACC>
__global__ void __launch_bounds__(SEG_THREADS) k_segment_tiles(const double* __restrict__ v,
                                                               const int* __restrict__ perm,
                                                               const long long* __restrict__ offs, long long R,
                                                               long long J, const double* __restrict__ starts,
                                                               double* __restrict__ ws, double* __restrict__ out) {
  __shared__ double val[SEG_TILE + SEG_TILE / SEG_PER_THREAD];
  __shared__ int head[SEG_TILE];  // the destination that begins at the entry, or -1
  __shared__ double wagg_s[SEG_WAVES];  // what is open at each wave's end (a seg_run, by field)
  __shared__ int wagg_pos[SEG_WAVES], wagg_f[SEG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long tile = blockIdx.x;
  const long long k0 = tile * SEG_TILE;
  const long long k1 = k0 + SEG_TILE < R ? k0 + SEG_TILE : R;
  const int n = (int)(k1 - k0);
  const bool last_tile = k1 == R;

  // the entries' values, and no beginnings yet
#pragma unroll
  for (int i = 0; i < SEG_PER_THREAD; ++i) {
    const int p = tid + i * SEG_THREADS;
    val[seg_slot(p)] = p < n ? v[perm[k0 + p]] : 0.0;
    head[p] = -1;
  }
  // the destinations of this tile's and of the next tile's first entry (k_segment_starts)
  const long long jb = (long long)starts[tile];
  const long long jnext = last_tile ? J - 1 : (long long)starts[tile + 1];
  const bool first_begins_here = offs[jb] == k0;
  __syncthreads();
  // the destinations this tile looks at: from its first entry's (tile 0: from
  // 0) to the next tile's first entry's (the last tile: to J - 1).  The empty
  // ones strictly between two tiles' first destinations, before the first and
  // after the last belong to exactly one tile.
  const long long jfrom = tile == 0 ? 0 : jb;
  const long long jto = jnext + 1;
  for (long long j = jfrom + tid; j < jto; j += SEG_THREADS) {
    const long long s = offs[j], e = offs[j + 1];
    if (s == e) {
      if (!ACC) out[j] = 0.0;
    } else if (j == jb) {
      head[0] = (int)j;
    } else if (s >= k0 && s < k1) {
      head[(int)(s - k0)] = (int)j;
    }
  }
  __syncthreads();

  // this thread's consecutive entries
  double x[SEG_PER_THREAD];
  int h[SEG_PER_THREAD];
  seg_run mine;
  mine.s = 0.0;
  mine.pos = -1;
  mine.f = 0;
#pragma unroll
  for (int i = 0; i < SEG_PER_THREAD; ++i) {
    const int p = tid * SEG_PER_THREAD + i;
    x[i] = val[seg_slot(p)];
    h[i] = head[p];
    if (h[i] >= 0) {
      mine.s = 0.0;
      mine.pos = p;
      mine.f = 1;
    }
    mine.s += x[i];
  }
  // segmented inclusive scan over the wave, the waves' ends through LDS
  seg_run inc = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const seg_run o = seg_shfl_up(inc, off);
    if (lane >= off) inc = seg_join(o, inc);
  }
  if (lane == 63) {
    wagg_s[wv] = inc.s;
    wagg_pos[wv] = inc.pos;
    wagg_f[wv] = inc.f;
  }
  seg_run before = seg_shfl_up(inc, 1);  // what is open when this thread's entries start
  if (lane == 0) {
    before.s = 0.0;
    before.pos = -1;
    before.f = 0;
  }
  __syncthreads();  // (every thread has also read its entries of val: the sums below reuse it)
  seg_run carry;
  carry.s = 0.0;
  carry.pos = -1;
  carry.f = 0;
#pragma unroll
  for (int w = 0; w < SEG_WAVES - 1; ++w) {  // (unrolled over every wave: a loop to wv put the struct in scratch)
    seg_run a;
    a.s = wagg_s[w];
    a.pos = wagg_pos[w];
    a.f = wagg_f[w];
    if (w < wv) carry = seg_join(carry, a);
  }
  before = seg_join(carry, before);

  // A finished sum whose destination begins and ends in this tile is left in
  // val at the entry where the destination begins, for the coalesced pass
  // below; any other is the tile's partial for it, and its mark is taken away.
  // Only the destination of the tile's first entry (the one at entry 0) can
  // have begun before the tile.
  auto close = [&](int pos, double total, bool ends_here) {
    if ((pos != 0 || first_begins_here) && ends_here) {
      val[seg_slot(pos)] = total;
    } else {
      ws[2 * tile + (pos == 0 ? 0 : 1)] = total;
      head[pos] = -1;
    }
  };
  double cur = before.s;
  int cur_pos = before.pos;
#pragma unroll
  for (int i = 0; i < SEG_PER_THREAD; ++i) {
    if (h[i] >= 0) {
      if (cur_pos >= 0) close(cur_pos, cur, true);
      cur = 0.0;
      cur_pos = tid * SEG_PER_THREAD + i;
    }
    cur += x[i];
  }
  if (tid == SEG_THREADS - 1) close(cur_pos, cur, offs[head[cur_pos] + 1] <= k1);
  __syncthreads();
  // the finished destinations: one owner each, neighbours in the tile by
  // neighbouring threads (stores of a run of small destinations coalesce)
#pragma unroll
  for (int i = 0; i < SEG_PER_THREAD; ++i) {
    const int p = tid + i * SEG_THREADS;
    const int id = head[p];
    if (id >= 0) {
      const double total = val[seg_slot(p)];
      out[id] = ACC ? out[id] + total : total;
    }
  }
}

template <bool ACC>
__global__ void __launch_bounds__(COMBINE_THREADS) k_segment_combine(const long long* __restrict__ offs,
                                                                    const double* __restrict__ starts,
                                                                    const double* __restrict__ ws,
                                                                    double* __restrict__ out) {
  const long long b = (long long)blockIdx.x + 1;  // the boundary between tiles b - 1 and b
  const long long p = b * SEG_TILE;
  const long long j = (long long)starts[b];
  const long long s = offs[j];
  if (s >= p || s / SEG_TILE != b - 1) return;  // nothing crosses here, or an earlier boundary's wave owns it
  const long long ta = b - 1, tb = (offs[j + 1] - 1) / SEG_TILE;
  // a thread's tiles are COMBINE_THREADS apart; four running sums keep four
  // loads in flight (one wave with one running sum took 0.03 ms over the
  // 8192 partials of a single destination at R = 2^24)
  __shared__ double lds[16];
  auto part = [&](long long t) { return t <= tb ? ws[2 * t + (t == ta && s != ta * SEG_TILE ? 1 : 0)] : 0.0; };
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (long long t = ta + threadIdx.x; t <= tb; t += 4 * COMBINE_THREADS) {
    s0 += part(t);
    s1 += part(t + COMBINE_THREADS);
    s2 += part(t + 2 * COMBINE_THREADS);
    s3 += part(t + 3 * COMBINE_THREADS);
  }
  const double sum = block_sum((s0 + s1) + (s2 + s3), lds);
  if (threadIdx.x == 0) out[j] = ACC ? out[j] + sum : sum;
}

inline long long seg_tiles(long long R) { return (R + SEG_TILE - 1) / SEG_TILE; }

}  // namespace

extern "C" {

int smg_index_launch_shape(smg_ctx* ctx, int* shape) {
  if (!ctx || !shape) return SMG_ERR_ARG;
  shape[0] = SEG_THREADS;
  shape[1] = SEG_TILE;
  shape[2] = MAP_THREADS;
  shape[3] = MAP_MAX_BLOCKS;
  shape[4] = map_width(ctx);
  return SMG_OK;
}

int smg_gather(smg_ctx* ctx, const double* src, const int* g, long long R, int accumulate, double* dst) {
  if (!ctx || R < 0) return SMG_ERR_ARG;
  if (R == 0) return SMG_OK;
  if (!src || !g || !dst) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_ELEMWISE);
  const bool wide = map_width(ctx) == 2 && aligned_to(dst, 16) && aligned_to(g, 8);
#define LAUNCH(W, ACC) \
  hipLaunchKernelGGL((k_gather<W, ACC>), dim3(map_grid(R, W)), dim3(MAP_THREADS), 0, ctx->stream, src, g, R, dst)
  if (wide) {
    if (accumulate) LAUNCH(2, true); else LAUNCH(2, false);
  } else {
    if (accumulate) LAUNCH(1, true); else LAUNCH(1, false);
  }
#undef LAUNCH
  SMG_LAUNCH_CHECK();
  return SMG_OK;
}

long long smg_segment_sum_ws_doubles(long long R, long long J) {
  (void)J;
  return R > 0 ? 3 * seg_tiles(R) : 3;  // two partials and the first destination per tile
}

int smg_segment_sum(smg_ctx* ctx, const double* v, const int* perm, const long long* offs, long long R, long long J,
                    int accumulate, double* ws, double* out) {
  if (!ctx || R < 0 || J < 0 || R > 0x7fffffffLL || J > 0x7fffffffLL) return SMG_ERR_ARG;
  if (R == 0 || J == 0) return SMG_OK;
  if (!v || !perm || !offs || !ws || !out) return SMG_ERR_ARG;
  smg_prof_scope prof(ctx, SMG_FAM_ELEMWISE);
  const long long tiles = seg_tiles(R);
  double* starts = ws + 2 * tiles;
  hipLaunchKernelGGL(k_segment_starts, dim3((unsigned)smg_ceil_div(tiles, SEG_THREADS)), dim3(SEG_THREADS), 0,
                     ctx->stream, offs, J, tiles, starts);
  if (accumulate)
    hipLaunchKernelGGL((k_segment_tiles<true>), dim3((unsigned)tiles), dim3(SEG_THREADS), 0, ctx->stream, v, perm, offs,
                       R, J, starts, ws, out);
  else
    hipLaunchKernelGGL((k_segment_tiles<false>), dim3((unsigned)tiles), dim3(SEG_THREADS), 0, ctx->stream, v, perm,
                       offs, R, J, starts, ws, out);
  SMG_LAUNCH_CHECK();
  if (tiles > 1) {
    if (accumulate)
      hipLaunchKernelGGL((k_segment_combine<true>), dim3((unsigned)(tiles - 1)), dim3(COMBINE_THREADS), 0, ctx->stream,
                         offs, starts, ws, out);
    else
      hipLaunchKernelGGL((k_segment_combine<false>), dim3((unsigned)(tiles - 1)), dim3(COMBINE_THREADS), 0,
                         ctx->stream, offs, starts, ws, out);
    SMG_LAUNCH_CHECK();
  }
  return SMG_OK;
}

}  // extern "C"
