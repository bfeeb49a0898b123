// Full-catalogue top-K retrieval for the LTHM towers, for gfx950.
//
//   scores[q, :k], rows[q, :k] = the k best items of  s[q, j] = qn[q] . items[j]
// under the total order (score descending, row ascending), with no [Q, N] buffer:
//   retr_prep_k   queries -> bf16 (optionally through F.normalize, as rownorm_v8_k does for the
//                 loss), and target_score[q] = qn[q] . items[target_row[q]] as a plain f32 dot;
//   retr_topk_k   grid (query tiles of 64) x (catalogue slabs): the block keeps its queries as
//                 MFMA B fragments, streams the slab's item rows through two LDS images and
//                 keeps, per query, the candidates that pass a threshold filter (below);
//   retr_merge_k  one wave per query merges the slabs' sorted k-lists and sums their counts.
// A candidate travels as one 64-bit key: the score's order-preserving integer image in the
// high word, ~row in the low word, so that "a precedes b" in the total order is key_a > key_b
// and the key 0 is free to mean "empty".  Selection never depends on the order in which the
// LDS atomics hand out slots (a prune writes each key at its rank), so the result is a pure
// function of the inputs.  No global atomics in any of these kernels (the plan of the clustered
// scan at the end of this file counts its pairs with two integer atomics that no output depends on).
//
// Exclusion (lthm_retrieve_topk_excl): every query may name up to RT_XMAX catalogue rows that
// are scored as -inf, so that they take none of the k slots and never count in the rank.
//   retr_excl_prep_k  sorts each query's list ascending into the workspace ([Q, X + 1] with
//                     ignored entries and the sentinel at index X set to INT_MAX);
//   retr_topk_k<true> a lane owns one query and a tile covers 64 consecutive rows, so the lane
//                     walks its sorted list with one cursor and sets the accumulator elements
//                     of excluded rows to -inf before the count and the filter see them.
// The plain call runs retr_topk_k<false>, which holds none of this.
//
// Groups (lthm_retrieve_topk_group): user u has G <= 8 queries and an item's score is its best
// over them, s[u, j] = max_g s_g[u, j].  The queries are laid out in slots, GP = next power of
// two of G per user (retr_prep_group_k; a pad slot repeats the user's first query, since a zero
// vector would score 0 and beat every negative score), so a user's slots are GP adjacent MFMA
// columns: GP adjacent lanes of one wave half.  retr_topk_k<EXCL, GP> takes the maximum of every
// accumulator element over those lanes, and the group's first lane (the leader) alone counts,
// masks, filters and appends, for the user: lists, targets, keys and counts are per user.  The
// other lanes of a group are inert the way the queries past Q are.
//
// Tags (lthm_retrieve_topk_tags): the catalogue carries one 32-bit attribute word per row and
// every query (user) a filter (all, any, none); a row that fails its query's filter is scored as
// -inf exactly as an excluded row is.  retr_topk_k<EXCL, GP, true> stages the 64 tag words of
// tile i + 1 with the image of tile i + 1 (one more LDS-DMA of wave 0, retired by the same wait
// and barrier), reads its 16 rows' words back as four broadcast 16-byte LDS reads, and masks the
// accumulator next to the exclusion mask.  The instantiations without tags hold none of this.
//
// Cursors (lthm_retrieve_topk_after): a query (user) may start its list behind a position
// (after_score, after_row) of the total order; a row at or before it is scored as -inf exactly
// as an excluded row is.  retr_topk_k<true, GP, TAGS, true> keeps the cursor in two registers
// and masks the accumulator next to the other masks; the instantiations without it hold none of
// this.  Since a (query, row) score does not depend on the slab cut, a page's last (score, row)
// as the next call's cursor continues the same order without a gap or a duplicate.
//
// Priors (lthm_retrieve_topk_bias): the catalogue may carry one f32 bias per row and a query (user)
// a weight, and the score becomes s = fmaf(weight, bias[row], dot), one explicit f32 fma on the
// MFMA's score, before anything looks at a score.  retr_topk_k<true, GP, TAGS, true, true> stages
// the 64 bias words of tile i + 1 with its image (one more LDS-DMA, of wave 1, retired by the same
// wait and barrier), reads its 16 rows' words back as four broadcast 16-byte LDS reads and applies
// 16 fmas behind the group maximum and ahead of every mask.  retr_bias_target_k gives the target
// score the same fma between the prep kernel and the scan, so that the value written out is the
// value counted against.  The instantiations without a prior hold none of this.
#include "mfma.hpp"

#include <climits>
#include <cmath>
#include <type_traits>

namespace lthm {
namespace {

typedef unsigned long long u64;

constexpr int RT_D = 128;     // LOSS_DE: the one embedding width
constexpr int RT_QT = 64;     // queries per block (two waves of 32 MFMA columns)
constexpr int RT_IT = 64;     // item rows per LDS image (two waves of 32 MFMA rows)
constexpr int RT_KMAX = 128;  // largest k
constexpr int RT_CAP = 192;   // candidate slots per query
constexpr int RT_LIM = RT_CAP - RT_IT;  // a query's count at the start of every tile is <= RT_LIM
// The selection invariant: a prune leaves at most k <= RT_KMAX candidates, a tile appends at
// most RT_IT per query (one per item row), and a query is pruned before the next tile
// whenever its count is above RT_LIM.  So no append can run past the buffer.
static_assert(RT_KMAX <= RT_LIM, "a pruned buffer must have a whole item tile of free slots");
static_assert(RT_LIM + RT_IT <= RT_CAP, "a tile's appends must fit behind the limit");

struct RetrShared {
  unsigned char img[2][RT_IT * 256];
  u64 cand[RT_QT][RT_CAP];
  float tau[RT_QT];  // current k-th best score of the query (-inf until k candidates are held)
  int cnt[RT_QT];    // candidates held
  int pc[RT_QT];     // #{rows of the slab scoring above the target}
  int flag[3];       // flag[i % 3]: tile i pushed some query past RT_LIM
};
static_assert(sizeof(RetrShared) <= 160 * 1024, "LDS budget");
// retr_topk_k<.., .., true>: the tag words of the two images' rows behind the plain layout
struct RetrSharedTags : RetrShared {
  alignas(16) int tag[2][RT_IT];  // a lane reads four words at once
};
static_assert(sizeof(RetrSharedTags) <= 160 * 1024, "LDS budget");
// retr_topk_k<.., .., TAGS, .., true>: the bias words of the two images' rows behind the layout of
// <.., .., TAGS>
template <class Base>
struct RetrSharedBias : Base {
  alignas(16) float bias[2][RT_IT];  // a lane reads four words at once
};
static_assert(sizeof(RetrSharedBias<RetrSharedTags>) <= 160 * 1024, "LDS budget");

__device__ __attribute__((aligned(16))) unsigned char retr_zero_row[256];
__device__ int retr_zero_tag;  // the tag of a row at or past the slab's end
__device__ float retr_zero_bias;  // and its bias

// the order-preserving integer image of a score, and back
__device__ __forceinline__ uint32_t retr_image(float s) {
  uint32_t u = __float_as_uint(s + 0.f);  // -0 -> +0: equal scores get equal images
  u ^= (uint32_t)((int32_t)u >> 31) | 0x80000000u;
  return u;
}
__device__ __forceinline__ float retr_image_score(uint32_t o) {
  return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu));
}
__device__ __forceinline__ u64 retr_key(float s, int row) { return ((u64)retr_image(s) << 32) | (uint32_t)~row; }
__device__ __forceinline__ float retr_key_score(u64 key) { return retr_image_score((uint32_t)(key >> 32)); }
__device__ __forceinline__ int retr_key_row(u64 key) { return (int)~(uint32_t)key; }

// One wave sorts buf[0, n) (distinct keys, n <= 64 PL) descending and keeps the first k:
// every key is written at its rank, the number of keys above it.  Returns min(n, k).
template <int PL>
__device__ __forceinline__ int retr_prune(u64* buf, int n, int k, int lane) {
  u64 key[PL];
  int rk[PL];
#pragma unroll
  for (int j = 0; j < PL; ++j) {
    const int idx = lane + 64 * j;
    key[j] = idx < n ? buf[idx] : 0ull;
    rk[j] = 0;
  }
  for (int i = 0; i < n; ++i) {
    const u64 kk = buf[i];
#pragma unroll
    for (int j = 0; j < PL; ++j) rk[j] += kk > key[j] ? 1 : 0;
  }
  // a wave's LDS accesses complete in order: every read above precedes these writes
#pragma unroll
  for (int j = 0; j < PL; ++j)
    if (lane + 64 * j < n && rk[j] < k) buf[rk[j]] = key[j];
  return n < k ? n : k;
}

struct RetrArgs {
  const bf16_t* items;  // [N, 128]
  const bf16_t* qn;     // [Q, 128] queries as the MFMA reads them
  const int* trow;      // [Q] or null
  const float* tscore;  // [Q] (with trow)
  u64* keys;            // [nslab, Q, k]
  int* pcnt;            // [nslab, Q]
  int64_t Q, N, slab_rows;
  int k;
  int shard;  // tscore is the caller's, for every query, whatever trow says (lthm_retrieve_topk_shard)
};

constexpr int RT_XMAX = 1024;  // longest exclusion list of a query
constexpr int RT_GMAX = 8;     // most queries of a group
// retr_topk_k<true> takes the plain arguments and the sorted lists behind them, so that the
// plain instantiation's argument block is the one it always had
struct RetrExclArgs : RetrArgs {
  const int* xs;  // [Q, xstride] ascending; ignored entries and the last one are INT_MAX
  int xstride;    // X + 1
};
// retr_topk_k<EXCL, GP > 1>: Q counts the slots (U GP), trow / tscore / keys / pcnt / xs are
// per user
struct RetrGroupArgs : RetrExclArgs {
  int64_t U;
};
template <bool EXCL, int GP>
using RetrBaseArgs = std::conditional_t<(GP > 1), RetrGroupArgs, std::conditional_t<EXCL, RetrExclArgs, RetrArgs>>;
// retr_topk_k<EXCL, GP, true>: the arguments of <EXCL, GP> and the tags behind them
template <class Base>
struct RetrTagArgs : Base {
  const int* tags;  // [N]
  const int* filt;  // [Q, 3] (GP > 1: [U, 3]): all, any, none
};
template <bool EXCL, int GP, bool TAGS>
using RetrFiltArgs = std::conditional_t<TAGS, RetrTagArgs<RetrBaseArgs<EXCL, GP>>, RetrBaseArgs<EXCL, GP>>;
// retr_topk_k<EXCL, GP, TAGS, true>: the arguments of <EXCL, GP, TAGS> and the cursors behind them
template <class Base>
struct RetrAfterArgs : Base {
  const float* ascore;  // [Q] (GP > 1: [U])
  const int* arow;      // [Q] (GP > 1: [U])
};
template <bool EXCL, int GP, bool TAGS, bool AFTER>
using RetrCursArgs = std::conditional_t<AFTER, RetrAfterArgs<RetrFiltArgs<EXCL, GP, TAGS>>, RetrFiltArgs<EXCL, GP, TAGS>>;
// retr_topk_k<true, GP, TAGS, true, true>: the arguments of <true, GP, TAGS, true> and the prior
// behind them
template <class Base>
struct RetrBiasArgs : Base {
  const float* bias;  // [N]
  const float* bw;    // [Q] (GP > 1: [U]) or null: 1 for everyone
};
template <bool EXCL, int GP, bool TAGS, bool AFTER, bool BIAS = false>
using RetrTopkArgs =
    std::conditional_t<BIAS, RetrBiasArgs<RetrCursArgs<EXCL, GP, TAGS, AFTER>>, RetrCursArgs<EXCL, GP, TAGS, AFTER>>;

// The maximum of x over the GP adjacent lanes of a group, in every lane of it: xor distances 1
// and 2 as DPP quad permutes ([1,0,3,2], [2,3,0,1]); then all four lanes of a quad hold the
// quad's maximum and the half-row mirror (lane i of 8 reads lane 7 - i) brings the other quad's.
// All 64 lanes are active where this runs.
template <int GP>
__device__ __forceinline__ float retr_group_max(float x) {
  if constexpr (GP >= 2)
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, false)));
  if constexpr (GP >= 4)
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, false)));
  if constexpr (GP >= 8)
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xF, 0xF, false)));
  return x;
}

// ---------------------------------------------------------------- exclusion lists, sorted
// One block per query: a bitonic sort of the list, padded to a power of two with INT_MAX, in
// LDS.  Entries outside [0, N) become INT_MAX (no catalogue row: N < 2^31), so they sort behind
// every row and the first X sorted values hold every valid entry.
__global__ __launch_bounds__(256) void retr_excl_prep_k(const int* __restrict__ rows, int X, int P, int64_t N,
                                                        int* __restrict__ xs) {
  __shared__ int buf[RT_XMAX];
  const int tid = threadIdx.x;
  const int* src = rows + (int64_t)blockIdx.x * X;
  for (int i = tid; i < P; i += 256) {
    int r = INT_MAX;
    if (i < X) {
      r = src[i];
      if (r < 0 || r >= N) r = INT_MAX;
    }
    buf[i] = r;
  }
  __syncthreads();
  for (int len = 2; len <= P; len <<= 1) {
    for (int j = len >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += 256) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const int x = buf[lo], y = buf[hi];
        if ((x > y) == ((lo & len) == 0)) {
          buf[lo] = y;
          buf[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  int* dst = xs + (int64_t)blockIdx.x * (X + 1);
  for (int i = tid; i < X; i += 256) dst[i] = buf[i];
  if (tid == 0) dst[X] = INT_MAX;  // the sentinel: a cursor never reads past it
}

// ---------------------------------------------------------------- queries -> bf16, target score
// 16 lanes per query, 8 contiguous elements per lane (rownorm_v8_k's arithmetic for D = 128).
// miss is the target score of a query without a target: -inf in the retrieval calls, NaN in
// lthm_retrieve_target_score.
template <typename TQ>
__global__ __launch_bounds__(256) void retr_prep_k(const TQ* __restrict__ q, int64_t Q, int normalize,
                                                   bf16_t* __restrict__ qn, const bf16_t* __restrict__ items,
                                                   int64_t N, const int* __restrict__ trow,
                                                   float* __restrict__ tscore, float miss) {
  const int sub = threadIdx.x & 15;
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool in = r0 < Q;
  const int64_t r = in ? r0 : Q - 1;  // every lane takes part in the group sums
  float v[8];
  if constexpr (sizeof(TQ) == 2) {
    load_vec<TQ, 16>(q + r * RT_D + 8 * sub, v);
  } else {
    load_vec<TQ, 16>(q + r * RT_D + 8 * sub, v);
    load_vec<TQ, 16>(q + r * RT_D + 8 * sub + 4, v + 4);
  }
  if (normalize) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ss += v[i] * v[i];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float den = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = v[i] / den;
  }
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
  if (in) *reinterpret_cast<u32x4*>(qn + r * RT_D + 8 * sub) = w;
  if (trow) {
    const int tr = trow[r];
    const bool ok = tr >= 0 && tr < N;
    float it[8];
    load_vec<bf16_t, 16>(items + (int64_t)(ok ? tr : 0) * RT_D + 8 * sub, it);
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dot = __builtin_fmaf(__uint_as_float(w[i] << 16), it[2 * i], dot);
      dot = __builtin_fmaf(__uint_as_float(w[i] & 0xffff0000u), it[2 * i + 1], dot);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if (in && sub == 0) tscore[r] = ok ? dot : miss;
  }
}

// The grouped layout: 16 lanes per user walk the user's GP slots; slot g holds query g of
// q [U, G, 128], a slot at or past G the user's query 0.  Every slot goes through retr_prep_k's
// arithmetic, and tscore[u] is the maximum of the slots' target dots.
template <typename TQ>
__global__ __launch_bounds__(256) void retr_prep_group_k(const TQ* __restrict__ q, int64_t U, int G, int GP,
                                                         int normalize, bf16_t* __restrict__ qn,
                                                         const bf16_t* __restrict__ items, int64_t N,
                                                         const int* __restrict__ trow, float* __restrict__ tscore,
                                                         float miss) {
  const int sub = threadIdx.x & 15;
  const int64_t u0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool in = u0 < U;
  const int64_t u = in ? u0 : U - 1;  // every lane takes part in the group sums
  int tr = -1;
  bool ok = false;
  float it[8];
  if (trow) {
    tr = trow[u];
    ok = tr >= 0 && tr < N;
    load_vec<bf16_t, 16>(items + (int64_t)(ok ? tr : 0) * RT_D + 8 * sub, it);
  }
  float best = -INFINITY;
  for (int g = 0; g < GP; ++g) {
    const int64_t r = u * G + (g < G ? g : 0);
    float v[8];
    if constexpr (sizeof(TQ) == 2) {
      load_vec<TQ, 16>(q + r * RT_D + 8 * sub, v);
    } else {
      load_vec<TQ, 16>(q + r * RT_D + 8 * sub, v);
      load_vec<TQ, 16>(q + r * RT_D + 8 * sub + 4, v + 4);
    }
    if (normalize) {
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) ss += v[i] * v[i];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
      const float den = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = v[i] / den;
    }
    u32x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
    if (in) *reinterpret_cast<u32x4*>(qn + (u * GP + g) * RT_D + 8 * sub) = w;
    if (trow) {
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dot = __builtin_fmaf(__uint_as_float(w[i] << 16), it[2 * i], dot);
        dot = __builtin_fmaf(__uint_as_float(w[i] & 0xffff0000u), it[2 * i + 1], dot);
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
      best = fmaxf(best, dot);
    }
  }
  if (trow && in && sub == 0) tscore[u] = ok ? best : miss;
}

// The prior of the target: tscore[q] = fmaf(weight[q], bias[target], tscore[q]) behind either prep
// kernel (with groups q is a user and tscore the best of the plain dots), ahead of the scan, which
// reads it as the score to count against.  No target (-inf, or the NaN of
// lthm_retrieve_target_score) stays what it is; bias is read at rows in [0, N) only.
__global__ __launch_bounds__(256) void retr_bias_target_k(const int* __restrict__ trow, int64_t Q, int64_t N,
                                                          const float* __restrict__ bias, const float* __restrict__ bw,
                                                          float* __restrict__ tscore) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  const int tr = trow[q];
  if (tr < 0 || tr >= N) return;
  tscore[q] = __builtin_fmaf(bw ? bw[q] : 1.f, bias[tr], tscore[q]);
}

// ---------------------------------------------------------------- scores + threshold selection
// Wave w: queries 32 (w & 1) + (lane & 31) of the tile (MFMA columns, so every per-query value
// is a per-lane scalar), image rows 32 (w >> 1) + 8 (v >> 2) + 4 (lane >> 5) + (v & 3).
//
// EXCL: the lane keeps a cursor into its query's sorted exclusion list (xp, with the entry it
// points at in nx).  The cursor starts at the first entry >= row_lo; every tile consumes the
// entries below its end, so at a tile's start nx is at or past the tile's first row and a
// tile without excluded rows costs one compare.  INT_MAX ends every list and is never below a
// tile's end (<= N < 2^31), so the cursor stops on it.
//
// GP > 1: queries are slots, GP per user and never across a wave half.  A group's first lane
// (lead) owns user uq = q / GP: it alone has a threshold, a target, a list cursor and a
// candidate buffer (those of its own slot ql), after every lane of the group took the group's
// maximum of its accumulator.
//
// TAGS: row j passes the lane's filter iff (tag & (all | none)) == all and (any == 0 or
// tag & any != 0); the lane keeps fm = all | none, fw = all, fy = any and yz = (any == 0), so that
// the any term is ((tag & fy) | yz) != 0.  An unsatisfiable filter (all & none != 0) becomes
// fm = 0, fw = 1, which no tag passes.  A lane that is no leader keeps the neutral filter: it is
// inert already.
//
// AFTER: the lane keeps its query's cursor (cs, cr) and row j with score s is eligible iff
// s < cs or (s == cs and j > cr), in f32 (so -0 == +0, and a NaN cs admits nothing).  A tile whose
// lane maximum is below cs costs the maximum and one compare; otherwise every element is tested,
// the row term as "element offset > cr - rb" with cr - rb clamped to [-1, 32], the offsets being
// 0..27.  A lane that is no leader keeps cs = +inf, which every finite score is below.  An
// AFTER instantiation takes a null list (a.xs) as "no exclusion": the cursor call without a list
// runs the excluding instantiation, whose walk then never starts.
//
// BIAS: the lane keeps its query's weight wq (1 without a.bw) and every accumulator element
// becomes fmaf(wq, bias of its row, element) behind the partial-tile mask and the group maximum
// and ahead of the other masks, the count and the filter.  A row past the slab reads the zero word
// and stays at -inf; a lane that is no leader keeps wq = 0.  BIAS exists for <true, GP, TAGS, true>
// only and takes a null cursor (a.ascore) as "no cursor", the way AFTER takes a null list.
template <bool EXCL, int GP = 1, bool TAGS = false, bool AFTER = false, bool BIAS = false>
__global__ __launch_bounds__(256) void retr_topk_k(RetrTopkArgs<EXCL, GP, TAGS, AFTER, BIAS> a) {
  static_assert(!BIAS || (EXCL && AFTER), "the prior rides on the excluding cursor instantiations");
  using RetrSharedFilt = std::conditional_t<TAGS, RetrSharedTags, RetrShared>;
  __shared__ __attribute__((aligned(16))) std::conditional_t<BIAS, RetrSharedBias<RetrSharedFilt>, RetrSharedFilt> sh;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5, ih = w >> 1;
  const int64_t q0 = (int64_t)blockIdx.x * RT_QT;
  const int slab = blockIdx.y;
  const int64_t row_lo = (int64_t)slab * a.slab_rows;
  const int64_t row_hi = row_lo + a.slab_rows < a.N ? row_lo + a.slab_rows : a.N;
  const int ntile = (int)((row_hi - row_lo + RT_IT - 1) / RT_IT);
  const int ql = 32 * (w & 1) + r32;
  const int64_t q = q0 + ql;
  const bool live = q < a.Q;
  bool lead = live;
  int64_t uq = q;
  if constexpr (GP > 1) {
    lead = live && (r32 & (GP - 1)) == 0;
    uq = q / GP;
  }
  int64_t nout = a.Q;  // rows of keys and pcnt per slab
  if constexpr (GP > 1) nout = a.U;

  if (tid < RT_QT) {
    // a query past Q never passes the filter, nor does a slot that is not its group's first
    bool first = q0 + tid < a.Q;
    if constexpr (GP > 1) first = first && (tid & (GP - 1)) == 0;
    sh.tau[tid] = first ? -INFINITY : INFINITY;
    sh.cnt[tid] = 0;
    sh.pc[tid] = 0;
  }
  if (tid < 3) sh.flag[tid] = 0;

  bf16x8v qf[8];
  {
    const bf16_t* rp = a.qn + (live ? q : 0) * RT_D;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (live) v = *reinterpret_cast<const u32x4*>(rp + 16 * s + 8 * hh);
      qf[s] = __builtin_bit_cast(bf16x8v, v);
    }
  }
  int tr = -1;
  float ts = INFINITY;  // no target: nothing counts
  if (lead && (a.trow || a.shard)) {
    if (a.trow) tr = a.trow[uq];
    if (tr < 0 || tr >= a.N) tr = -1;
    // shard: the score to count against is the caller's also where the target lives elsewhere (a
    // NaN, "no target", is above nothing and nothing is above it)
    if (tr >= 0 || a.shard) ts = a.tscore[uq];
  }
  const int* xp = nullptr;
  int nx = INT_MAX;  // a query past Q excludes nothing and reads nothing
  if constexpr (EXCL) {
    if (lead && (!AFTER || a.xs != nullptr)) {
      const int* xl = a.xs + uq * a.xstride;
      int lo = 0, hi = a.xstride - 1;  // xl[hi] = INT_MAX >= row_lo: lower_bound in at most 11 steps
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xl[mid] < row_lo) lo = mid + 1;
        else hi = mid;
      }
      xp = xl + lo;
      nx = *xp;
    }
  }
  int fm = 0, fw = 0, fy = 0;
  int yz = 1;
  if constexpr (TAGS) {
    if (lead) {
      const int* fp = a.filt + uq * 3;
      const int fall = fp[0], fnone = fp[2];
      fy = fp[1];
      yz = fy == 0;
      fm = (fall & fnone) ? 0 : (fall | fnone);
      fw = (fall & fnone) ? 1 : fall;
    }
  }
  float cs = INFINITY;  // a query past Q and a slot that is no leader: no cursor
  int cr = -1;
  if constexpr (AFTER) {
    if (lead && (!BIAS || a.ascore != nullptr)) {
      cs = a.ascore[uq];
      cr = a.arow[uq];
    }
  }
  float wq = 0.f;  // a query past Q and a slot that is no leader: no prior
  if constexpr (BIAS) {
    if (lead) wq = a.bw ? a.bw[uq] : 1.f;
  }
  int roff[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) roff[s] = ih * 8192 + ko32(r32, 2 * s + hh);

  // wave w stages rows 16 w .. 16 w + 15 of an image with four DMAs of 4 rows x 256 B (lane l:
  // row 16 w + 4 j + l / 16, slot l % 16, source chunk slot ^ swz32(row)); rows at or past
  // row_hi come from the zero row
  const int srow = 16 * w + (lane >> 4), sch = (lane & 15) ^ (((lane >> 4) & 3) << 2);
  const unsigned char* ibase = reinterpret_cast<const unsigned char*>(a.items);
  auto stage = [&](int t) {
    unsigned char* img = sh.img[t & 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t row = row_lo + (int64_t)RT_IT * t + srow + 4 * j;
      const void* src = row < row_hi ? (const void*)(ibase + row * 256 + ((sch ^ j) << 4))
                                     : (const void*)(retr_zero_row + 16 * (lane & 15));
      glds16(src, img + (16 * w + 4 * j) * 256);
    }
    if constexpr (TAGS) {
      // wave 0, lane l: the tag of the image's row l; never a read at or past row_hi <= N
      if (w == 0) {
        const int64_t row = row_lo + (int64_t)RT_IT * t + lane;
        glds4(row < row_hi ? a.tags + row : &retr_zero_tag, sh.tag[t & 1]);
      }
    }
    if constexpr (BIAS) {
      // wave 1, lane l: the bias of the image's row l (wave 0 carries the tags); never a read at
      // or past row_hi <= N
      if (w == 1) {
        const int64_t row = row_lo + (int64_t)RT_IT * t + lane;
        glds4(row < row_hi ? a.bias + row : &retr_zero_bias, sh.bias[t & 1]);
      }
    }
  };
  retire_loads();
  stage(0);
  int above = 0;
  for (int i = 0; i < ntile; ++i) {
    wait_vm<0>();
    __syncthreads();  // image i landed; every wave is past tile i - 1 (its image and its appends)
    if (i + 1 < ntile) stage(i + 1);
    if (tid == 0) sh.flag[(i + 1) % 3] = 0;  // last read in tile i - 1, next set in tile i + 1
    if (sh.flag[(i + 2) % 3]) {              // tile i - 1 pushed a query past the limit
      for (int pq = w * GP; pq < RT_QT; pq += 4 * GP) {  // the groups' first slots
        const int n = sh.cnt[pq];
        if (n > RT_LIM) {
          const int m = retr_prune<RT_CAP / 64>(sh.cand[pq], n, a.k, lane);
          if (lane == 0) {
            sh.cnt[pq] = m;
            if (m == a.k) sh.tau[pq] = retr_key_score(sh.cand[pq][a.k - 1]);
          }
        }
      }
      __syncthreads();
    }
    const unsigned char* img = sh.img[i & 1];
    // TAGS: the lane's rows are four runs of four consecutive tag words, the same in all 32
    // lanes of a wave half (broadcast reads): element 4 j + c is image row 32 ih + 4 hh + 8 j + c.
    // Read ahead of the MFMAs, used behind them.
    int4 t4[4];
    if constexpr (TAGS) {
      const int4* tp = reinterpret_cast<const int4*>(sh.tag[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) t4[j] = tp[2 * j];
    }
    // BIAS: the same four runs of the bias words, read the same way
    float4 b4[4];
    if constexpr (BIAS) {
      const float4* bp = reinterpret_cast<const float4*>(sh.bias[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) b4[j] = bp[2 * j];
    }
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8v af = frag_at(img + roff[s]);
      acc = mfma32(af, qf[s], acc);
    }
    // first catalogue row of this lane's elements: element v is row rb + 8 (v >> 2) + (v & 3)
    const int64_t rb = row_lo + (int64_t)RT_IT * i + 32 * ih + 4 * hh;
    if (row_lo + (int64_t)RT_IT * (i + 1) > row_hi) {  // partial tile: the rows past the slab never count or pass
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (rb + 8 * (v >> 2) + (v & 3) >= row_hi) acc[v] = -INFINITY;
    }
    if constexpr (GP > 1) {
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[v] = retr_group_max<GP>(acc[v]);
    }
    if constexpr (BIAS) {
      // the score from here on; a row past the slab is fmaf(wq, 0, -inf) = -inf
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bw4[4] = {b4[j].x, b4[j].y, b4[j].z, b4[j].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[4 * j + c] = __builtin_fmaf(wq, bw4[c], acc[4 * j + c]);
      }
    }
    if constexpr (EXCL) {
      // the tile's excluded rows, folded into a mask of this lane's own elements (the target's
      // mapping below: 0 <= rel < 32 and !(rel & 4) are this lane's rows), then applied with
      // static indices: an excluded row scores -inf for the count and the filter alike
      const int64_t tile_end = row_lo + (int64_t)RT_IT * (i + 1) < row_hi ? row_lo + (int64_t)RT_IT * (i + 1) : row_hi;
      unsigned xm = 0u;
      while (nx < tile_end) {
        const int64_t xrel = (int64_t)nx - rb;
        if (xrel >= 0 && xrel < 32 && !(xrel & 4)) xm |= 1u << (int)(((xrel >> 3) << 2) | (xrel & 3));
        nx = *++xp;
      }
      if (xm) {
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if ((xm >> v) & 1u) acc[v] = -INFINITY;
      }
    }
    if constexpr (TAGS) {
      // two compares and one select per element: an ineligible row scores -inf like an excluded one
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int tw[4] = {t4[j].x, t4[j].y, t4[j].z, t4[j].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool bad = ((tw[c] & fm) != fw) | (((tw[c] & fy) | yz) == 0);
          acc[4 * j + c] = bad ? -INFINITY : acc[4 * j + c];
        }
      }
    }
    if constexpr (AFTER) {
      // rows at or before the cursor score -inf like an excluded row; !(m < cs) also holds for a
      // NaN cs, which then fails both terms of every element
      float m = acc[0];
#pragma unroll
      for (int v = 1; v < 16; ++v) m = fmaxf(m, acc[v]);
      if (!(m < cs)) {
        const int64_t cd = (int64_t)cr - rb;
        const int cq = cd < -1 ? -1 : cd > 32 ? 32 : (int)cd;  // element offsets are 0..27
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const float s = acc[v];
          const bool ok = (s < cs) | ((s == cs) & (8 * (v >> 2) + (v & 3) > cq));
          acc[v] = ok ? s : -INFINITY;
        }
      }
    }
    float mx = acc[0];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      above += acc[v] > ts ? 1 : 0;
      mx = fmaxf(mx, acc[v]);
    }
    const int64_t rel = (int64_t)tr - rb;
    if (tr >= 0 && rel >= 0 && rel < 32 && !(rel & 4)) {  // the target's own row is not counted
      const int vt = (int)(((rel >> 3) << 2) | (rel & 3));
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (v == vt && acc[v] > ts) --above;
    }
    const float tau = sh.tau[ql];
    if (mx >= tau) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float s = acc[v];
        if (s >= tau && s > -INFINITY) {
          const int slot = atomicAdd(&sh.cnt[ql], 1);
          if (slot < RT_CAP) sh.cand[ql][slot] = retr_key(s, (int)(rb + 8 * (v >> 2) + (v & 3)));
          if (slot >= RT_LIM) sh.flag[i % 3] = 1;
        }
      }
    }
  }
  above += __shfl_xor(above, 32, 64);
  if (hh == 0 && live && above) atomicAdd(&sh.pc[ql], above);
  __syncthreads();
  // the slab's k best of every query, sorted; empty slots are key 0
  for (int pq = w * GP; pq < RT_QT; pq += 4 * GP) {
    if (q0 + pq >= a.Q) break;
    const int m = retr_prune<RT_CAP / 64>(sh.cand[pq], sh.cnt[pq], a.k, lane);
    u64* out = a.keys + ((int64_t)slab * nout + (q0 + pq) / GP) * a.k;
    for (int idx = lane; idx < a.k; idx += 64) out[idx] = idx < m ? sh.cand[pq][idx] : 0ull;
  }
  if constexpr (GP == 1) {
    if ((a.trow || a.shard) && tid < RT_QT && q0 + tid < a.Q) a.pcnt[(int64_t)slab * a.Q + q0 + tid] = sh.pc[tid];
  } else {
    if ((a.trow || a.shard) && tid < RT_QT && q0 + tid < a.Q && (tid & (GP - 1)) == 0)
      a.pcnt[(int64_t)slab * nout + (q0 + tid) / GP] = sh.pc[tid];
  }
}

// ---------------------------------------------------------------- merge of the slabs' k-lists
// One wave per query; the lists are sorted and hold their empty slots (key 0) at the end.
__global__ __launch_bounds__(256) void retr_merge_k(const u64* __restrict__ keys, const int* __restrict__ pcnt,
                                                    const int* __restrict__ trow, int64_t Q, int64_t N, int nslab,
                                                    int k, float* __restrict__ scores, int* __restrict__ rows,
                                                    int* __restrict__ rank, const float* __restrict__ tsin) {
  __shared__ u64 sbuf[4][2 * RT_KMAX];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q = (int64_t)blockIdx.x * 4 + w;
  if (q >= Q) return;  // whole waves; no block barrier below
  u64* buf = sbuf[w];
  int n = 0;
  for (int s = 0; s < nslab; ++s) {
    const u64* src = keys + ((int64_t)s * Q + q) * k;
    if (n == k && src[0] < buf[k - 1]) continue;  // nothing in this list reaches the k best
    int v = 0;
    for (int idx = lane; idx < 64 * ((k + 63) / 64); idx += 64) {
      const u64 key = idx < k ? src[idx] : 0ull;
      if (key) buf[n + idx] = key;
      v += __popcll(__ballot(key != 0ull));
    }
    n = retr_prune<2 * RT_KMAX / 64>(buf, n + v, k, lane);
  }
  for (int idx = lane; idx < k; idx += 64) {
    const bool has = idx < n;
    const u64 key = has ? buf[idx] : 0ull;
    scores[q * k + idx] = has ? retr_key_score(key) : -INFINITY;
    rows[q * k + idx] = has ? retr_key_row(key) : -1;
  }
  if (rank) {
    int c = 0;
    for (int s = lane; s < nslab; s += 64) c += pcnt[(int64_t)s * Q + q];  // integers: any order, one sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    // tsin (lthm_retrieve_topk_shard): a query has a target iff its given score is no NaN
    bool has;
    if (tsin) {
      has = !(tsin[q] != tsin[q]);
    } else {
      const int tr = trow[q];
      has = tr >= 0 && tr < N;
    }
    if (lane == 0) rank[q] = has ? c : -1;
  }
}

// ---------------------------------------------------------------- deep lists: 128 < k <= 1024 in one scan
// retr_deep_topk_k is retr_topk_k<true, GP, TAGS, true, true> (the tile loop, the masks and the
// count are its text) with the candidate keys in the workspace instead of LDS: 64 queries of
// RD_CAP keys are 1 MiB.  Each (slab, query or user) owns `stride` key slots in global memory
// (RD_CAP, or max(k, slab_rows) for a slab shorter than RD_CAP, which can never hold more), and
// only the block of that (slab, query tile) ever touches them.  The per-query count, tau and the
// flags stay in LDS.  An append takes its slot from the LDS counter and writes the key with an
// ordinary vector store; the barrier at the top of the next tile (workgroup release / acquire:
// the stores have left the wave, and all waves of a block share one L1) orders it ahead of the
// prune, which one wave runs per flagged query: the n <= RD_CAP keys into the wave's own LDS
// buffer, a bitonic sort (descending, padded with key 0 to a power of two), the first k back to
// the query's slots, tau from key k - 1.  All keys are distinct, so the sorted list, and with it
// the result, does not depend on the order in which slots were handed out.  A null list, a null
// cursor and a null bias are "none": the walk never starts, cs stays +inf, and the bias words
// are neither staged nor applied.
constexpr int RD_KMAX = 1024;            // largest k
constexpr int RD_CAP = 2048;             // candidate slots per (slab, query): a power of two, the sort's size
constexpr int RD_LIM = RD_CAP - RT_IT;   // a query's count at the start of every tile is <= RD_LIM
// The same invariant as above, with 960 free slots behind a full list: a prune leaves at most
// k <= RD_KMAX keys, a tile appends at most RT_IT per query, and a query above RD_LIM is pruned
// before the next tile.
static_assert(RD_KMAX <= RD_LIM, "a pruned buffer must have a whole item tile of free slots");
static_assert(RD_LIM + RT_IT <= RD_CAP, "a tile's appends must fit behind the limit");
static_assert(RD_LIM - RD_KMAX >= RD_KMAX / 2, "a full list must absorb many appends between two sorts");
static_assert((RD_CAP & (RD_CAP - 1)) == 0 && RD_CAP >= 512, "the sort takes a power of two, four pairs per lane");

struct RetrDeepShared {
  unsigned char img[2][RT_IT * 256];
  u64 sort[4][RD_CAP];  // one buffer per wave
  float tau[RT_QT];
  int cnt[RT_QT];
  int pc[RT_QT];
  int flag[3];
  alignas(16) int tag[2][RT_IT];
  alignas(16) float bias[2][RT_IT];
};
static_assert(sizeof(RetrDeepShared) <= 100 * 1024, "LDS budget: the images, four sort buffers and change");

template <int GP, bool TAGS>
struct RetrDeepArgs : RetrTopkArgs<true, GP, TAGS, true, true> {
  int stride;  // key slots per (slab, query or user): keys is [nslab, Q or U, stride]
};

// One wave sorts buf[0, P) descending, P a power of two in 512..RD_CAP: a bitonic network, four
// compare-exchanges per lane and step (all four pairs read, then written).  A wave's LDS
// accesses complete in order, so a step sees the step before it.
__device__ __forceinline__ void retr_deep_sort(u64* buf, int P, int lane) {
  for (int len = 2; len <= P; len <<= 1) {
    for (int j = len >> 1; j > 0; j >>= 1) {
      for (int t0 = lane; t0 < (P >> 1); t0 += 256) {
        int lo[4];
        u64 x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = t0 + 64 * u;  // < P / 2: P / 2 is a multiple of 256
          lo[u] = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          x[u] = buf[lo[u]];
          y[u] = buf[lo[u] | j];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if ((x[u] < y[u]) == ((lo[u] & len) == 0)) {
            buf[lo[u]] = y[u];
            buf[lo[u] | j] = x[u];
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// One wave: the n keys of g[0, n) sorted descending into buf, the first min(n, k) of them back
// to g (with fill: key 0 behind them up to k).  Returns min(n, k).
__device__ __forceinline__ int retr_deep_prune(u64* g, u64* buf, int n, int k, bool fill, int lane) {
  int P = 512;
  while (P < n) P <<= 1;  // n <= stride <= RD_CAP
  for (int idx = lane; idx < P; idx += 64) buf[idx] = idx < n ? g[idx] : 0ull;
  __builtin_amdgcn_wave_barrier();
  if (n > 1) retr_deep_sort(buf, P, lane);
  const int m = n < k ? n : k;
  const int top = fill ? k : m;
  for (int idx = lane; idx < top; idx += 64) g[idx] = idx < m ? buf[idx] : 0ull;
  return m;
}

template <int GP, bool TAGS>
__global__ __launch_bounds__(256) void retr_deep_topk_k(RetrDeepArgs<GP, TAGS> a) {
  __shared__ __attribute__((aligned(16))) RetrDeepShared sh;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5, ih = w >> 1;
  const int64_t q0 = (int64_t)blockIdx.x * RT_QT;
  const int slab = blockIdx.y;
  const int64_t row_lo = (int64_t)slab * a.slab_rows;
  const int64_t row_hi = row_lo + a.slab_rows < a.N ? row_lo + a.slab_rows : a.N;
  const int ntile = (int)((row_hi - row_lo + RT_IT - 1) / RT_IT);
  const int ql = 32 * (w & 1) + r32;
  const int64_t q = q0 + ql;
  const bool live = q < a.Q;
  bool lead = live;
  int64_t uq = q;
  if constexpr (GP > 1) {
    lead = live && (r32 & (GP - 1)) == 0;
    uq = q / GP;
  }
  int64_t nout = a.Q;  // rows of keys and pcnt per slab
  if constexpr (GP > 1) nout = a.U;
  const int stride = a.stride;
  const bool hasb = a.bias != nullptr;  // uniform

  if (tid < RT_QT) {
    bool first = q0 + tid < a.Q;
    if constexpr (GP > 1) first = first && (tid & (GP - 1)) == 0;
    sh.tau[tid] = first ? -INFINITY : INFINITY;
    sh.cnt[tid] = 0;
    sh.pc[tid] = 0;
  }
  if (tid < 3) sh.flag[tid] = 0;

  bf16x8v qf[8];
  {
    const bf16_t* rp = a.qn + (live ? q : 0) * RT_D;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (live) v = *reinterpret_cast<const u32x4*>(rp + 16 * s + 8 * hh);
      qf[s] = __builtin_bit_cast(bf16x8v, v);
    }
  }
  int tr = -1;
  float ts = INFINITY;  // no target: nothing counts
  if (lead && (a.trow || a.shard)) {
    if (a.trow) tr = a.trow[uq];
    if (tr < 0 || tr >= a.N) tr = -1;
    // shard: the score to count against is the caller's also where the target lives elsewhere (a
    // NaN, "no target", is above nothing and nothing is above it)
    if (tr >= 0 || a.shard) ts = a.tscore[uq];
  }
  const int* xp = nullptr;
  int nx = INT_MAX;  // no list, a query past Q: excludes nothing and reads nothing
  if (lead && a.xs != nullptr) {
    const int* xl = a.xs + uq * a.xstride;
    int lo = 0, hi = a.xstride - 1;  // xl[hi] = INT_MAX >= row_lo
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (xl[mid] < row_lo) lo = mid + 1;
      else hi = mid;
    }
    xp = xl + lo;
    nx = *xp;
  }
  int fm = 0, fw = 0, fy = 0;
  int yz = 1;
  if constexpr (TAGS) {
    if (lead) {
      const int* fp = a.filt + uq * 3;
      const int fall = fp[0], fnone = fp[2];
      fy = fp[1];
      yz = fy == 0;
      fm = (fall & fnone) ? 0 : (fall | fnone);
      fw = (fall & fnone) ? 1 : fall;
    }
  }
  float cs = INFINITY;  // no cursor, a query past Q, a slot that is no leader
  int cr = -1;
  if (lead && a.ascore != nullptr) {
    cs = a.ascore[uq];
    cr = a.arow[uq];
  }
  float wq = 0.f;
  if (lead && hasb) wq = a.bw ? a.bw[uq] : 1.f;
  // the leader's key slots; a lane that is no leader never appends (its tau is +inf)
  u64* const kbuf = a.keys + ((int64_t)slab * nout + (lead ? uq : 0)) * stride;
  int roff[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) roff[s] = ih * 8192 + ko32(r32, 2 * s + hh);

  const int srow = 16 * w + (lane >> 4), sch = (lane & 15) ^ (((lane >> 4) & 3) << 2);
  const unsigned char* ibase = reinterpret_cast<const unsigned char*>(a.items);
  auto stage = [&](int t) {
    unsigned char* img = sh.img[t & 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t row = row_lo + (int64_t)RT_IT * t + srow + 4 * j;
      const void* src = row < row_hi ? (const void*)(ibase + row * 256 + ((sch ^ j) << 4))
                                     : (const void*)(retr_zero_row + 16 * (lane & 15));
      glds16(src, img + (16 * w + 4 * j) * 256);
    }
    if constexpr (TAGS) {
      if (w == 0) {
        const int64_t row = row_lo + (int64_t)RT_IT * t + lane;
        glds4(row < row_hi ? a.tags + row : &retr_zero_tag, sh.tag[t & 1]);
      }
    }
    if (hasb && w == 1) {
      const int64_t row = row_lo + (int64_t)RT_IT * t + lane;
      glds4(row < row_hi ? a.bias + row : &retr_zero_bias, sh.bias[t & 1]);
    }
  };
  retire_loads();
  stage(0);
  int above = 0;
  for (int i = 0; i < ntile; ++i) {
    // the key stores of tile i - 1 count in vmcnt like the DMA: this wait retires both
    wait_vm<0>();
    __syncthreads();  // image i landed; every wave is past tile i - 1 (its image and its appends)
    if (i + 1 < ntile) stage(i + 1);
    if (tid == 0) sh.flag[(i + 1) % 3] = 0;
    if (sh.flag[(i + 2) % 3]) {  // tile i - 1 pushed a query past the limit
      for (int pq = w * GP; pq < RT_QT; pq += 4 * GP) {
        int n = sh.cnt[pq];
        if (n > RD_LIM) {
          n = n < stride ? n : stride;
          u64* g = a.keys + ((int64_t)slab * nout + (q0 + pq) / GP) * stride;
          const int m = retr_deep_prune(g, sh.sort[w], n, a.k, false, lane);
          if (lane == 0) {
            sh.cnt[pq] = m;
            if (m == a.k) sh.tau[pq] = retr_key_score(sh.sort[w][a.k - 1]);
          }
        }
      }
      __syncthreads();
    }
    const unsigned char* img = sh.img[i & 1];
    int4 t4[4];
    if constexpr (TAGS) {
      const int4* tp = reinterpret_cast<const int4*>(sh.tag[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) t4[j] = tp[2 * j];
    }
    float4 b4[4] = {};
    if (hasb) {
      const float4* bp = reinterpret_cast<const float4*>(sh.bias[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) b4[j] = bp[2 * j];
    }
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8v af = frag_at(img + roff[s]);
      acc = mfma32(af, qf[s], acc);
    }
    const int64_t rb = row_lo + (int64_t)RT_IT * i + 32 * ih + 4 * hh;
    if (row_lo + (int64_t)RT_IT * (i + 1) > row_hi) {
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (rb + 8 * (v >> 2) + (v & 3) >= row_hi) acc[v] = -INFINITY;
    }
    if constexpr (GP > 1) {
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[v] = retr_group_max<GP>(acc[v]);
    }
    if (hasb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bw4[4] = {b4[j].x, b4[j].y, b4[j].z, b4[j].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[4 * j + c] = __builtin_fmaf(wq, bw4[c], acc[4 * j + c]);
      }
    }
    {
      const int64_t tile_end = row_lo + (int64_t)RT_IT * (i + 1) < row_hi ? row_lo + (int64_t)RT_IT * (i + 1) : row_hi;
      unsigned xm = 0u;
      while (nx < tile_end) {
        const int64_t xrel = (int64_t)nx - rb;
        if (xrel >= 0 && xrel < 32 && !(xrel & 4)) xm |= 1u << (int)(((xrel >> 3) << 2) | (xrel & 3));
        nx = *++xp;
      }
      if (xm) {
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if ((xm >> v) & 1u) acc[v] = -INFINITY;
      }
    }
    if constexpr (TAGS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int tw[4] = {t4[j].x, t4[j].y, t4[j].z, t4[j].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool bad = ((tw[c] & fm) != fw) | (((tw[c] & fy) | yz) == 0);
          acc[4 * j + c] = bad ? -INFINITY : acc[4 * j + c];
        }
      }
    }
    {
      float m = acc[0];
#pragma unroll
      for (int v = 1; v < 16; ++v) m = fmaxf(m, acc[v]);
      if (!(m < cs)) {
        const int64_t cd = (int64_t)cr - rb;
        const int cq = cd < -1 ? -1 : cd > 32 ? 32 : (int)cd;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const float s = acc[v];
          const bool ok = (s < cs) | ((s == cs) & (8 * (v >> 2) + (v & 3) > cq));
          acc[v] = ok ? s : -INFINITY;
        }
      }
    }
    float mx = acc[0];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      above += acc[v] > ts ? 1 : 0;
      mx = fmaxf(mx, acc[v]);
    }
    const int64_t rel = (int64_t)tr - rb;
    if (tr >= 0 && rel >= 0 && rel < 32 && !(rel & 4)) {
      const int vt = (int)(((rel >> 3) << 2) | (rel & 3));
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (v == vt && acc[v] > ts) --above;
    }
    const float tau = sh.tau[ql];
    if (mx >= tau) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float s = acc[v];
        if (s >= tau && s > -INFINITY) {
          const int slot = atomicAdd(&sh.cnt[ql], 1);
          if (lead && slot < stride) kbuf[slot] = retr_key(s, (int)(rb + 8 * (v >> 2) + (v & 3)));
          if (slot >= RD_LIM) sh.flag[i % 3] = 1;
        }
      }
    }
  }
  above += __shfl_xor(above, 32, 64);
  if (hh == 0 && live && above) atomicAdd(&sh.pc[ql], above);
  __syncthreads();  // the last tile's appends have left their waves
  // the slab's k best of every query, sorted, in the first k of its slots; empty slots are key 0
  for (int pq = w * GP; pq < RT_QT; pq += 4 * GP) {
    if (q0 + pq >= a.Q) break;
    int n = sh.cnt[pq];
    n = n < stride ? n : stride;
    u64* g = a.keys + ((int64_t)slab * nout + (q0 + pq) / GP) * stride;
    retr_deep_prune(g, sh.sort[w], n, a.k, true, lane);
  }
  if constexpr (GP == 1) {
    if ((a.trow || a.shard) && tid < RT_QT && q0 + tid < a.Q) a.pcnt[(int64_t)slab * a.Q + q0 + tid] = sh.pc[tid];
  } else {
    if ((a.trow || a.shard) && tid < RT_QT && q0 + tid < a.Q && (tid & (GP - 1)) == 0)
      a.pcnt[(int64_t)slab * nout + (q0 + tid) / GP] = sh.pc[tid];
  }
}

// The merge of the slabs' lists, one wave per query.  A is the best list so far (n keys, sorted,
// in LDS) and B a slab's list (nb keys, sorted, in LDS); all keys are distinct, so the rank of
// a_i in the union is i + #{b > a_i}, found by binary search, and the same for B.  Every lane
// takes its keys and their ranks into registers, then the keys of rank < k are written at their
// rank into A: a wave's LDS accesses complete in order, so every read precedes these writes.
__global__ __launch_bounds__(256) void retr_deep_merge_k(const u64* __restrict__ keys, int stride,
                                                         const int* __restrict__ pcnt, const int* __restrict__ trow,
                                                         int64_t Q, int64_t N, int nslab, int k,
                                                         float* __restrict__ scores, int* __restrict__ rows,
                                                         int* __restrict__ rank, const float* __restrict__ tsin) {
  __shared__ u64 sbuf[4][2][RD_KMAX];
  static_assert(sizeof(sbuf) <= 64 * 1024, "LDS budget");
  constexpr int PL = RD_KMAX / 64;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q = (int64_t)blockIdx.x * 4 + w;
  if (q >= Q) return;  // whole waves; no block barrier below
  u64* A = sbuf[w][0];
  u64* B = sbuf[w][1];
  int n = 0;
  for (int s = 0; s < nslab; ++s) {
    const u64* src = keys + ((int64_t)s * Q + q) * stride;
    if (n == k && src[0] < A[k - 1]) continue;  // nothing in this list reaches the k best
    int nb = 0;
    for (int idx = lane; idx < 64 * ((k + 63) / 64); idx += 64) {
      const u64 key = idx < k ? src[idx] : 0ull;
      if (key) B[idx] = key;  // sorted, the empty slots at the end: the keys are B[0, nb)
      nb += __popcll(__ballot(key != 0ull));
    }
    __builtin_amdgcn_wave_barrier();
    u64 ka[PL] = {}, kb[PL] = {};
    int ra[PL], rb[PL];
#pragma unroll
    for (int j = 0; j < PL; ++j) {
      const int idx = lane + 64 * j;
      ra[j] = rb[j] = k;  // not written
      if (64 * j < n) {   // uniform
        const u64 key = idx < n ? A[idx] : 0ull;
        int lo = 0, hi = nb;  // #{b > key}: B is descending
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (B[mid] > key) lo = mid + 1;
          else hi = mid;
        }
        ka[j] = key;
        if (idx < n) ra[j] = idx + lo;
      }
      if (64 * j < nb) {
        const u64 key = idx < nb ? B[idx] : 0ull;
        int lo = 0, hi = n;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (A[mid] > key) lo = mid + 1;
          else hi = mid;
        }
        kb[j] = key;
        if (idx < nb) rb[j] = idx + lo;
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < PL; ++j) {
      if (ra[j] < k) A[ra[j]] = ka[j];
      if (rb[j] < k) A[rb[j]] = kb[j];
    }
    __builtin_amdgcn_wave_barrier();
    n = n + nb < k ? n + nb : k;
  }
  for (int idx = lane; idx < k; idx += 64) {
    const bool has = idx < n;
    const u64 key = has ? A[idx] : 0ull;
    scores[q * k + idx] = has ? retr_key_score(key) : -INFINITY;
    rows[q * k + idx] = has ? retr_key_row(key) : -1;
  }
  if (rank) {
    int c = 0;
    for (int s = lane; s < nslab; s += 64) c += pcnt[(int64_t)s * Q + q];  // integers: any order, one sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    // tsin (lthm_retrieve_topk_shard): a query has a target iff its given score is no NaN
    bool has;
    if (tsin) {
      has = !(tsin[q] != tsin[q]);
    } else {
      const int tr = trow[q];
      has = tr >= 0 && tr < N;
    }
    if (lane == 0) rank[q] = has ? c : -1;
  }
}

// ---------------------------------------------------------------- the scan's host side
// Every scan entry point is one call of retr_scan: the checks, the plan of the grid and the
// workspace (RetrPlan), then prep, the target's prior, the sorted lists, the scan and the merge.
// The workspace is, in this order and each part rounded up to 256 bytes,
//   qn    [S, 128] bf16     the queries as slots, S = U gp
//   keys  [nslab, U, stride] u64
//   pcnt  [nslab, U] int
//   xs    [U, X + 1] int    only with an exclusion list
// and the four size queries return the plan's total.
constexpr int64_t RETR_MAX_SLABS = 65535;  // grid.y

inline int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

// slots per user: the next power of two of G
inline int retr_gp(int G) {
  int gp = 1;
  while (gp < G) gp <<= 1;
  return gp;
}

// Rows per slab (a multiple of the item tile), or -1 for sizes the kernels do not take.  S counts
// the query slots.  floor is the shortest slab the rule picks by itself: 1024 rows for k <= RT_KMAX,
// 4 RD_KMAX for a deep list (a slab much shorter than k only pads lists); an explicit multiple of
// the item tile is honoured.
int64_t retr_slab_rows(int64_t S, int64_t N, int64_t slab_rows, int64_t floor) {
  if (S < 1 || S >= (1ll << 31) || N < 1 || N >= (1ll << 31)) return -1;
  int64_t sr = slab_rows;
  if (sr == 0) {
    // one block per CU: with few query tiles (serving) the catalogue is cut into enough slabs
    // to fill 256 CUs; with many (evaluation) into few long ones, which prune and merge less
    const int64_t nqt = (S + RT_QT - 1) / RT_QT;
    const int64_t want = nqt >= 256 ? 1 : (256 + nqt - 1) / nqt;
    sr = (N + want - 1) / want;
    if (sr < floor) sr = floor;
    sr = (sr + RT_IT - 1) / RT_IT * RT_IT;
  }
  if (sr < RT_IT || sr % RT_IT != 0) return -1;
  if ((N + sr - 1) / sr > RETR_MAX_SLABS) return -1;
  return sr;
}

// key slots per (slab, query or user) of a deep call: a slab shorter than RD_CAP never holds more
// keys than rows
inline int64_t retr_deep_stride(int64_t sr, int k) { return sr >= RD_CAP ? RD_CAP : (sr > k ? sr : k); }

struct RetrPlan {
  int gp;                             // slots per user
  bool deep;                          // k > RT_KMAX: retr_deep_topk_k and retr_deep_merge_k
  int64_t S, sr, nslab, stride;       // slots, rows per slab, slabs, key slots per (slab, user)
  int64_t qn, keys, pcnt, xs, total;  // byte offsets into the workspace, and its size
};

// the plan of a scan of U users with G queries each (X = 0: no exclusion list); false for sizes
// the kernels do not take
bool retr_plan(int64_t U, int G, int64_t N, int k, int64_t slab_rows, int64_t X, RetrPlan* p) {
  if (G < 1 || G > RT_GMAX || k < 1 || k > RD_KMAX || X < 0 || X > RT_XMAX || slab_rows < 0) return false;
  if (U < 1 || U >= (1ll << 31)) return false;
  p->gp = retr_gp(G);
  p->deep = k > RT_KMAX;
  p->S = U * p->gp;  // the slab rule sees the query tiles of the padded slots
  p->sr = retr_slab_rows(p->S, N, slab_rows, p->deep ? 4 * RD_KMAX : 1024);
  if (p->sr < 0) return false;
  p->nslab = (N + p->sr - 1) / p->sr;
  p->stride = p->deep ? retr_deep_stride(p->sr, k) : k;
  p->qn = 0;
  p->keys = p->qn + up256(p->S * RT_D * 2);
  p->pcnt = p->keys + up256(p->nslab * U * p->stride * 8);
  p->xs = p->pcnt + up256(p->nslab * U * 4);
  p->total = p->xs + (X ? up256(U * (X + 1) * 4) : 0);
  return true;
}

int64_t retr_plan_bytes(int64_t U, int G, int64_t N, int k, int64_t slab_rows, int64_t X) {
  RetrPlan p;
  return retr_plan(U, G, N, k, slab_rows, X, &p) ? p.total : -1;
}

inline bool retr_cursor_ok(const lthm_retrieve_cursor* c) {
  return !c || (c->after_score && c->after_row && ((uintptr_t)c->after_score & 3) == 0 &&
                ((uintptr_t)c->after_row & 3) == 0);
}

// without a shard descriptor a target brings its two outputs; with one the target score is the
// caller's, d->target_score stays unused (NULL) and every query gets a rank
inline bool retr_target_ok(const lthm_retrieve_desc* d, const lthm_retrieve_shard* sd) {
  if (!sd) return !d->target_row || (d->rank && d->target_score);
  return sd->target_score_in && ((uintptr_t)sd->target_score_in & 3) == 0 && !d->target_score && d->rank;
}

inline bool retr_bias_ok(const lthm_retrieve_bias* b) {
  return !b || (b->bias && ((uintptr_t)b->bias & 3) == 0 && ((uintptr_t)b->weight & 3) == 0);
}

// f(std::integral_constant<int, gp>) for gp = 1, 2, 4, 8
template <class F>
void retr_with_gp(int gp, F&& f) {
  if (gp == 1) f(std::integral_constant<int, 1>{});
  else if (gp == 2) f(std::integral_constant<int, 2>{});
  else if (gp == 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

// The argument block of one instantiation: the common arguments sliced to the kernel's own base
// type (a GP = 1 kernel holds no U, a plain one no lists) and the parts it has behind them.  An
// instantiation that takes a cursor or a prior takes a null one as "none".
template <bool EXCL, int GP, bool TAGS, bool AFTER, bool BIAS>
void retr_fill(RetrTopkArgs<EXCL, GP, TAGS, AFTER, BIAS>& r, const RetrGroupArgs& a, const lthm_retrieve_tags* t,
               const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b) {
  static_cast<RetrBaseArgs<EXCL, GP>&>(r) = a;
  if constexpr (TAGS) {
    r.tags = t->tags;
    r.filt = t->filter;
  }
  if constexpr (AFTER) {
    r.ascore = c ? c->after_score : nullptr;
    r.arow = c ? c->after_row : nullptr;
  }
  if constexpr (BIAS) {
    r.bias = b ? b->bias : nullptr;
    r.bw = b ? b->weight : nullptr;
  }
}

template <bool EXCL, int GP, bool TAGS, bool AFTER, bool BIAS>
void retr_launch_topk(dim3 grid, hipStream_t s, const RetrGroupArgs& a, const lthm_retrieve_tags* t,
                      const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b) {
  RetrTopkArgs<EXCL, GP, TAGS, AFTER, BIAS> r;
  retr_fill<EXCL, GP, TAGS, AFTER, BIAS>(r, a, t, c, b);
  hipLaunchKernelGGL((retr_topk_k<EXCL, GP, TAGS, AFTER, BIAS>), grid, dim3(256), 0, s, r);
}

// The scan kernel of a call.  A deep list has one kernel per (GP, TAGS), which takes every other
// part as it comes.  For k <= RT_KMAX the instantiation holds only what the call needs: a prior
// brings the cursor and the lists with it (null where absent), a cursor the lists (a.xs == nullptr
// without one), and the plain call runs retr_topk_k<false>.
template <int GP, bool TAGS>
void retr_launch_scan(const RetrPlan& p, dim3 grid, hipStream_t s, const RetrGroupArgs& a, const lthm_retrieve_tags* t,
                      const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b) {
  if (p.deep) {
    RetrDeepArgs<GP, TAGS> da;
    retr_fill<true, GP, TAGS, true, true>(da, a, t, c, b);
    da.stride = (int)p.stride;
    hipLaunchKernelGGL((retr_deep_topk_k<GP, TAGS>), grid, dim3(256), 0, s, da);
  } else if (b) {
    retr_launch_topk<true, GP, TAGS, true, true>(grid, s, a, t, c, b);
  } else if (c) {
    retr_launch_topk<true, GP, TAGS, true, false>(grid, s, a, t, c, b);
  } else if (a.xs) {
    retr_launch_topk<true, GP, TAGS, false, false>(grid, s, a, t, c, b);
  } else {
    retr_launch_topk<false, GP, TAGS, false, false>(grid, s, a, t, c, b);
  }
}

// Every scan entry point: d->Q queries, or with g users of g->G queries each; x, t, c and b are the
// parts of the call that are present; sd (lthm_retrieve_topk_shard) makes the target scores the
// caller's.  1 <= d->k <= RD_KMAX.
int retr_scan(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x, const lthm_retrieve_group* g,
              const lthm_retrieve_tags* t, const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b,
              const lthm_retrieve_shard* sd, void* stream) {
  LTHM_REQUIRE(d != nullptr);
  LTHM_REQUIRE(d->items && d->q && d->scores && d->rows && d->workspace);
  LTHM_REQUIRE(d->q_dtype == LTHM_F32 || d->q_dtype == LTHM_BF16);
  LTHM_REQUIRE(retr_target_ok(d, sd));
  LTHM_REQUIRE(((uintptr_t)d->items & 15) == 0 && ((uintptr_t)d->q & 15) == 0 && ((uintptr_t)d->workspace & 15) == 0);
  LTHM_REQUIRE(!x || (x->rows && x->X >= 1 && x->X <= RT_XMAX && ((uintptr_t)x->rows & 3) == 0));
  LTHM_REQUIRE(!t || (t->tags && t->filter && ((uintptr_t)t->tags & 3) == 0 && ((uintptr_t)t->filter & 3) == 0));
  LTHM_REQUIRE(retr_cursor_ok(c));
  LTHM_REQUIRE(retr_bias_ok(b));
  const int G = g ? g->G : 1;
  const int64_t U = d->Q, N = d->N;
  RetrPlan p;
  LTHM_REQUIRE(retr_plan(U, G, N, d->k, d->slab_rows, x ? x->X : 0, &p) && d->ws_bytes >= p.total);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)d->workspace;
  bf16_t* qn = (bf16_t*)(ws + p.qn);
  u64* keys = (u64*)(ws + p.keys);
  int* pcnt = (int*)(ws + p.pcnt);
  const bf16_t* items = (const bf16_t*)d->items;
  const int32_t* ptrow = sd ? nullptr : d->target_row;  // shard: the prep kernel computes no target score
  // queries -> slots: the plain kernel for G = 1, the padded slots for G >= 2
  auto prep = [&](auto* q) {
    using TQ = std::remove_const_t<std::remove_pointer_t<decltype(q)>>;
    const dim3 pgrid((unsigned)((U + 15) / 16));
    if (G == 1)
      hipLaunchKernelGGL((retr_prep_k<TQ>), pgrid, dim3(256), 0, s, q, U, d->normalize_q, qn, items, N, ptrow,
                         d->target_score, -INFINITY);
    else
      hipLaunchKernelGGL((retr_prep_group_k<TQ>), pgrid, dim3(256), 0, s, q, U, G, p.gp, d->normalize_q, qn, items, N,
                         ptrow, d->target_score, -INFINITY);
  };
  if (d->q_dtype == LTHM_BF16) prep((const bf16_t*)d->q);
  else prep((const float*)d->q);
  LTHM_CHECK_LAUNCH();
  if (b && ptrow) {  // the target's prior, behind the prep kernel that wrote d->target_score
    hipLaunchKernelGGL(retr_bias_target_k, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, s, ptrow, U, N, b->bias,
                       b->weight, d->target_score);
    LTHM_CHECK_LAUNCH();
  }
  RetrGroupArgs a;
  a.items = items;
  a.qn = qn;
  a.trow = d->target_row;
  a.tscore = sd ? sd->target_score_in : d->target_score;
  a.shard = sd ? 1 : 0;
  a.keys = keys;
  a.pcnt = pcnt;
  a.Q = p.S;
  a.N = N;
  a.slab_rows = p.sr;
  a.k = d->k;
  a.xs = nullptr;
  a.xstride = 0;
  a.U = U;
  if (x) {
    const int X = (int)x->X;
    int P = 1;
    while (P < X) P <<= 1;
    int* xs = (int*)(ws + p.xs);
    hipLaunchKernelGGL(retr_excl_prep_k, dim3((unsigned)U), dim3(256), 0, s, x->rows, X, P, N, xs);  // one list per user
    LTHM_CHECK_LAUNCH();
    a.xs = xs;
    a.xstride = X + 1;
  }
  const dim3 tgrid((unsigned)((p.S + RT_QT - 1) / RT_QT), (unsigned)p.nslab);
  retr_with_gp(p.gp, [&](auto GP) {
    if (t) retr_launch_scan<decltype(GP)::value, true>(p, tgrid, s, a, t, c, b);
    else retr_launch_scan<decltype(GP)::value, false>(p, tgrid, s, a, t, c, b);
  });
  LTHM_CHECK_LAUNCH();
  const dim3 mgrid((unsigned)((U + 3) / 4));
  int32_t* rank = (d->target_row || sd) ? d->rank : nullptr;
  const float* tsin = sd ? sd->target_score_in : nullptr;
  if (p.deep)
    hipLaunchKernelGGL(retr_deep_merge_k, mgrid, dim3(256), 0, s, keys, (int)p.stride, pcnt, d->target_row, U, N,
                       (int)p.nslab, d->k, d->scores, d->rows, rank, tsin);
  else
    hipLaunchKernelGGL(retr_merge_k, mgrid, dim3(256), 0, s, keys, pcnt, d->target_row, U, N, (int)p.nslab, d->k,
                       d->scores, d->rows, rank, tsin);
  LTHM_CHECK_LAUNCH();
  return 0;
}

// the entry points for k <= RT_KMAX refuse a deep list
inline bool retr_shallow(const lthm_retrieve_desc* d) { return d && d->k <= RT_KMAX; }

}  // namespace
}  // namespace lthm

using namespace lthm;

extern "C" int64_t lthm_retrieve_ws_bytes(int64_t Q, int64_t N, int32_t k, int32_t slab_rows) {
  return k > RT_KMAX ? -1 : retr_plan_bytes(Q, 1, N, k, slab_rows, 0);
}

extern "C" int64_t lthm_retrieve_excl_ws_bytes(int64_t Q, int64_t N, int32_t k, int32_t slab_rows, int64_t X) {
  return k > RT_KMAX || X < 1 ? -1 : retr_plan_bytes(Q, 1, N, k, slab_rows, X);
}

extern "C" int64_t lthm_retrieve_group_ws_bytes(int64_t U, int32_t G, int64_t N, int32_t k, int32_t slab_rows,
                                                int64_t X) {
  return k > RT_KMAX ? -1 : retr_plan_bytes(U, G, N, k, slab_rows, X);
}

extern "C" int64_t lthm_retrieve_deep_ws_bytes(int64_t U, int32_t G, int64_t N, int32_t k, int32_t slab_rows,
                                               int64_t X) {
  return retr_plan_bytes(U, G, N, k, slab_rows, X);
}

extern "C" int lthm_retrieve_topk(const lthm_retrieve_desc* d, void* stream) {
  LTHM_REQUIRE(retr_shallow(d));
  return retr_scan(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int lthm_retrieve_topk_excl(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x, void* stream) {
  LTHM_REQUIRE(retr_shallow(d));
  return retr_scan(d, x, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int lthm_retrieve_topk_group(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x,
                                        const lthm_retrieve_group* g, void* stream) {
  LTHM_REQUIRE(retr_shallow(d));
  return retr_scan(d, x, g, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int lthm_retrieve_topk_tags(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x,
                                       const lthm_retrieve_group* g, const lthm_retrieve_tags* t, void* stream) {
  LTHM_REQUIRE(retr_shallow(d));
  return retr_scan(d, x, g, t, nullptr, nullptr, nullptr, stream);
}

extern "C" int lthm_retrieve_topk_after(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x,
                                        const lthm_retrieve_group* g, const lthm_retrieve_tags* t,
                                        const lthm_retrieve_cursor* c, void* stream) {
  LTHM_REQUIRE(retr_shallow(d));
  return retr_scan(d, x, g, t, c, nullptr, nullptr, stream);
}

extern "C" int lthm_retrieve_topk_bias(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x,
                                       const lthm_retrieve_group* g, const lthm_retrieve_tags* t,
                                       const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b, void* stream) {
  LTHM_REQUIRE(retr_shallow(d));
  return retr_scan(d, x, g, t, c, b, nullptr, stream);
}

extern "C" int lthm_retrieve_topk_deep(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x,
                                       const lthm_retrieve_group* g, const lthm_retrieve_tags* t,
                                       const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b, void* stream) {
  return retr_scan(d, x, g, t, c, b, nullptr, stream);
}

// ---------------------------------------------------------------- sharded catalogues
// lthm_retrieve_topk_shard is the scan above with the caller's target scores (RetrArgs::shard);
// lthm_retrieve_target_score is the prep kernels' target dot alone; retr_shard_merge_k merges the
// lists that S shards return for one query.
//
// Merge by rank: a (score, id) pair does not fit the 64-bit key, so an entry is compared as
// (score image, id): a precedes b iff image_a > image_b, or the images are equal and id_a < id_b
// (or the pairs are equal, which the contract rules out, and a's list comes first: so that also
// then the positions below are a permutation and every output slot is written once).  The output
// position of entry i of list s is i plus, for every other list, the number of its entries that
// precede this one: one binary search per list over that list's filled prefix, cut short at the
// k - pos entries that can still matter, and given up once pos reaches k.  No sort, no atomics, no
// slot hand-out: the result is a pure function of the inputs.
//
// A team (one wave of a block for S k <= 1024, else the block) owns one query.  The lists are staged
// in LDS as images and ids (12 bytes per entry) when they fit CAP entries per team, and searched
// in global memory otherwise (CAP = 0).  Every index is below S k and every write below k,
// whatever the lists hold.
namespace lthm {
namespace {

constexpr int RS_SMAX = 64;    // most lists
constexpr uint32_t RS_EMPTY = 0x007fffffu;  // retr_image(-inf): an entry at or below it is an empty slot

template <int TEAM, int CAP>
__global__ __launch_bounds__(256) void retr_shard_merge_k(const float* __restrict__ scores,
                                                          const int64_t* __restrict__ ids,
                                                          const int* __restrict__ ranks, int64_t Q, int S, int k,
                                                          float* __restrict__ out_scores, int64_t* __restrict__ out_ids,
                                                          int64_t* __restrict__ out_rank) {
  constexpr int NT = 256 / TEAM;  // queries of a block
  constexpr bool LDS = CAP > 0;
  __shared__ uint32_t simg[LDS ? NT * CAP : 1];
  __shared__ int64_t sid[LDS ? NT * CAP : 1];
  __shared__ int slen[NT][RS_SMAX];
  static_assert(sizeof(simg) + sizeof(sid) + sizeof(slen) <= 160 * 1024, "LDS budget");
  const int team = threadIdx.x / TEAM, t = threadIdx.x % TEAM;
  const int64_t q0 = (int64_t)blockIdx.x * NT + team;
  const bool live = q0 < Q;
  const int64_t q = live ? q0 : Q - 1;  // a team past Q reads the last query and writes nothing
  const int n = S * k;                  // <= 65536
  uint32_t* const im = simg + (LDS ? team * CAP : 0);
  int64_t* const idl = sid + (LDS ? team * CAP : 0);
  // entry i of list s
  auto src = [&](int s, int i) { return ((int64_t)s * Q + q) * k + i; };
  auto img_at = [&](int s, int i) { return LDS ? im[s * k + i] : retr_image(scores[src(s, i)]); };
  auto id_at = [&](int s, int i) { return LDS ? idl[s * k + i] : ids[src(s, i)]; };
  if constexpr (LDS) {
    for (int e = t; e < n; e += TEAM) {
      const int s = e / k, i = e - s * k;
      im[e] = retr_image(scores[src(s, i)]);
      idl[e] = ids[src(s, i)];
    }
    __syncthreads();
  }
  // the filled prefix of every list: the first empty slot of a descending list
  for (int s = t; s < S; s += TEAM) {
    int lo = 0, hi = k;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (img_at(s, mid) > RS_EMPTY) lo = mid + 1;
      else hi = mid;
    }
    slen[team][s] = lo;
  }
  __syncthreads();
  for (int e = t; e < n; e += TEAM) {
    const int s = e / k, i = e - s * k;
    if (i >= slen[team][s]) continue;
    const uint32_t ei = img_at(s, i);
    const int64_t eid = id_at(s, i);
    int pos = i;
    for (int o = 0; o < S && pos < k; ++o) {
      if (o == s) continue;
      int lo = 0, hi = slen[team][o];
      if (hi > k - pos) hi = k - pos;  // k - pos predecessors already put this entry past the list
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t mi = img_at(o, mid);
        bool before = mi > ei;
        if (mi == ei) {
          const int64_t mid_id = id_at(o, mid);
          before = mid_id < eid || (mid_id == eid && o < s);
        }
        if (before) lo = mid + 1;
        else hi = mid;
      }
      pos += lo;
    }
    if (live && pos < k) {
      out_scores[q * k + pos] = retr_image_score(ei);
      out_ids[q * k + pos] = eid;
    }
  }
  int total = 0;
  for (int s = 0; s < S; ++s) total += slen[team][s];
  for (int p = (total < k ? total : k) + t; p < k; p += TEAM) {
    if (live) {
      out_scores[q * k + p] = -INFINITY;
      out_ids[q * k + p] = 0;
    }
  }
  if (ranks && live && t == 0) {
    int64_t c = 0;
    bool none = false;
    for (int s = 0; s < S; ++s) {
      const int r = ranks[(int64_t)s * Q + q];
      none = none || r == -1;
      c += r;
    }
    out_rank[q] = none ? -1 : c;
  }
}

}  // namespace
}  // namespace lthm

extern "C" int64_t lthm_retrieve_target_score_ws_bytes(int64_t Q, int32_t G) {
  if (Q < 1 || Q >= (1ll << 31) || G < 1 || G > RT_GMAX) return -1;
  return up256(Q * retr_gp(G) * RT_D * 2);
}

extern "C" int lthm_retrieve_target_score(const void* items, int64_t N, const void* q, int32_t q_dtype,
                                          int32_t normalize_q, int32_t G, const int32_t* target_row, const float* bias,
                                          const float* weight, float* out, int64_t Q, void* workspace, int64_t ws_bytes,
                                          void* stream) {
  LTHM_REQUIRE(items && q && target_row && out && workspace);
  LTHM_REQUIRE(N >= 1 && N < (1ll << 31));
  LTHM_REQUIRE(q_dtype == LTHM_F32 || q_dtype == LTHM_BF16);
  LTHM_REQUIRE(((uintptr_t)items & 15) == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
  LTHM_REQUIRE(((uintptr_t)bias & 3) == 0 && ((uintptr_t)weight & 3) == 0 && (bias || !weight));
  const int64_t need = lthm_retrieve_target_score_ws_bytes(Q, G);
  LTHM_REQUIRE(need >= 0 && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  bf16_t* qn = (bf16_t*)workspace;  // the prep kernels' other output, not used here
  const bf16_t* it = (const bf16_t*)items;
  const unsigned pgrid = (unsigned)((Q + 15) / 16);
  const float miss = __builtin_nanf("");
  if (G == 1) {
    if (q_dtype == LTHM_BF16)
      hipLaunchKernelGGL((retr_prep_k<bf16_t>), dim3(pgrid), dim3(256), 0, s, (const bf16_t*)q, Q, normalize_q, qn, it, N,
                         target_row, out, miss);
    else
      hipLaunchKernelGGL((retr_prep_k<float>), dim3(pgrid), dim3(256), 0, s, (const float*)q, Q, normalize_q, qn, it, N,
                         target_row, out, miss);
  } else {
    if (q_dtype == LTHM_BF16)
      hipLaunchKernelGGL((retr_prep_group_k<bf16_t>), dim3(pgrid), dim3(256), 0, s, (const bf16_t*)q, Q, G, retr_gp(G),
                         normalize_q, qn, it, N, target_row, out, miss);
    else
      hipLaunchKernelGGL((retr_prep_group_k<float>), dim3(pgrid), dim3(256), 0, s, (const float*)q, Q, G, retr_gp(G),
                         normalize_q, qn, it, N, target_row, out, miss);
  }
  LTHM_CHECK_LAUNCH();
  if (bias) {
    hipLaunchKernelGGL(retr_bias_target_k, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, target_row, Q, N, bias,
                       weight, out);
    LTHM_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int lthm_retrieve_topk_shard(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x,
                                        const lthm_retrieve_group* g, const lthm_retrieve_tags* t,
                                        const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b,
                                        const lthm_retrieve_shard* s, void* stream) {
  return retr_scan(d, x, g, t, c, b, s, stream);
}

extern "C" int lthm_retrieve_merge_shards(const float* scores, const int64_t* ids, const int32_t* ranks, int32_t S,
                                          int64_t Q, int32_t k, float* out_scores, int64_t* out_ids, int64_t* out_rank,
                                          void* stream) {
  LTHM_REQUIRE(S >= 1 && S <= RS_SMAX && k >= 1 && k <= RD_KMAX && Q >= 1 && Q < (1ll << 31));
  LTHM_REQUIRE(scores && ids && out_scores && out_ids && (!ranks || out_rank));
  LTHM_REQUIRE(((uintptr_t)scores & 3) == 0 && ((uintptr_t)ids & 7) == 0 && ((uintptr_t)ranks & 3) == 0);
  LTHM_REQUIRE(((uintptr_t)out_scores & 3) == 0 && ((uintptr_t)out_ids & 7) == 0 && ((uintptr_t)out_rank & 7) == 0);
  hipStream_t st = (hipStream_t)stream;
  const int n = S * k;
  if (n <= 1024)
    hipLaunchKernelGGL((retr_shard_merge_k<64, 1024>), dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, scores, ids, ranks,
                       Q, S, k, out_scores, out_ids, out_rank);
  else if (n <= 8192)
    hipLaunchKernelGGL((retr_shard_merge_k<256, 8192>), dim3((unsigned)Q), dim3(256), 0, st, scores, ids, ranks, Q, S, k,
                       out_scores, out_ids, out_rank);
  else
    hipLaunchKernelGGL((retr_shard_merge_k<256, 0>), dim3((unsigned)Q), dim3(256), 0, st, scores, ids, ranks, Q, S, k,
                       out_scores, out_ids, out_rank);
  LTHM_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- clustered catalogues (IVF)
// lthm_retrieve_ivf_topk: the catalogue's rows are grouped into L lists (rows [list_off[c],
// list_off[c + 1]), ids ascending inside a list, row_ids[row] the item id) and query q scans only
// the lists its probe row names, probes[q, 0..P).  A (query, probe slot) pair p = q P + s with a
// valid list is one MFMA column of one block:
//   retr_ivf_count_k    cnt[c] = the pairs that probe list c; a pair without a list (an entry
//                       outside [0, L)) gets its empty k-list written here;
//   retr_ivf_offsets_k  one block: the exclusive prefix sums of cnt (pair_off) and of
//                       ceil(cnt / 64) (tile_off); tile_off[L] is the true tile count;
//   retr_ivf_fill_k     the pair indices grouped by list (pair_idx), and for every tile of up to
//                       64 pairs of one list the table entry (list, first pair slot, pairs);
//   retr_ivf_topk_k     block b < tile_off[L] scans the whole list of its tile for the tile's
//                       pairs: retr_topk_k's tile loop (the 64 x 64 score tile, the queries as B
//                       fragments, the LDS-DMA images, the keys and the CAP / LIM invariant)
//                       without a slab cut, a target count or a merge; it writes every pair's
//                       sorted k-list as (score, id) into scores / ids [P, Q, k], the layout
//                       retr_shard_merge_k reads, empty slots as (-inf, 0).
// Nothing comes back to the host in between: the scan's grid is the bound Q P / 64 + min(L, Q P)
// on the tile count and a block past the count exits before it touches LDS or the DMA.  The two
// integer atomics of the plan (cnt, fill) decide only which column of which block serves a pair.
// A column's state (B fragments, threshold, candidates, list cursor) is its own and a prune
// writes each key at its rank, so every pair's list, and with it the merged result, is a pure
// function of the inputs.  A list named twice in one probe row is two pairs with two outputs.
//
// Groups (lthm_retrieve_ivf_topk_group, G >= 2 queries per user): a pair is (user, probe slot), the
// plan cuts a list's pairs into tiles of retr_ivf_tile_pairs(G) instead of 64, and the scan takes the
// maximum over a pair's G columns in registers before anything selects (retr_ivf_topk_k<.., true>), so
// the pairs' lists and the merge see one score per (user, row) and a row takes one slot per user.
namespace lthm {
namespace {

struct RetrIvfShared {
  unsigned char img[2][RT_IT * 256];
  u64 cand[RT_QT][RT_CAP];
  float tau[RT_QT];  // current k-th best score of the pair (-inf until k candidates are held)
  int cnt[RT_QT];    // candidates held
  int pair[RT_QT];   // the pair of every column
  int flag[3];       // flag[i % 3]: tile i pushed some pair past RT_LIM
};
static_assert(sizeof(RetrIvfShared) <= 160 * 1024, "LDS budget");
// retr_ivf_topk_k<true, true, TAGS, BIAS>: the tag and the bias words of the two images' rows behind
// the plain layout, as RetrSharedTags / RetrSharedBias hold them
struct RetrIvfSharedTags : RetrIvfShared {
  alignas(16) int tag[2][RT_IT];  // a lane reads four words at once
};
template <class Base>
struct RetrIvfSharedBias : Base {
  alignas(16) float bias[2][RT_IT];  // a lane reads four words at once
};
static_assert(sizeof(RetrIvfSharedBias<RetrIvfSharedTags>) <= 160 * 1024, "LDS budget");

struct RetrIvfArgs {
  const bf16_t* items;      // [N, 128], list-major
  const bf16_t* qn;         // [Q, 128] queries as the MFMA reads them
  const int64_t* row_ids;   // [N]
  const int64_t* list_off;  // [L + 1]
  const int* tile_off;      // [L + 1]; tile_off[L]: the tiles there are
  const int4* tab;          // per tile: list, first slot in pair_idx, pairs (1..64)
  const int* pair_idx;      // [Q P] pairs grouped by list
  const int* xs;            // EXCL: [Q, xstride] ascending rows; ignored entries and the last one are INT_MAX
  int xstride;              // X + 1
  float* scores;            // [P, Q, k]
  int64_t* ids;             // [P, Q, k]
  int64_t Q, N;
  int L, P, k;
};
// retr_ivf_topk_k<true, true, TAGS, BIAS> takes the plain arguments and the filters behind them, so
// that the plain instantiations' argument block is the one they always had
struct RetrIvfFiltArgs : RetrIvfArgs {
  const int* tags;      // TAGS: [N], clustered numbering
  const int* filt;      // TAGS: [Q, 3]: all, any, none
  const float* bias;    // BIAS: [N], clustered numbering
  const float* bw;      // BIAS: [Q] or null: 1 for everyone
  const float* ascore;  // [Q] or null: no cursor
  const int* crow;      // with ascore: [Q P] the cursor row of every pair (retr_ivf_cursor_k)
};
// retr_ivf_topk_k<true, true, TAGS, BIAS, true> takes the filters' arguments and the group size behind
// them: Q counts the users, qn is [Q G, 128] and everything else is per user
struct RetrIvfGroupArgs : RetrIvfFiltArgs {
  int G;  // queries per user, 2..RT_GMAX
};
template <bool FILT, bool GRP = false>
using RetrIvfScanArgs = std::conditional_t<GRP, RetrIvfGroupArgs, std::conditional_t<FILT, RetrIvfFiltArgs, RetrIvfArgs>>;

// Groups: a pair is (user, probe slot) and takes G adjacent MFMA columns, one per query of the user,
// that never cross a row of 16 lanes, so that the maximum over them is a few DPP row shifts in
// registers.  A row of 16 columns holds 16 / G pairs, a tile 4 (16 / G); the columns behind a row's
// last pair hold no query (whole columns of padding where G does not divide 16).
__host__ __device__ constexpr int retr_ivf_row_pairs(int G) { return 16 / G; }
__host__ __device__ constexpr int retr_ivf_tile_pairs(int G) { return (RT_QT / 16) * retr_ivf_row_pairs(G); }

// x of lane i + N of the same row of 16 lanes, the lane's own x where i + N is past the row
template <int N>
__device__ __forceinline__ float retr_row_shl(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x100 + N, 0xF, 0xF, false));
}
// acc[v] of lane i becomes the maximum over lanes i .. i + G - 1 wherever those lie in the lane's row of
// 16, which is every pair's first lane: windows of 2, 4 and 8 by doubling, then two windows of the
// largest power of two p <= G that overlap, at distance G - p.  G is uniform and all 64 lanes are active.
__device__ __forceinline__ void retr_ivf_group_max(f32x16& acc, int G) {
  if (G >= 2) {
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = fmaxf(acc[v], retr_row_shl<1>(acc[v]));
  }
  if (G >= 4) {
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = fmaxf(acc[v], retr_row_shl<2>(acc[v]));
  }
  if (G >= 8) {
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = fmaxf(acc[v], retr_row_shl<4>(acc[v]));
  }
  const int rest = G - (G >= 8 ? 8 : G >= 4 ? 4 : G >= 2 ? 2 : 1);
  if (rest == 1) {
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = fmaxf(acc[v], retr_row_shl<1>(acc[v]));
  } else if (rest == 2) {
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = fmaxf(acc[v], retr_row_shl<2>(acc[v]));
  } else if (rest == 3) {
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = fmaxf(acc[v], retr_row_shl<3>(acc[v]));
  }
}

__global__ __launch_bounds__(256) void retr_ivf_count_k(const int* __restrict__ probes, int64_t NP, int L, int P,
                                                        int64_t Q, int k, int* __restrict__ cnt,
                                                        float* __restrict__ scores, int64_t* __restrict__ ids) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= NP) return;
  const int c = probes[p];
  if (c >= 0 && c < L) {
    atomicAdd(&cnt[c], 1);
    return;
  }
  const int64_t q = p / P, s = p - q * P;
  const int64_t o = (s * Q + q) * k;
  for (int i = 0; i < k; ++i) {
    scores[o + i] = -INFINITY;
    ids[o + i] = 0;
  }
}

// One block: thread t owns lists [t per, (t + 1) per).  GRP: a tile holds tp pairs (retr_ivf_tile_pairs)
// instead of RT_QT; <false> ignores tp
template <bool GRP>
__global__ __launch_bounds__(256) void retr_ivf_offsets_k(const int* __restrict__ cnt, int L, int* __restrict__ pair_off,
                                                          int* __restrict__ tile_off, int tp) {
  __shared__ int sp[256], st[256];
  const int tq = GRP ? tp : RT_QT;
  const int tid = threadIdx.x;
  const int per = (L + 255) / 256;
  const int64_t lo64 = (int64_t)tid * per;
  const int lo = lo64 < L ? (int)lo64 : L, hi = lo64 + per < L ? (int)(lo64 + per) : L;
  int np = 0, nt = 0;
  for (int c = lo; c < hi; ++c) {
    const int n = cnt[c];
    np += n;
    nt += (n + tq - 1) / tq;
  }
  sp[tid] = np;
  st[tid] = nt;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int x = tid >= o ? sp[tid - o] : 0, y = tid >= o ? st[tid - o] : 0;
    __syncthreads();
    sp[tid] += x;
    st[tid] += y;
    __syncthreads();
  }
  int pa = sp[tid] - np, ta = st[tid] - nt;
  for (int c = lo; c < hi; ++c) {
    const int n = cnt[c];
    pair_off[c] = pa;
    tile_off[c] = ta;
    pa += n;
    ta += (n + tq - 1) / tq;
  }
  if (tid == 255) {
    pair_off[L] = sp[255];
    tile_off[L] = st[255];
  }
}

// pos < cnt[c] (the same pairs were counted), so every index is below Q P and every tile below
// tile_off[L]
template <bool GRP>
__global__ __launch_bounds__(256) void retr_ivf_fill_k(const int* __restrict__ probes, int64_t NP, int L,
                                                       const int* __restrict__ cnt, const int* __restrict__ pair_off,
                                                       const int* __restrict__ tile_off, int* __restrict__ fill,
                                                       int* __restrict__ pair_idx, int4* __restrict__ tab, int tp) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= NP) return;
  const int c = probes[p];
  if (c < 0 || c >= L) return;
  const int pos = atomicAdd(&fill[c], 1);
  const int base = pair_off[c];
  pair_idx[base + pos] = (int)p;
  const int tq = GRP ? tp : RT_QT;  // the pairs of a tile
  if (pos % tq == 0) {
    const int n = cnt[c] - pos;
    tab[tile_off[c] + pos / tq] = make_int4(c, base + pos, n < tq ? n : tq, 0);
  }
}

// The cursor row of every pair p = q P + s with a list c: inside a list ids ascend with rows, so
// "id > after_id" is "row > cr" with cr = row_lo + #{rows of the list with row_ids <= after_id} - 1,
// whether or not the list, or the catalogue, holds after_id (row_lo - 1: every row of the list is
// behind the id; row_hi - 1: none is).  One thread per pair: an upper bound over row_ids[row_lo,
// row_hi) in at most 31 steps, on the scan's own clamped offsets.  A pair without a list gets -1,
// which nothing reads.
__global__ __launch_bounds__(256) void retr_ivf_cursor_k(const int* __restrict__ probes, int64_t NP, int L, int P,
                                                         int64_t N, const int64_t* __restrict__ list_off,
                                                         const int64_t* __restrict__ row_ids,
                                                         const int64_t* __restrict__ after_ids, int* __restrict__ crow) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= NP) return;
  const int c = probes[p];
  if (c < 0 || c >= L) {
    crow[p] = -1;
    return;
  }
  int64_t row_lo = list_off[c], row_hi = list_off[c + 1];
  row_lo = row_lo < 0 ? 0 : row_lo > N ? N : row_lo;
  row_hi = row_hi < row_lo ? row_lo : row_hi > N ? N : row_hi;
  const int64_t aid = after_ids[p / P];
  int64_t lo = row_lo, hi = row_hi;  // the first row of [row_lo, row_hi) whose id is above aid
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (row_ids[mid] <= aid) lo = mid + 1;
    else hi = mid;
  }
  crow[p] = (int)(lo - 1);  // row_lo - 1 >= -1 and row_hi - 1 < N < 2^31
}

// Shards (lthm_retrieve_ivf_topk_shards): S clustered catalogues with tensors of their own are scanned
// as one catalogue whose lists are the shards' lists side by side: shard s owns the lists lbase[s] ..
// lbase[s] + L_s of the plan and the probe slots pbase[s] .. pbase[s] + P_s of every query.  The plan
// kernels see only list numbers, so they run unchanged; a scan block looks its tile's shard up from
// the list number (at most six steps over the descriptors) and reads that shard's tensors.
struct RetrIvfShardDev {
  const bf16_t* items;      // [N, 128], list-major
  const int64_t* row_ids;   // [N]
  const int64_t* list_off;  // [L + 1]
  const int* tags;          // [N] or null
  const float* bias;        // [N] or null
  int64_t N;
  int lbase;                // the shard's first list in the plan's numbering
};
// retr_ivf_topk_k<true, true, TAGS, BIAS, false, true> and retr_ivf_deep_topk_k<TAGS, true>: L counts all
// lists and P all probe slots, xs is [S, Q, xstride] (the excluded rows in every shard's own numbering),
// items, row_ids, list_off, N, tags and bias are unused: the descriptors hold them.
// Targets (rank != null): tsc [Q] is every query's target score (NaN: no shard holds the target), trow
// [S, Q] the target's row in every shard (-1: not there), and rank [P, Q], zeroed by the caller, receives
// per pair the rows of its list that pass every mask, are not the target's and score strictly above tsc:
// integer adds of per-lane counts, so the sums are a pure function of the inputs.
struct RetrIvfShardArgs : RetrIvfFiltArgs {
  u64* keys;                  // deep: [Q P, RD_CAP]
  const RetrIvfShardDev* sh;  // [S], lbase ascending from 0
  const float* tsc;
  const int* trow;
  int* rank;
  int S;
};

// the last shard whose first list is at or below c (0 <= c < L)
__device__ __forceinline__ int retr_ivf_shard_of(const RetrIvfShardDev* sh, int S, int c) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sh[mid].lbase <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// what a scan block reads of its catalogue: the arguments' own tensors, or with SH those of the shard
// that owns list c, which becomes the list's number inside the shard
struct RetrIvfView {
  const bf16_t* items;
  const int64_t* row_ids;
  const int64_t* list_off;
  const int* tags;
  const float* bias;
  const int* xs;
  int64_t N;
  int shard;  // SH: the shard of the tile, else 0
};
template <bool SH, class A>
__device__ __forceinline__ RetrIvfView retr_ivf_view(const A& a, int& c) {
  RetrIvfView cv;
  if constexpr (SH) {
    const int s = retr_ivf_shard_of(a.sh, a.S, c);
    const RetrIvfShardDev d = a.sh[s];
    c -= d.lbase;
    cv.shard = s;
    cv.items = d.items, cv.row_ids = d.row_ids, cv.list_off = d.list_off, cv.tags = d.tags, cv.bias = d.bias, cv.N = d.N;
    cv.xs = a.xs ? a.xs + (int64_t)s * a.Q * a.xstride : nullptr;
  } else {
    cv.items = a.items, cv.row_ids = a.row_ids, cv.list_off = a.list_off, cv.N = a.N, cv.xs = a.xs;
    cv.tags = nullptr, cv.bias = nullptr, cv.shard = 0;
    if constexpr (std::is_base_of_v<RetrIvfFiltArgs, A>) cv.tags = a.tags, cv.bias = a.bias;
  }
  return cv;
}

// retr_ivf_cursor_k over shards: pair p = q P + slot probes list c of the plan, which is list c - lbase
// of the shard that owns it; the bound runs over that shard's row_ids
__global__ __launch_bounds__(256) void retr_ivf_cursor_shards_k(const int* __restrict__ probes, int64_t NP, int L, int P,
                                                                const RetrIvfShardDev* __restrict__ sh, int S,
                                                                const int64_t* __restrict__ after_ids,
                                                                int* __restrict__ crow) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= NP) return;
  const int c = probes[p];
  if (c < 0 || c >= L) {
    crow[p] = -1;
    return;
  }
  const RetrIvfShardDev d = sh[retr_ivf_shard_of(sh, S, c)];
  int64_t row_lo = d.list_off[c - d.lbase], row_hi = d.list_off[c - d.lbase + 1];
  row_lo = row_lo < 0 ? 0 : row_lo > d.N ? d.N : row_lo;
  row_hi = row_hi < row_lo ? row_lo : row_hi > d.N ? d.N : row_hi;
  const int64_t aid = after_ids[p / P];
  int64_t lo = row_lo, hi = row_hi;  // the first row of [row_lo, row_hi) whose id is above aid
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (d.row_ids[mid] <= aid) lo = mid + 1;
    else hi = mid;
  }
  crow[p] = (int)(lo - 1);
}

// the probe slots of shard s, for every query: probes[q, pbase + j] = lbase + rows[q, j], the shard's
// probe row (retr_topk_k over its centroids) in the plan's list numbering; -1 stays -1
__global__ __launch_bounds__(256) void retr_ivf_probe_pack_k(const int* __restrict__ rows, int64_t Q, int Ps, int lbase,
                                                             int pbase, int P, int* __restrict__ probes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Q * Ps) return;
  const int64_t q = i / Ps;
  const int j = (int)(i - q * Ps);
  const int r = rows[i];
  probes[q * P + pbase + j] = r >= 0 ? lbase + r : -1;
}

// Wave w: columns 32 (w & 1) + (lane & 31) of the tile (one pair each, so every per-pair value is a
// per-lane scalar), image rows 32 (w >> 1) + 8 (v >> 2) + 4 (lane >> 5) + (v & 3), as in retr_topk_k.
// EXCL: the lane walks its query's sorted list of excluded rows (the clustered numbering) from the
// first entry >= row_lo; entries of other lists lie outside [row_lo, row_hi) and the walk, which
// stops at the tile's end <= row_hi, never applies them.
//
// FILT (with EXCL): retr_topk_k's tags, prior and cursor with its arithmetic, in its order: the
// partial-tile mask, the prior, exclusion, tags, the cursor, then the threshold and the appends.
// A null list (a.xs) is "no exclusion" and a null cursor (a.ascore) "no cursor", as retr_topk_k's
// AFTER / BIAS instantiations take them.  TAGS: wave 0 stages the 64 tag words of tile i + 1 with
// its image (the zero word for rows at or past row_hi, so never a read at or past row_hi <= N) and a
// lane reads its 16 rows' words back as four broadcast 16-byte LDS reads ahead of the MFMAs.  BIAS:
// wave 1 stages the bias words the same way and every element becomes fmaf(wq, bias of its row,
// element), the score from there on.  The cursor: the pair's score cs and its cursor row cr
// (retr_ivf_cursor_k), then retr_topk_k's AFTER code unchanged.  The filter, the weight and the
// cursor are per lane, like every other per-pair value.  <false> and <true> hold none of this.
//
// GRP (with FILT; lthm_retrieve_ivf_topk_group, G >= 2): a pair is (user, probe slot) and owns G
// adjacent columns of one row of 16 (retr_ivf_row_pairs), column g holding the user's query g; the
// columns behind a row's last pair, and those of a pair the tile does not have, hold zeros.  Behind the
// partial-tile mask every pair's first lane (the leader) takes the maximum of its G columns
// (retr_ivf_group_max), as retr_topk_k<EXCL, GP> does ahead of the prior and the masks; the leader
// alone has a list cursor, a filter, a weight, a cursor, a threshold and a candidate buffer (its own
// column's), so everything from the prior on sees one score per (user, row) and a row takes one slot
// however many of the user's queries it matches.  Every other lane keeps tau = +inf and never appends.
template <bool EXCL, bool FILT = false, bool TAGS = false, bool BIAS = false, bool GRP = false, bool SH = false>
__global__ __launch_bounds__(256) void retr_ivf_topk_k(std::conditional_t<SH, RetrIvfShardArgs, RetrIvfScanArgs<FILT, GRP>> a) {
  static_assert(FILT ? EXCL : !(TAGS || BIAS), "tags, prior and cursor ride on the excluding instantiation");
  static_assert(!GRP || FILT, "groups ride on the filtering instantiations");
  static_assert(!SH || (FILT && !GRP), "shards ride on the filtering instantiations, one query per pair");
  const int blk = blockIdx.x;
  if (blk >= a.tile_off[a.L]) return;  // past the tiles there are: before LDS and the DMA
  using RetrIvfSharedFilt = std::conditional_t<TAGS, RetrIvfSharedTags, RetrIvfShared>;
  __shared__ __attribute__((aligned(16))) std::conditional_t<BIAS, RetrIvfSharedBias<RetrIvfSharedFilt>, RetrIvfSharedFilt> sh;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5, ih = w >> 1;
  const int4 tt = a.tab[blk];
  const int pbase = tt.y, np = tt.z;
  int c = tt.x;
  const RetrIvfView cv = retr_ivf_view<SH>(a, c);  // SH: the tile's shard, c its list there
  // the caller's offsets, kept inside the catalogue whatever they hold
  int64_t row_lo = cv.list_off[c], row_hi = cv.list_off[c + 1];
  row_lo = row_lo < 0 ? 0 : row_lo > cv.N ? cv.N : row_lo;
  row_hi = row_hi < row_lo ? row_lo : row_hi > cv.N ? cv.N : row_hi;
  const int ntile = (int)((row_hi - row_lo + RT_IT - 1) / RT_IT);
  const int ql = 32 * (w & 1) + r32;
  // column ql serves the tile's pair pl (live), as its query gq; lead: the pair's first column
  int pl = ql, gq = 0, G = 1, upr = 16;
  bool live = ql < np;
  if constexpr (GRP) {
    G = a.G;
    upr = retr_ivf_row_pairs(G);
    const int j = (ql & 15) / G;
    gq = (ql & 15) - j * G;
    pl = (ql >> 4) * upr + j;
    live = j < upr && pl < np;
  }
  const bool lead = GRP ? (live && gq == 0) : live;
  const int64_t q = live ? a.pair_idx[pbase + pl] / a.P : 0;
  // SH with targets: the lane counts the rows of its elements that stand above the query's target
  float tsq = NAN;
  int trq = -1, nabove = 0;
  if constexpr (SH) {
    if (a.rank != nullptr && lead) {
      tsq = a.tsc[q];
      trq = a.trow[(int64_t)cv.shard * a.Q + q];
    }
  }

  if (tid < RT_QT) {
    // a column without a pair never passes the filter, nor does one that is not its pair's first
    if constexpr (GRP) {
      const int j = (tid & 15) / G, pt = (tid >> 4) * upr + j;
      const bool first = j < upr && pt < np && (tid & 15) == j * G;
      sh.tau[tid] = first ? -INFINITY : INFINITY;
      sh.cnt[tid] = 0;
      sh.pair[tid] = first ? a.pair_idx[pbase + pt] : 0;
    } else {
      sh.tau[tid] = tid < np ? -INFINITY : INFINITY;
      sh.cnt[tid] = 0;
      sh.pair[tid] = tid < np ? a.pair_idx[pbase + tid] : 0;
    }
  }
  if (tid < 3) sh.flag[tid] = 0;

  bf16x8v qf[8];
  {
    const bf16_t* rp = a.qn + (GRP ? q * G + gq : q) * RT_D;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (live) v = *reinterpret_cast<const u32x4*>(rp + 16 * s + 8 * hh);
      qf[s] = __builtin_bit_cast(bf16x8v, v);
    }
  }
  const int* xp = nullptr;
  int nx = INT_MAX;  // a column without a pair excludes nothing and reads nothing
  if constexpr (EXCL) {
    if (lead && (!FILT || cv.xs != nullptr)) {
      const int* xl = cv.xs + q * a.xstride;
      int lo = 0, hi = a.xstride - 1;  // xl[hi] = INT_MAX >= row_lo: lower_bound in at most 11 steps
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xl[mid] < row_lo) lo = mid + 1;
        else hi = mid;
      }
      xp = xl + lo;
      nx = *xp;
    }
  }
  int fm = 0, fw = 0, fy = 0;
  int yz = 1;
  if constexpr (TAGS) {
    if (lead) {
      const int* fp = a.filt + q * 3;
      const int fall = fp[0], fnone = fp[2];
      fy = fp[1];
      yz = fy == 0;
      fm = (fall & fnone) ? 0 : (fall | fnone);
      fw = (fall & fnone) ? 1 : fall;
    }
  }
  float cs = INFINITY;  // a column without a pair: no cursor
  int cr = -1;
  float wq = 0.f;  // a column without a pair: no prior
  if constexpr (FILT) {
    if (lead && a.ascore != nullptr) {
      cs = a.ascore[q];
      cr = a.crow[a.pair_idx[pbase + pl]];
    }
    if constexpr (BIAS) {
      if (lead) wq = a.bw ? a.bw[q] : 1.f;
    }
  }
  int roff[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) roff[s] = ih * 8192 + ko32(r32, 2 * s + hh);

  // retr_topk_k's staging: wave w brings rows 16 w .. 16 w + 15 of an image with four DMAs of
  // 4 rows x 256 B; rows at or past row_hi come from the zero row
  const int srow = 16 * w + (lane >> 4), sch = (lane & 15) ^ (((lane >> 4) & 3) << 2);
  const unsigned char* ibase = reinterpret_cast<const unsigned char*>(cv.items);
  auto stage = [&](int t) {
    unsigned char* img = sh.img[t & 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t row = row_lo + (int64_t)RT_IT * t + srow + 4 * j;
      const void* src = row < row_hi ? (const void*)(ibase + row * 256 + ((sch ^ j) << 4))
                                     : (const void*)(retr_zero_row + 16 * (lane & 15));
      glds16(src, img + (16 * w + 4 * j) * 256);
    }
    if constexpr (TAGS) {
      // wave 0, lane l: the tag of the image's row l; never a read at or past row_hi <= N
      if (w == 0) {
        const int64_t row = row_lo + (int64_t)RT_IT * t + lane;
        glds4(row < row_hi ? cv.tags + row : &retr_zero_tag, sh.tag[t & 1]);
      }
    }
    if constexpr (BIAS) {
      // wave 1, lane l: the bias of the image's row l; never a read at or past row_hi <= N
      if (w == 1) {
        const int64_t row = row_lo + (int64_t)RT_IT * t + lane;
        glds4(row < row_hi ? cv.bias + row : &retr_zero_bias, sh.bias[t & 1]);
      }
    }
  };
  retire_loads();
  if (ntile > 0) stage(0);
  for (int i = 0; i < ntile; ++i) {
    wait_vm<0>();
    __syncthreads();  // image i landed; every wave is past tile i - 1 (its image and its appends)
    if (i + 1 < ntile) stage(i + 1);
    if (tid == 0) sh.flag[(i + 1) % 3] = 0;  // last read in tile i - 1, next set in tile i + 1
    if (sh.flag[(i + 2) % 3]) {              // tile i - 1 pushed a pair past the limit
      for (int pq = w; pq < RT_QT; pq += 4) {
        const int n = sh.cnt[pq];
        if (n > RT_LIM) {
          const int m = retr_prune<RT_CAP / 64>(sh.cand[pq], n, a.k, lane);
          if (lane == 0) {
            sh.cnt[pq] = m;
            if (m == a.k) sh.tau[pq] = retr_key_score(sh.cand[pq][a.k - 1]);
          }
        }
      }
      __syncthreads();
    }
    const unsigned char* img = sh.img[i & 1];
    // TAGS / BIAS: element 4 j + c is image row 32 ih + 4 hh + 8 j + c, so the lane's words are four
    // runs of four, the same in all 32 lanes of a wave half (broadcast reads); read ahead of the
    // MFMAs, used behind them
    int4 t4[4];
    if constexpr (TAGS) {
      const int4* tp = reinterpret_cast<const int4*>(sh.tag[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) t4[j] = tp[2 * j];
    }
    float4 b4[4];
    if constexpr (BIAS) {
      const float4* bp = reinterpret_cast<const float4*>(sh.bias[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) b4[j] = bp[2 * j];
    }
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8v af = frag_at(img + roff[s]);
      acc = mfma32(af, qf[s], acc);
    }
    // first catalogue row of this lane's elements: element v is row rb + 8 (v >> 2) + (v & 3)
    const int64_t rb = row_lo + (int64_t)RT_IT * i + 32 * ih + 4 * hh;
    if (row_lo + (int64_t)RT_IT * (i + 1) > row_hi) {  // partial tile: the rows past the list never pass
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (rb + 8 * (v >> 2) + (v & 3) >= row_hi) acc[v] = -INFINITY;
    }
    if constexpr (GRP) retr_ivf_group_max(acc, G);  // the leader's elements: the user's best over its queries
    if constexpr (BIAS) {
      // the score from here on; a row past the list is fmaf(wq, 0, -inf) = -inf
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bw4[4] = {b4[j].x, b4[j].y, b4[j].z, b4[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * j + e] = __builtin_fmaf(wq, bw4[e], acc[4 * j + e]);
      }
    }
    if constexpr (EXCL) {
      const int64_t tile_end = row_lo + (int64_t)RT_IT * (i + 1) < row_hi ? row_lo + (int64_t)RT_IT * (i + 1) : row_hi;
      unsigned xm = 0u;
      while (nx < tile_end) {
        const int64_t xrel = (int64_t)nx - rb;
        if (xrel >= 0 && xrel < 32 && !(xrel & 4)) xm |= 1u << (int)(((xrel >> 3) << 2) | (xrel & 3));
        nx = *++xp;
      }
      if (xm) {
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if ((xm >> v) & 1u) acc[v] = -INFINITY;
      }
    }
    if constexpr (TAGS) {
      // two compares and one select per element: an ineligible row scores -inf like an excluded one
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int tw[4] = {t4[j].x, t4[j].y, t4[j].z, t4[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool bad = ((tw[e] & fm) != fw) | (((tw[e] & fy) | yz) == 0);
          acc[4 * j + e] = bad ? -INFINITY : acc[4 * j + e];
        }
      }
    }
    if constexpr (FILT) {
      // rows at or before the cursor score -inf like an excluded row; !(m < cs) also holds for a
      // NaN cs, which then fails both terms of every element.  Without a cursor cs = +inf
      float m = acc[0];
#pragma unroll
      for (int v = 1; v < 16; ++v) m = fmaxf(m, acc[v]);
      if (!(m < cs)) {
        const int64_t cd = (int64_t)cr - rb;
        const int cq = cd < -1 ? -1 : cd > 32 ? 32 : (int)cd;  // element offsets are 0..27
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const float s = acc[v];
          const bool ok = (s < cs) | ((s == cs) & (8 * (v >> 2) + (v & 3) > cq));
          acc[v] = ok ? s : -INFINITY;
        }
      }
    }
    if constexpr (SH) {
      if (a.rank != nullptr) {  // uniform; a NaN target score counts nothing, a masked row is -inf
#pragma unroll
        for (int v = 0; v < 16; ++v)
          nabove += (acc[v] > tsq) & (rb + 8 * (v >> 2) + (v & 3) != (int64_t)trq);
      }
    }
    float mx = acc[0];
#pragma unroll
    for (int v = 1; v < 16; ++v) mx = fmaxf(mx, acc[v]);
    const float tau = sh.tau[ql];
    if ((!GRP || lead) && mx >= tau) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float s = acc[v];
        if (s >= tau && s > -INFINITY) {
          const int slot = atomicAdd(&sh.cnt[ql], 1);
          if (slot < RT_CAP) sh.cand[ql][slot] = retr_key(s, (int)(rb + 8 * (v >> 2) + (v & 3)));
          if (slot >= RT_LIM) sh.flag[i % 3] = 1;
        }
      }
    }
  }
  if constexpr (SH) {
    if (a.rank != nullptr && lead && nabove) {
      const int pr = a.pair_idx[pbase + pl];
      atomicAdd(&a.rank[(int64_t)(pr - q * a.P) * a.Q + q], nabove);
    }
  }
  __syncthreads();
  // every pair's k best of the list, sorted, as (score, id); empty slots are (-inf, 0)
  for (int pi = w; pi < np; pi += 4) {
    const int pq = GRP ? 16 * (pi / upr) + G * (pi % upr) : pi;  // the pair's (first) column
    const int m = retr_prune<RT_CAP / 64>(sh.cand[pq], sh.cnt[pq], a.k, lane);
    const int pr = sh.pair[pq];
    const int64_t pq_q = pr / a.P, pq_s = pr - pq_q * a.P;
    const int64_t o = (pq_s * a.Q + pq_q) * a.k;
    for (int idx = lane; idx < a.k; idx += 64) {
      const bool has = idx < m;
      const u64 key = has ? sh.cand[pq][idx] : 0ull;
      a.scores[o + idx] = has ? retr_key_score(key) : -INFINITY;
      a.ids[o + idx] = has ? cv.row_ids[retr_key_row(key)] : 0;
    }
  }
}

// ---------------------------------------------------------------- clustered deep lists: 128 < k <= 1024
// retr_ivf_deep_topk_k is retr_ivf_topk_k<true, true, TAGS, BIAS>'s work unit (the block, its list, its
// up to 64 pairs, the tile loop and the masks are its text) with retr_deep_topk_k's selection: pair p
// owns the RD_CAP key slots keys[p RD_CAP ..] of the workspace, and only the block that serves the pair
// ever touches them.  Count, tau and the flags stay in LDS.  An append takes its slot from the LDS
// counter and writes the key with an ordinary vector store guarded by slot < RD_CAP; the wait and the
// barrier at the top of the next tile order it ahead of the prune, as retr_deep_topk_k documents.  One
// wave per flagged pair sorts the pair's keys in its own LDS buffer and writes the first k back.  The
// stride is RD_CAP whatever list_off holds: a pair whose count is at most RD_LIM at the top of a tile
// gains at most RT_IT keys in it, so no append passes the guard unwritten and none is lost.  A list
// of at most RD_CAP rows never sets the flag before its last tile has run (slot >= RD_LIM needs more
// than RD_LIM appends) and where it does the flag is not read again: its one sort is the final one,
// which also writes the pair's k-list as (score, id), straight from the sorted LDS buffer, into the
// layout retr_shard_merge_k reads.  A null list, a null cursor and a null bias are "none", as in
// retr_deep_topk_k.
struct RetrIvfDeepShared {
  unsigned char img[2][RT_IT * 256];
  u64 sort[4][RD_CAP];  // one buffer per wave
  float tau[RT_QT];
  int cnt[RT_QT];
  int pair[RT_QT];
  int flag[3];
  alignas(16) int tag[2][RT_IT];
  alignas(16) float bias[2][RT_IT];
};
static_assert(sizeof(RetrIvfDeepShared) <= 100 * 1024, "LDS budget: the images, four sort buffers and change");
static_assert(sizeof(RetrIvfDeepShared) <= 160 * 1024, "LDS budget: one block per CU at the least");

struct RetrIvfDeepArgs : RetrIvfFiltArgs {
  u64* keys;  // [Q P, RD_CAP]: the candidates of every pair
};

template <bool TAGS, bool SH = false>
__global__ __launch_bounds__(256) void retr_ivf_deep_topk_k(std::conditional_t<SH, RetrIvfShardArgs, RetrIvfDeepArgs> a) {
  const int blk = blockIdx.x;
  if (blk >= a.tile_off[a.L]) return;  // past the tiles there are: before LDS and the DMA
  __shared__ __attribute__((aligned(16))) RetrIvfDeepShared sh;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5, ih = w >> 1;
  const int4 tt = a.tab[blk];
  const int pbase = tt.y, np = tt.z;
  int c = tt.x;
  const RetrIvfView cv = retr_ivf_view<SH>(a, c);  // SH: the tile's shard, c its list there
  // the caller's offsets, kept inside the catalogue whatever they hold
  int64_t row_lo = cv.list_off[c], row_hi = cv.list_off[c + 1];
  row_lo = row_lo < 0 ? 0 : row_lo > cv.N ? cv.N : row_lo;
  row_hi = row_hi < row_lo ? row_lo : row_hi > cv.N ? cv.N : row_hi;
  const int ntile = (int)((row_hi - row_lo + RT_IT - 1) / RT_IT);
  const int ql = 32 * (w & 1) + r32;
  const bool live = ql < np;
  const int pr = live ? a.pair_idx[pbase + ql] : 0;  // < Q P
  const int64_t q = pr / a.P;
  const bool hasb = cv.bias != nullptr;  // uniform
  // SH with targets: the lane counts the rows of its elements that stand above the query's target
  float tsq = NAN;
  int trq = -1, nabove = 0;
  if constexpr (SH) {
    if (a.rank != nullptr && live) {
      tsq = a.tsc[q];
      trq = a.trow[(int64_t)cv.shard * a.Q + q];
    }
  }

  if (tid < RT_QT) {
    // a column without a pair never passes the filter
    sh.tau[tid] = tid < np ? -INFINITY : INFINITY;
    sh.cnt[tid] = 0;
    sh.pair[tid] = tid < np ? a.pair_idx[pbase + tid] : 0;
  }
  if (tid < 3) sh.flag[tid] = 0;

  bf16x8v qf[8];
  {
    const bf16_t* rp = a.qn + q * RT_D;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (live) v = *reinterpret_cast<const u32x4*>(rp + 16 * s + 8 * hh);
      qf[s] = __builtin_bit_cast(bf16x8v, v);
    }
  }
  const int* xp = nullptr;
  int nx = INT_MAX;  // no list, a column without a pair: excludes nothing and reads nothing
  if (live && cv.xs != nullptr) {
    const int* xl = cv.xs + q * a.xstride;
    int lo = 0, hi = a.xstride - 1;  // xl[hi] = INT_MAX >= row_lo
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (xl[mid] < row_lo) lo = mid + 1;
      else hi = mid;
    }
    xp = xl + lo;
    nx = *xp;
  }
  int fm = 0, fw = 0, fy = 0;
  int yz = 1;
  if constexpr (TAGS) {
    if (live) {
      const int* fp = a.filt + q * 3;
      const int fall = fp[0], fnone = fp[2];
      fy = fp[1];
      yz = fy == 0;
      fm = (fall & fnone) ? 0 : (fall | fnone);
      fw = (fall & fnone) ? 1 : fall;
    }
  }
  float cs = INFINITY;  // no cursor, a column without a pair
  int cr = -1;
  if (live && a.ascore != nullptr) {
    cs = a.ascore[q];
    cr = a.crow[pr];
  }
  float wq = 0.f;
  if (live && hasb) wq = a.bw ? a.bw[q] : 1.f;
  // the pair's key slots; a column without a pair never appends (its tau is +inf)
  u64* const kbuf = a.keys + (int64_t)pr * RD_CAP;
  int roff[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) roff[s] = ih * 8192 + ko32(r32, 2 * s + hh);

  const int srow = 16 * w + (lane >> 4), sch = (lane & 15) ^ (((lane >> 4) & 3) << 2);
  const unsigned char* ibase = reinterpret_cast<const unsigned char*>(cv.items);
  auto stage = [&](int t) {
    unsigned char* img = sh.img[t & 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t row = row_lo + (int64_t)RT_IT * t + srow + 4 * j;
      const void* src = row < row_hi ? (const void*)(ibase + row * 256 + ((sch ^ j) << 4))
                                     : (const void*)(retr_zero_row + 16 * (lane & 15));
      glds16(src, img + (16 * w + 4 * j) * 256);
    }
    if constexpr (TAGS) {
      if (w == 0) {  // never a read at or past row_hi <= N
        const int64_t row = row_lo + (int64_t)RT_IT * t + lane;
        glds4(row < row_hi ? cv.tags + row : &retr_zero_tag, sh.tag[t & 1]);
      }
    }
    if (hasb && w == 1) {
      const int64_t row = row_lo + (int64_t)RT_IT * t + lane;
      glds4(row < row_hi ? cv.bias + row : &retr_zero_bias, sh.bias[t & 1]);
    }
  };
  retire_loads();
  if (ntile > 0) stage(0);
  for (int i = 0; i < ntile; ++i) {
    // the key stores of tile i - 1 count in vmcnt like the DMA: this wait retires both
    wait_vm<0>();
    __syncthreads();  // image i landed; every wave is past tile i - 1 (its image and its appends)
    if (i + 1 < ntile) stage(i + 1);
    if (tid == 0) sh.flag[(i + 1) % 3] = 0;
    if (sh.flag[(i + 2) % 3]) {  // tile i - 1 pushed a pair past the limit
      for (int pq = w; pq < np; pq += 4) {
        int n = sh.cnt[pq];
        if (n > RD_LIM) {
          n = n < RD_CAP ? n : RD_CAP;
          u64* g = a.keys + (int64_t)sh.pair[pq] * RD_CAP;
          const int m = retr_deep_prune(g, sh.sort[w], n, a.k, false, lane);
          if (lane == 0) {
            sh.cnt[pq] = m;
            if (m == a.k) sh.tau[pq] = retr_key_score(sh.sort[w][a.k - 1]);
          }
        }
      }
      __syncthreads();
    }
    const unsigned char* img = sh.img[i & 1];
    int4 t4[4];
    if constexpr (TAGS) {
      const int4* tp = reinterpret_cast<const int4*>(sh.tag[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) t4[j] = tp[2 * j];
    }
    float4 b4[4] = {};
    if (hasb) {
      const float4* bp = reinterpret_cast<const float4*>(sh.bias[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) b4[j] = bp[2 * j];
    }
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8v af = frag_at(img + roff[s]);
      acc = mfma32(af, qf[s], acc);
    }
    // first catalogue row of this lane's elements: element v is row rb + 8 (v >> 2) + (v & 3)
    const int64_t rb = row_lo + (int64_t)RT_IT * i + 32 * ih + 4 * hh;
    if (row_lo + (int64_t)RT_IT * (i + 1) > row_hi) {  // partial tile: the rows past the list never pass
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (rb + 8 * (v >> 2) + (v & 3) >= row_hi) acc[v] = -INFINITY;
    }
    if (hasb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bw4[4] = {b4[j].x, b4[j].y, b4[j].z, b4[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * j + e] = __builtin_fmaf(wq, bw4[e], acc[4 * j + e]);
      }
    }
    {
      const int64_t tile_end = row_lo + (int64_t)RT_IT * (i + 1) < row_hi ? row_lo + (int64_t)RT_IT * (i + 1) : row_hi;
      unsigned xm = 0u;
      while (nx < tile_end) {
        const int64_t xrel = (int64_t)nx - rb;
        if (xrel >= 0 && xrel < 32 && !(xrel & 4)) xm |= 1u << (int)(((xrel >> 3) << 2) | (xrel & 3));
        nx = *++xp;
      }
      if (xm) {
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if ((xm >> v) & 1u) acc[v] = -INFINITY;
      }
    }
    if constexpr (TAGS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int tw[4] = {t4[j].x, t4[j].y, t4[j].z, t4[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool bad = ((tw[e] & fm) != fw) | (((tw[e] & fy) | yz) == 0);
          acc[4 * j + e] = bad ? -INFINITY : acc[4 * j + e];
        }
      }
    }
    {
      float m = acc[0];
#pragma unroll
      for (int v = 1; v < 16; ++v) m = fmaxf(m, acc[v]);
      if (!(m < cs)) {
        const int64_t cd = (int64_t)cr - rb;
        const int cq = cd < -1 ? -1 : cd > 32 ? 32 : (int)cd;  // element offsets are 0..27
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const float s = acc[v];
          const bool ok = (s < cs) | ((s == cs) & (8 * (v >> 2) + (v & 3) > cq));
          acc[v] = ok ? s : -INFINITY;
        }
      }
    }
    if constexpr (SH) {
      if (a.rank != nullptr) {  // uniform; a NaN target score counts nothing, a masked row is -inf
#pragma unroll
        for (int v = 0; v < 16; ++v)
          nabove += (acc[v] > tsq) & (rb + 8 * (v >> 2) + (v & 3) != (int64_t)trq);
      }
    }
    float mx = acc[0];
#pragma unroll
    for (int v = 1; v < 16; ++v) mx = fmaxf(mx, acc[v]);
    const float tau = sh.tau[ql];
    if (mx >= tau) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float s = acc[v];
        if (s >= tau && s > -INFINITY) {
          const int slot = atomicAdd(&sh.cnt[ql], 1);
          if (live && slot < RD_CAP) kbuf[slot] = retr_key(s, (int)(rb + 8 * (v >> 2) + (v & 3)));
          if (slot >= RD_LIM) sh.flag[i % 3] = 1;
        }
      }
    }
  }
  if constexpr (SH) {
    if (a.rank != nullptr && live && nabove) atomicAdd(&a.rank[(int64_t)(pr - q * a.P) * a.Q + q], nabove);
  }
  wait_vm<0>();
  __syncthreads();  // the last tile's appends have left their waves
  // every pair's k best of the list, sorted, as (score, id); empty slots are (-inf, 0)
  for (int pq = w; pq < np; pq += 4) {
    int n = sh.cnt[pq];
    n = n < RD_CAP ? n : RD_CAP;
    const int pp = sh.pair[pq];
    u64* buf = sh.sort[w];
    int PS = 512;
    while (PS < n) PS <<= 1;  // n <= RD_CAP
    const u64* g = a.keys + (int64_t)pp * RD_CAP;
    for (int idx = lane; idx < PS; idx += 64) buf[idx] = idx < n ? g[idx] : 0ull;
    __builtin_amdgcn_wave_barrier();
    if (n > 1) retr_deep_sort(buf, PS, lane);
    const int m = n < a.k ? n : a.k;
    const int64_t pq_q = pp / a.P, pq_s = pp - pq_q * a.P;
    const int64_t o = (pq_s * a.Q + pq_q) * a.k;
    for (int idx = lane; idx < a.k; idx += 64) {
      const bool has = idx < m;
      const u64 key = has ? buf[idx] : 0ull;  // idx < m <= PS
      a.scores[o + idx] = has ? retr_key_score(key) : -INFINITY;
      a.ids[o + idx] = has ? cv.row_ids[retr_key_row(key)] : 0;
    }
    __builtin_amdgcn_wave_barrier();  // the buffer is read before the wave's next pair refills it
  }
}

// the workspace of one call, in bytes from its start
struct RetrIvfWs {
  int64_t qn, cnt, off, pidx, tab, xs, scores, ids, crow, keys, total, grid;
};

// the scan's grid: sum_c ceil(n_c / 64) <= floor(sum_c n_c / 64) + #{c : n_c > 0} with sum_c n_c <= Q P;
// with groups a tile holds tq = retr_ivf_tile_pairs(G) pairs instead of 64 (the same bound with tq)
inline int64_t retr_ivf_grid(int64_t Q, int64_t P, int64_t L, int64_t tq = RT_QT) {
  const int64_t np = Q * P;
  return np / tq + (L < np ? L : np);
}

// cursor: the pairs' cursor rows behind everything else, so that the call without one has the
// layout and the size it always had
// deep: k up to RD_KMAX and the pairs' key slots behind everything else, for retr_ivf_deep_topk_k
// G > 1 (lthm_retrieve_ivf_topk_group, never deep): Q users of G queries; the queries and the tile
// table grow, everything else is per user.  G = 1 is the layout it always was
bool retr_ivf_ws(int64_t Q, int64_t N, int64_t L, int64_t P, int64_t k, int64_t X, RetrIvfWs* o, bool cursor = false,
                 bool deep = false, int64_t G = 1) {
  if (Q < 1 || Q >= (1ll << 31) || N < 1 || N >= (1ll << 31) || L < 1 || L >= (1ll << 31)) return false;
  if (P < 1 || P > RS_SMAX || k < 1 || k > (deep ? RD_KMAX : RT_KMAX) || X < 0 || X > RT_XMAX) return false;
  if (G < 1 || G > RT_GMAX || (deep && G > 1)) return false;
  if (Q * P >= (1ll << 31) || Q * G >= (1ll << 31)) return false;
  o->grid = retr_ivf_grid(Q, P, L, retr_ivf_tile_pairs((int)G));
  if (o->grid >= (1ll << 31)) return false;
  int64_t at = 0;
  o->qn = at, at += up256(Q * G * RT_D * 2);
  o->cnt = at, at += up256(2 * L * 4);        // cnt, fill
  o->off = at, at += up256(2 * (L + 1) * 4);  // pair_off, tile_off
  o->pidx = at, at += up256(Q * P * 4);
  o->tab = at, at += up256(o->grid * 16);
  o->xs = at, at += X ? up256(Q * (X + 1) * 4) : 0;
  o->scores = at, at += up256(P * Q * k * 4);
  o->ids = at, at += up256(P * Q * k * 8);
  o->crow = at, at += cursor ? up256(Q * P * 4) : 0;
  o->keys = at, at += deep ? up256(Q * P * RD_CAP * 8) : 0;
  o->total = at;
  return true;
}

}  // namespace
}  // namespace lthm

extern "C" int64_t lthm_retrieve_ivf_grid(int64_t Q, int32_t P, int64_t L) {
  if (Q < 1 || P < 1 || L < 1 || Q >= (1ll << 31) || L >= (1ll << 31)) return -1;
  return retr_ivf_grid(Q, P, L);
}

extern "C" int64_t lthm_retrieve_ivf_ws_bytes(int64_t Q, int64_t N, int64_t L, int32_t P, int32_t k, int64_t X) {
  RetrIvfWs w;
  return retr_ivf_ws(Q, N, L, P, k, X, &w) ? w.total : -1;
}

extern "C" int64_t lthm_retrieve_ivf_filt_ws_bytes(int64_t Q, int64_t N, int64_t L, int32_t P, int32_t k, int64_t X,
                                                   int32_t has_cursor) {
  RetrIvfWs w;
  return retr_ivf_ws(Q, N, L, P, k, X, &w, has_cursor != 0) ? w.total : -1;
}

extern "C" int64_t lthm_retrieve_ivf_group_grid(int64_t U, int32_t G, int32_t P, int64_t L) {
  if (U < 1 || P < 1 || L < 1 || U >= (1ll << 31) || L >= (1ll << 31) || G < 1 || G > RT_GMAX) return -1;
  return retr_ivf_grid(U, P, L, retr_ivf_tile_pairs(G));
}

extern "C" int64_t lthm_retrieve_ivf_group_ws_bytes(int64_t U, int32_t G, int64_t N, int64_t L, int32_t P, int32_t k,
                                                    int64_t X, int32_t has_cursor) {
  RetrIvfWs w;
  return retr_ivf_ws(U, N, L, P, k, X, &w, has_cursor != 0, false, G) ? w.total : -1;
}

extern "C" int lthm_retrieve_ivf_topk(const void* items, int64_t N, const int64_t* row_ids, const int64_t* list_off,
                                      int64_t L, const void* q, int32_t q_dtype, int32_t normalize_q, int64_t Q,
                                      const int32_t* probes, int32_t P, int32_t k, const lthm_retrieve_excl* x,
                                      float* out_scores, int64_t* out_ids, void* workspace, int64_t ws_bytes,
                                      void* stream) {
  return lthm_retrieve_ivf_topk_filt(items, N, row_ids, list_off, L, q, q_dtype, normalize_q, Q, probes, P, k, x, nullptr,
                                     nullptr, nullptr, out_scores, out_ids, workspace, ws_bytes, stream);
}

namespace lthm {
namespace {

// The one call path of the clustered scan: without t, b and c it launches retr_ivf_topk_k<false> /
// <true>, as lthm_retrieve_ivf_topk always did; with any of them <true, true, TAGS, BIAS>, which takes
// a null list and a null cursor as "none".  deep (lthm_retrieve_ivf_topk_deep with k > 128): the same
// steps with retr_ivf_deep_topk_k<TAGS> as the scan and the pairs' key slots in the workspace.  G > 1
// (lthm_retrieve_ivf_topk_group): Q users of G queries, the plan with retr_ivf_tile_pairs(G) pairs per
// tile and retr_ivf_topk_k<true, true, TAGS, BIAS, true> as the scan; G = 1 is the call it always was.
int retr_ivf_call(const void* items, int64_t N, const int64_t* row_ids, const int64_t* list_off, int64_t L,
                  const void* q, int32_t q_dtype, int32_t normalize_q, int64_t Q, const int32_t* probes, int32_t P,
                  int32_t k, const lthm_retrieve_excl* x, const lthm_retrieve_tags* t, const lthm_retrieve_bias* b,
                  const lthm_retrieve_ivf_cursor* c, float* out_scores, int64_t* out_ids, void* workspace,
                  int64_t ws_bytes, void* stream, bool deep, int G = 1) {
  LTHM_REQUIRE(items && row_ids && list_off && q && probes && out_scores && out_ids && workspace);
  LTHM_REQUIRE(G >= 1 && G <= RT_GMAX && !(deep && G > 1));
  LTHM_REQUIRE(!t || (t->tags && t->filter && ((uintptr_t)t->tags & 3) == 0 && ((uintptr_t)t->filter & 3) == 0));
  LTHM_REQUIRE(!b || (b->bias && ((uintptr_t)b->bias & 3) == 0 && ((uintptr_t)b->weight & 3) == 0));
  LTHM_REQUIRE(!c || (c->after_score && c->after_id && ((uintptr_t)c->after_score & 3) == 0 &&
                      ((uintptr_t)c->after_id & 7) == 0));
  LTHM_REQUIRE(q_dtype == LTHM_F32 || q_dtype == LTHM_BF16);
  LTHM_REQUIRE(((uintptr_t)items & 15) == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
  LTHM_REQUIRE(((uintptr_t)row_ids & 7) == 0 && ((uintptr_t)list_off & 7) == 0 && ((uintptr_t)probes & 3) == 0);
  LTHM_REQUIRE(((uintptr_t)out_scores & 3) == 0 && ((uintptr_t)out_ids & 7) == 0);
  LTHM_REQUIRE(!x || (x->rows && x->X >= 1 && x->X <= RT_XMAX && ((uintptr_t)x->rows & 3) == 0));
  RetrIvfWs wo;
  LTHM_REQUIRE(retr_ivf_ws(Q, N, L, P, k, x ? x->X : 0, &wo, c != nullptr, deep, G) && ws_bytes >= wo.total);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  bf16_t* qn = (bf16_t*)(ws + wo.qn);
  int* cnt = (int*)(ws + wo.cnt);
  int* fill = cnt + L;
  int* pair_off = (int*)(ws + wo.off);
  int* tile_off = pair_off + (L + 1);
  int* pair_idx = (int*)(ws + wo.pidx);
  int4* tab = (int4*)(ws + wo.tab);
  float* lscores = (float*)(ws + wo.scores);
  int64_t* lids = (int64_t*)(ws + wo.ids);
  const bf16_t* it = (const bf16_t*)items;
  const int64_t NP = Q * P;
  // 1: the queries, by the arithmetic of every other entry (with groups q [Q, G, 128] is Q G rows)
  const int64_t QG = Q * G;
  const unsigned pgrid = (unsigned)((QG + 15) / 16);
  if (q_dtype == LTHM_BF16)
    hipLaunchKernelGGL((retr_prep_k<bf16_t>), dim3(pgrid), dim3(256), 0, s, (const bf16_t*)q, QG, normalize_q, qn, it, N,
                       (const int*)nullptr, (float*)nullptr, -INFINITY);
  else
    hipLaunchKernelGGL((retr_prep_k<float>), dim3(pgrid), dim3(256), 0, s, (const float*)q, QG, normalize_q, qn, it, N,
                       (const int*)nullptr, (float*)nullptr, -INFINITY);
  LTHM_CHECK_LAUNCH();
  // 2: the plan
  {
    const hipError_t e = hipMemsetAsync(cnt, 0, (size_t)(2 * L) * 4, s);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned ngrid = (unsigned)((NP + 255) / 256);
  hipLaunchKernelGGL(retr_ivf_count_k, dim3(ngrid), dim3(256), 0, s, probes, NP, (int)L, (int)P, Q, (int)k, cnt, lscores,
                     lids);
  LTHM_CHECK_LAUNCH();
  const int tp = retr_ivf_tile_pairs(G);
  if (G > 1) hipLaunchKernelGGL(retr_ivf_offsets_k<true>, dim3(1), dim3(256), 0, s, cnt, (int)L, pair_off, tile_off, tp);
  else hipLaunchKernelGGL(retr_ivf_offsets_k<false>, dim3(1), dim3(256), 0, s, cnt, (int)L, pair_off, tile_off, tp);
  LTHM_CHECK_LAUNCH();
  if (G > 1)
    hipLaunchKernelGGL(retr_ivf_fill_k<true>, dim3(ngrid), dim3(256), 0, s, probes, NP, (int)L, cnt, pair_off, tile_off,
                       fill, pair_idx, tab, tp);
  else
    hipLaunchKernelGGL(retr_ivf_fill_k<false>, dim3(ngrid), dim3(256), 0, s, probes, NP, (int)L, cnt, pair_off, tile_off,
                       fill, pair_idx, tab, tp);
  LTHM_CHECK_LAUNCH();
  // 3: the scan (with a cursor, the pairs' cursor rows first: one more kernel of the plan's shape)
  const bool filt = t || b || c;
  RetrIvfDeepArgs a;  // the other instantiations take its bases
  a.keys = deep ? (u64*)(ws + wo.keys) : nullptr;
  a.tags = t ? t->tags : nullptr;
  a.filt = t ? t->filter : nullptr;
  a.bias = b ? b->bias : nullptr;
  a.bw = b ? b->weight : nullptr;
  a.ascore = nullptr;
  a.crow = nullptr;
  if (c) {
    int* crow = (int*)(ws + wo.crow);
    hipLaunchKernelGGL(retr_ivf_cursor_k, dim3(ngrid), dim3(256), 0, s, probes, NP, (int)L, (int)P, N, list_off, row_ids,
                       c->after_id, crow);
    LTHM_CHECK_LAUNCH();
    a.ascore = c->after_score;
    a.crow = crow;
  }
  a.items = it;
  a.qn = qn;
  a.row_ids = row_ids;
  a.list_off = list_off;
  a.tile_off = tile_off;
  a.tab = tab;
  a.pair_idx = pair_idx;
  a.xs = nullptr;
  a.xstride = 0;
  a.scores = lscores;
  a.ids = lids;
  a.Q = Q;
  a.N = N;
  a.L = (int)L;
  a.P = P;
  a.k = k;
  if (x) {
    int* xs = (int*)(ws + wo.xs);
    const int X = (int)x->X;
    int XP = 1;
    while (XP < X) XP <<= 1;
    hipLaunchKernelGGL(retr_excl_prep_k, dim3((unsigned)Q), dim3(256), 0, s, x->rows, X, XP, N, xs);
    LTHM_CHECK_LAUNCH();
    a.xs = xs;
    a.xstride = X + 1;
  }
  const dim3 grid((unsigned)wo.grid);
  if (G > 1) {
    RetrIvfGroupArgs ga;
    static_cast<RetrIvfFiltArgs&>(ga) = a;
    ga.G = G;
    if (t && b) hipLaunchKernelGGL((retr_ivf_topk_k<true, true, true, true, true>), grid, dim3(256), 0, s, ga);
    else if (t) hipLaunchKernelGGL((retr_ivf_topk_k<true, true, true, false, true>), grid, dim3(256), 0, s, ga);
    else if (b) hipLaunchKernelGGL((retr_ivf_topk_k<true, true, false, true, true>), grid, dim3(256), 0, s, ga);
    else hipLaunchKernelGGL((retr_ivf_topk_k<true, true, false, false, true>), grid, dim3(256), 0, s, ga);
  } else if (deep) {
    if (t) hipLaunchKernelGGL(retr_ivf_deep_topk_k<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(retr_ivf_deep_topk_k<false>, grid, dim3(256), 0, s, a);
  } else if (!filt) {
    const RetrIvfArgs& pa = a;
    if (x) hipLaunchKernelGGL(retr_ivf_topk_k<true>, grid, dim3(256), 0, s, pa);
    else hipLaunchKernelGGL(retr_ivf_topk_k<false>, grid, dim3(256), 0, s, pa);
  } else if (t && b) {
    const RetrIvfFiltArgs& fa = a;
    hipLaunchKernelGGL((retr_ivf_topk_k<true, true, true, true>), grid, dim3(256), 0, s, fa);
  } else if (t) {
    const RetrIvfFiltArgs& fa = a;
    hipLaunchKernelGGL((retr_ivf_topk_k<true, true, true, false>), grid, dim3(256), 0, s, fa);
  } else if (b) {
    const RetrIvfFiltArgs& fa = a;
    hipLaunchKernelGGL((retr_ivf_topk_k<true, true, false, true>), grid, dim3(256), 0, s, fa);
  } else {
    const RetrIvfFiltArgs& fa = a;
    hipLaunchKernelGGL((retr_ivf_topk_k<true, true, false, false>), grid, dim3(256), 0, s, fa);
  }
  LTHM_CHECK_LAUNCH();
  // 4: the merge of every query's P lists
  return lthm_retrieve_merge_shards(lscores, lids, nullptr, P, Q, k, out_scores, out_ids, nullptr, stream);
}

}  // namespace
}  // namespace lthm

extern "C" int lthm_retrieve_ivf_topk_filt(const void* items, int64_t N, const int64_t* row_ids,
                                           const int64_t* list_off, int64_t L, const void* q, int32_t q_dtype,
                                           int32_t normalize_q, int64_t Q, const int32_t* probes, int32_t P, int32_t k,
                                           const lthm_retrieve_excl* x, const lthm_retrieve_tags* t,
                                           const lthm_retrieve_bias* b, const lthm_retrieve_ivf_cursor* c,
                                           float* out_scores, int64_t* out_ids, void* workspace, int64_t ws_bytes,
                                           void* stream) {
  return retr_ivf_call(items, N, row_ids, list_off, L, q, q_dtype, normalize_q, Q, probes, P, k, x, t, b, c, out_scores,
                       out_ids, workspace, ws_bytes, stream, false);
}

// g == NULL or g->G == 1 is lthm_retrieve_ivf_topk_filt: the same kernels, the same workspace and the same bits
extern "C" int lthm_retrieve_ivf_topk_group(const void* items, int64_t N, const int64_t* row_ids,
                                            const int64_t* list_off, int64_t L, const void* q, int32_t q_dtype,
                                            int32_t normalize_q, int64_t U, const lthm_retrieve_group* g,
                                            const int32_t* probes, int32_t P, int32_t k, const lthm_retrieve_excl* x,
                                            const lthm_retrieve_tags* t, const lthm_retrieve_bias* b,
                                            const lthm_retrieve_ivf_cursor* c, float* out_scores, int64_t* out_ids,
                                            void* workspace, int64_t ws_bytes, void* stream) {
  return retr_ivf_call(items, N, row_ids, list_off, L, q, q_dtype, normalize_q, U, probes, P, k, x, t, b, c, out_scores,
                       out_ids, workspace, ws_bytes, stream, false, g ? g->G : 1);
}

// k <= 128 is lthm_retrieve_ivf_topk_filt: the same kernels, the same workspace and the same bits
extern "C" int64_t lthm_retrieve_ivf_deep_ws_bytes(int64_t Q, int64_t N, int64_t L, int32_t P, int32_t k, int64_t X,
                                                   int32_t has_cursor) {
  RetrIvfWs w;
  return retr_ivf_ws(Q, N, L, P, k, X, &w, has_cursor != 0, k > RT_KMAX) ? w.total : -1;
}

extern "C" int lthm_retrieve_ivf_topk_deep(const void* items, int64_t N, const int64_t* row_ids,
                                           const int64_t* list_off, int64_t L, const void* q, int32_t q_dtype,
                                           int32_t normalize_q, int64_t Q, const int32_t* probes, int32_t P, int32_t k,
                                           const lthm_retrieve_excl* x, const lthm_retrieve_tags* t,
                                           const lthm_retrieve_bias* b, const lthm_retrieve_ivf_cursor* c,
                                           float* out_scores, int64_t* out_ids, void* workspace, int64_t ws_bytes,
                                           void* stream) {
  return retr_ivf_call(items, N, row_ids, list_off, L, q, q_dtype, normalize_q, Q, probes, P, k, x, t, b, c, out_scores,
                       out_ids, workspace, ws_bytes, stream, k > RT_KMAX);
}

// ---------------------------------------------------------------- sharded clustered catalogues
// lthm_retrieve_ivf_topk_shards: S clustered catalogues of one device, each with centroids and lists of
// its own, answer one batch of queries in one call.
//   1  per shard: its probe row, retr_scan over the shard's centroids with k = P_s = min(nprobe, L_s)
//      (the kernels, and so the bits and the ties, of the single catalogue's probe), packed into the
//      probe slots [pbase_s, pbase_s + P_s) of probes [Q, P], P = sum_s P_s, as list numbers lbase_s + c;
//   2  once: retr_ivf_call's plan over the L = sum_s L_s lists (count, offsets, fill: unchanged kernels),
//      the excluded rows of every shard sorted (one retr_excl_prep_k launch for all), the cursor rows;
//   3  once: the scan, retr_ivf_topk_k<true, true, TAGS, BIAS, false, true> or retr_ivf_deep_topk_k<TAGS,
//      true>: the block-to-(shard, list) map is the plan's tile table and the descriptors' lbase, both on
//      the device; every pair's list lands in [P, Q, k] as (score, id);
//   4  once: lthm_retrieve_merge_shards over the P lists of every query, which also sums the pairs' counts
//      of rows above the target into the query's rank where targets are given.
// The descriptors reach the device as kernel arguments of retr_ivf_desc_k (32 per launch), which stores
// them into the workspace with ordinary vector stores: the call stays stream-ordered end to end.
namespace lthm {
namespace {

constexpr int RI_PACK = 32;  // descriptors per retr_ivf_desc_k launch: 2 KiB of kernel arguments
struct RetrIvfShardPack {
  RetrIvfShardDev d[RI_PACK];
};
__global__ __launch_bounds__(64) void retr_ivf_desc_k(RetrIvfShardPack pk, int n, RetrIvfShardDev* __restrict__ dst) {
  const int t = threadIdx.x;
  if (t < n) dst[t] = pk.d[t];
}

struct RetrIvfShardsWs {
  int64_t desc, probes, prow, pscore, pws, pws_bytes, xs, rank, ivf, total;
  int64_t L, P, Nmax;
  int Pmax;
  RetrIvfWs w;
};

// nprobe <= 0 is refused; P_s = min(nprobe, L_s)
bool retr_ivf_shards_ws(const lthm_retrieve_ivf_shard* sh, int S, int64_t Q, int nprobe, int k, int64_t X, bool cursor,
                        RetrIvfShardsWs* o) {
  if (!sh || S < 1 || S > RS_SMAX || nprobe < 1 || Q < 1 || Q >= (1ll << 31) || X < 0 || X > RT_XMAX) return false;
  int64_t L = 0, P = 0, Nmax = 0, pws = 0;
  int Pmax = 0;
  for (int s = 0; s < S; ++s) {
    if (sh[s].N < 1 || sh[s].N >= (1ll << 31) || sh[s].L < 1 || sh[s].L >= (1ll << 31)) return false;
    const int Ps = (int)(sh[s].L < nprobe ? sh[s].L : nprobe);
    const int64_t b = retr_plan_bytes(Q, 1, sh[s].L, Ps, 0, 0);
    if (b < 0) return false;
    pws = b > pws ? b : pws;
    L += sh[s].L, P += Ps;
    Nmax = sh[s].N > Nmax ? sh[s].N : Nmax;
    Pmax = Ps > Pmax ? Ps : Pmax;
  }
  if (L >= (1ll << 31) || P > RS_SMAX) return false;
  if (!retr_ivf_ws(Q, Nmax, L, P, k, 0, &o->w, cursor, k > RT_KMAX)) return false;
  o->L = L, o->P = P, o->Nmax = Nmax, o->Pmax = Pmax, o->pws_bytes = pws;
  int64_t at = 0;
  o->desc = at, at += up256((int64_t)S * (int64_t)sizeof(RetrIvfShardDev));
  o->probes = at, at += up256(Q * P * 4);
  o->prow = at, at += up256(Q * Pmax * 4);
  o->pscore = at, at += up256(Q * Pmax * 4);
  o->pws = at, at += up256(pws);
  o->xs = at, at += X ? up256((int64_t)S * Q * (X + 1) * 4) : 0;
  o->rank = at, at += up256(Q * P * 4);
  o->ivf = at, at += o->w.total;
  o->total = at;
  return true;
}

}  // namespace
}  // namespace lthm

extern "C" int64_t lthm_retrieve_ivf_shards_ws_bytes(const lthm_retrieve_ivf_shard* shards, int32_t S, int64_t Q,
                                                     int32_t nprobe, int32_t k, int64_t X, int32_t has_cursor) {
  RetrIvfShardsWs o;
  return retr_ivf_shards_ws(shards, S, Q, nprobe, k, X, has_cursor != 0, &o) ? o.total : -1;
}

extern "C" int lthm_retrieve_ivf_topk_shards(const lthm_retrieve_ivf_shard* shards, int32_t S, const void* q,
                                             int32_t q_dtype, int32_t normalize_q, int64_t Q, int32_t nprobe, int32_t k,
                                             const int32_t* exclude_rows, int64_t X, const int32_t* tag_filter,
                                             int32_t use_bias, const float* bias_weight,
                                             const lthm_retrieve_ivf_cursor* c, const int32_t* target_rows,
                                             const float* target_score, float* out_scores, int64_t* out_ids,
                                             int64_t* out_rank, void* workspace, int64_t ws_bytes, void* stream) {
  LTHM_REQUIRE(shards && q && out_scores && out_ids && workspace);
  LTHM_REQUIRE((target_rows != nullptr) == (target_score != nullptr) && (target_rows != nullptr) == (out_rank != nullptr));
  LTHM_REQUIRE(((uintptr_t)target_rows & 3) == 0 && ((uintptr_t)target_score & 3) == 0 && ((uintptr_t)out_rank & 7) == 0);
  LTHM_REQUIRE(q_dtype == LTHM_F32 || q_dtype == LTHM_BF16);
  LTHM_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)workspace & 255) == 0);
  LTHM_REQUIRE(((uintptr_t)out_scores & 3) == 0 && ((uintptr_t)out_ids & 7) == 0);
  LTHM_REQUIRE((exclude_rows != nullptr) == (X > 0) && ((uintptr_t)exclude_rows & 3) == 0);
  LTHM_REQUIRE(((uintptr_t)tag_filter & 3) == 0 && ((uintptr_t)bias_weight & 3) == 0 && (use_bias || !bias_weight));
  LTHM_REQUIRE(!c || (c->after_score && c->after_id && ((uintptr_t)c->after_score & 3) == 0 &&
                      ((uintptr_t)c->after_id & 7) == 0));
  RetrIvfShardsWs wo;
  LTHM_REQUIRE(retr_ivf_shards_ws(shards, S, Q, nprobe, k, X, c != nullptr, &wo) && ws_bytes >= wo.total);
  const bool deep = k > RT_KMAX;
  RetrIvfShardPack pk[(RS_SMAX + RI_PACK - 1) / RI_PACK] = {};
  int sP[RS_SMAX], sPbase[RS_SMAX];  // every shard's probe slots and the first of them
  {
    int lbase = 0, pbase = 0;
    for (int s = 0; s < S; ++s) {
      const lthm_retrieve_ivf_shard& h = shards[s];
      LTHM_REQUIRE(h.items && h.row_ids && h.list_off && h.centroids);
      LTHM_REQUIRE(((uintptr_t)h.items & 15) == 0 && ((uintptr_t)h.centroids & 15) == 0);
      LTHM_REQUIRE(((uintptr_t)h.row_ids & 7) == 0 && ((uintptr_t)h.list_off & 7) == 0);
      LTHM_REQUIRE(((uintptr_t)h.tags & 3) == 0 && ((uintptr_t)h.bias & 3) == 0);
      LTHM_REQUIRE(!tag_filter || h.tags);
      LTHM_REQUIRE(!use_bias || h.bias);
      RetrIvfShardDev& d = pk[s / RI_PACK].d[s % RI_PACK];
      d.items = (const bf16_t*)h.items;
      d.row_ids = h.row_ids;
      d.list_off = h.list_off;
      d.tags = tag_filter ? h.tags : nullptr;
      d.bias = use_bias ? h.bias : nullptr;
      d.N = h.N;
      d.lbase = lbase;
      sP[s] = (int)(h.L < nprobe ? h.L : nprobe), sPbase[s] = pbase;
      lbase += (int)h.L, pbase += sP[s];
    }
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  RetrIvfShardDev* dsh = (RetrIvfShardDev*)(ws + wo.desc);
  for (int s0 = 0; s0 < S; s0 += RI_PACK) {
    const int n = S - s0 < RI_PACK ? S - s0 : RI_PACK;
    hipLaunchKernelGGL(retr_ivf_desc_k, dim3(1), dim3(64), 0, st, pk[s0 / RI_PACK], n, dsh + s0);
    LTHM_CHECK_LAUNCH();
  }
  const int64_t L = wo.L, P = wo.P, NP = Q * P;
  int* probes = (int*)(ws + wo.probes);
  int* prow = (int*)(ws + wo.prow);
  // 1: every shard's probe row
  for (int s = 0; s < S; ++s) {
    const RetrIvfShardDev& d = pk[s / RI_PACK].d[s % RI_PACK];
    lthm_retrieve_desc pd = {};
    pd.items = shards[s].centroids;
    pd.N = shards[s].L;
    pd.q = q;
    pd.q_dtype = q_dtype;
    pd.normalize_q = normalize_q;
    pd.Q = Q;
    pd.k = sP[s];
    pd.slab_rows = 0;
    pd.scores = (float*)(ws + wo.pscore);
    pd.rows = prow;
    pd.workspace = ws + wo.pws;
    pd.ws_bytes = wo.pws_bytes;
    const int rc = retr_scan(&pd, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(retr_ivf_probe_pack_k, dim3((unsigned)((Q * sP[s] + 255) / 256)), dim3(256), 0, st, prow, Q, sP[s],
                       d.lbase, sPbase[s], (int)P, probes);
    LTHM_CHECK_LAUNCH();
  }
  // 2: retr_ivf_call's preparation and plan over all lists
  unsigned char* iw = ws + wo.ivf;
  const RetrIvfWs& w = wo.w;
  bf16_t* qn = (bf16_t*)(iw + w.qn);
  int* cnt = (int*)(iw + w.cnt);
  int* fill = cnt + L;
  int* pair_off = (int*)(iw + w.off);
  int* tile_off = pair_off + (L + 1);
  int* pair_idx = (int*)(iw + w.pidx);
  int4* tab = (int4*)(iw + w.tab);
  float* lscores = (float*)(iw + w.scores);
  int64_t* lids = (int64_t*)(iw + w.ids);
  const bf16_t* it0 = (const bf16_t*)shards[0].items;  // retr_prep_k reads no item without a target
  const unsigned pgrid = (unsigned)((Q + 15) / 16);
  if (q_dtype == LTHM_BF16)
    hipLaunchKernelGGL((retr_prep_k<bf16_t>), dim3(pgrid), dim3(256), 0, st, (const bf16_t*)q, Q, normalize_q, qn, it0,
                       shards[0].N, (const int*)nullptr, (float*)nullptr, -INFINITY);
  else
    hipLaunchKernelGGL((retr_prep_k<float>), dim3(pgrid), dim3(256), 0, st, (const float*)q, Q, normalize_q, qn, it0,
                       shards[0].N, (const int*)nullptr, (float*)nullptr, -INFINITY);
  LTHM_CHECK_LAUNCH();
  {
    const hipError_t e = hipMemsetAsync(cnt, 0, (size_t)(2 * L) * 4, st);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned ngrid = (unsigned)((NP + 255) / 256);
  hipLaunchKernelGGL(retr_ivf_count_k, dim3(ngrid), dim3(256), 0, st, probes, NP, (int)L, (int)P, Q, (int)k, cnt, lscores,
                     lids);
  LTHM_CHECK_LAUNCH();
  hipLaunchKernelGGL(retr_ivf_offsets_k<false>, dim3(1), dim3(256), 0, st, cnt, (int)L, pair_off, tile_off, RT_QT);
  LTHM_CHECK_LAUNCH();
  hipLaunchKernelGGL(retr_ivf_fill_k<false>, dim3(ngrid), dim3(256), 0, st, probes, NP, (int)L, cnt, pair_off, tile_off,
                     fill, pair_idx, tab, RT_QT);
  LTHM_CHECK_LAUNCH();
  RetrIvfShardArgs a = {};
  a.keys = deep ? (u64*)(iw + w.keys) : nullptr;
  a.sh = dsh;
  a.S = S;
  a.filt = tag_filter;
  a.bw = bias_weight;
  if (c) {
    int* crow = (int*)(iw + w.crow);
    hipLaunchKernelGGL(retr_ivf_cursor_shards_k, dim3(ngrid), dim3(256), 0, st, probes, NP, (int)L, (int)P, dsh, (int)S,
                       c->after_id, crow);
    LTHM_CHECK_LAUNCH();
    a.ascore = c->after_score;
    a.crow = crow;
  }
  a.qn = qn;
  a.tile_off = tile_off;
  a.tab = tab;
  a.pair_idx = pair_idx;
  a.scores = lscores;
  a.ids = lids;
  a.Q = Q;
  a.L = (int)L;
  a.P = (int)P;
  a.k = k;
  if (X) {
    int* xs = (int*)(ws + wo.xs);
    int XP = 1;
    while (XP < X) XP <<= 1;
    // one launch for the S Q lists.  The bound is the longest shard's: a row at or past its own shard's
    // N_s stays in the list and excludes nothing, since a block's walk ends at its list's end <= N_s
    LTHM_REQUIRE((int64_t)S * Q < (1ll << 31));
    hipLaunchKernelGGL(retr_excl_prep_k, dim3((unsigned)(S * Q)), dim3(256), 0, st, exclude_rows, (int)X, XP, wo.Nmax, xs);
    LTHM_CHECK_LAUNCH();
    a.xs = xs;
    a.xstride = (int)X + 1;
  }
  int* ranks = nullptr;
  if (target_rows) {
    ranks = (int*)(ws + wo.rank);
    const hipError_t e = hipMemsetAsync(ranks, 0, (size_t)NP * 4, st);
    if (e != hipSuccess) return (int)e;
    a.tsc = target_score;
    a.trow = target_rows;
    a.rank = ranks;
  }
  // 3: the scan
  const dim3 grid((unsigned)w.grid);
  const bool t = tag_filter != nullptr, b = use_bias != 0;
  if (deep) {
    if (t) hipLaunchKernelGGL((retr_ivf_deep_topk_k<true, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((retr_ivf_deep_topk_k<false, true>), grid, dim3(256), 0, st, a);
  } else if (t && b) {
    hipLaunchKernelGGL((retr_ivf_topk_k<true, true, true, true, false, true>), grid, dim3(256), 0, st, a);
  } else if (t) {
    hipLaunchKernelGGL((retr_ivf_topk_k<true, true, true, false, false, true>), grid, dim3(256), 0, st, a);
  } else if (b) {
    hipLaunchKernelGGL((retr_ivf_topk_k<true, true, false, true, false, true>), grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((retr_ivf_topk_k<true, true, false, false, false, true>), grid, dim3(256), 0, st, a);
  }
  LTHM_CHECK_LAUNCH();
  // 4: the merge of every query's P lists
  return lthm_retrieve_merge_shards(lscores, lids, ranks, (int32_t)P, Q, k, out_scores, out_ids, out_rank, stream);
}

// ---------------------------------------------------------------- diversified lists (MMR, per-group caps)
// lthm_retrieve_diversify: greedy maximal-marginal-relevance selection of k out of a pool of M <= 1024
// candidates per query, with at most `cap` selected items per non-zero group key.  One block of 256
// threads owns one query; thread t owns the candidates at pool positions t + 256 j, j < CPT = ceil(M /
// 256) <= 4, and keeps for each its score s, its running maximum similarity d to the selected set, its
// row, its group key and the key's count among the selected.
// Where the rows live: the candidates' bf16 rows are gathered ONCE into registers, 64 packed dwords
// per candidate (256 VGPRs at CPT = 4, inside the 512-register budget of one wave per SIMD that
// __launch_bounds__(256) gives).  1,024 rows (256 KiB) do not fit the 160 KiB LDS, and a re-read from
// global memory per step would put k dependent gathers on the critical path.  A step is then
//   1: every thread's best eligible key (retr_key of the objective, so one integer order decides:
//      objective descending, row ascending) with its pool position; the wave maximum by shuffles;
//      one LDS exchange between the four waves (barrier 1);
//   2: the winner's owner writes the outputs, the winner's row (256 B) and its group key to LDS
//      (barrier 2);
//   3: every thread reads the row back as 16 broadcast 16-byte LDS reads (all lanes one address: no
//      bank conflict), takes CPT x 128 multiply-adds, d = fmaxf(d, dot), and bumps the count of its
//      candidates that share the winner's non-zero key.
// Two candidates with equal keys (a row named twice in one pool) are told apart by the pool position,
// the lower first, so every output is a pure function of the inputs.  No atomics, no workspace.
// Every gather is guarded by 0 <= row < N and every pool read by position < M; an output index is
// below Q k.
namespace lthm {
namespace {

constexpr int RV_MMAX = 1024;  // the largest pool (RD_KMAX)
static_assert(RV_MMAX == RD_KMAX, "a deep list is a pool");

struct RetrDivShared {
  uint4 row[16];  // the winner's bf16 row
  u64 wkey[4];    // every wave's best key
  uint32_t wpos[4];  // and its pool position (RV_NONE: the wave has no eligible candidate)
  int gkey;       // the winner's group key
  // 16 and 0xffff0000, republished with every winner: the bf16 -> f32 unpacking of the candidates'
  // rows takes its shift and its mask from here, so that it stays inside the step loop.  With
  // literal constants the compiler hoists it and holds every row twice over, as 128 f32 (CPT = 4:
  // 256 VGPRs + 256 AGPRs and 1,292 bytes of scratch per lane)
  uint32_t shl, himask;
};
constexpr uint32_t RV_NONE = 0xffffffffu;


template <int CPT>
__global__ __launch_bounds__(256) void retr_diversify_k(const bf16_t* __restrict__ items, int64_t N,
                                                        const int* __restrict__ rows, const float* __restrict__ scores,
                                                        int M, int k, const float* __restrict__ lam,
                                                        const int* __restrict__ groups, int cap, int* __restrict__ out_rows,
                                                        float* __restrict__ out_scores, float* __restrict__ out_obj) {
  __shared__ __attribute__((aligned(16))) RetrDivShared sh;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t q = blockIdx.x;
  const float l = lam ? lam[q] : 1.f;
  const float nl = -(1.0f - l);
  uint4 r[CPT][16];
  float s[CPT], d[CPT];
  int row[CPT], gk[CPT], gc[CPT];
  uint32_t avail = 0;  // bit j: candidate j is one and is not yet selected
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int pos = tid + 256 * j;
    int rw = -1;
    float sc = -INFINITY;
    if (pos < M) {
      rw = rows[q * M + pos];
      sc = scores[q * M + pos];
    }
    const bool ok = rw >= 0 && (int64_t)rw < N && sc == sc && sc != -INFINITY;
    row[j] = rw;
    s[j] = sc;
    d[j] = 0.f;
    gk[j] = ok && groups ? groups[rw] : 0;
    gc[j] = 0;
    avail |= ok ? 1u << j : 0u;
    const uint4* src = (const uint4*)(items + (int64_t)(ok ? rw : 0) * RT_D);
#pragma unroll
    for (int e = 0; e < 16; ++e) r[j][e] = ok ? src[e] : make_uint4(0, 0, 0, 0);
  }
  int t = 0;
  for (; t < k; ++t) {
    // 1: the best eligible candidate of the thread, the wave, the block
    u64 bk = 0;
    uint32_t bp = RV_NONE;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const bool el = ((avail >> j) & 1u) && (gk[j] == 0 || gc[j] < cap);
      const u64 key = retr_key(fmaf(nl, d[j], l * s[j]), row[j]);
      if (el && key > bk) bk = key, bp = (uint32_t)(tid + 256 * j);  // ascending positions: a tie keeps the lower
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 ok = __shfl_xor(bk, o, 64);
      const uint32_t op = __shfl_xor(bp, o, 64);
      if (ok > bk || (ok == bk && op < bp)) bk = ok, bp = op;
    }
    if (lane == 0) sh.wkey[w] = bk, sh.wpos[w] = bp;
    __syncthreads();
    bk = sh.wkey[0], bp = sh.wpos[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      const u64 ok = sh.wkey[i];
      const uint32_t op = sh.wpos[i];
      if (ok > bk || (ok == bk && op < bp)) bk = ok, bp = op;
    }
    if (bp == RV_NONE) break;  // nothing eligible: the same in every thread
    // 2: the winner's owner publishes it
    if ((int)(bp & 255u) == tid) {
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        if ((int)(bp >> 8) == j) {
#pragma unroll
          for (int e = 0; e < 16; ++e) sh.row[e] = r[j][e];
          sh.gkey = gk[j];
          sh.shl = 16u, sh.himask = 0xffff0000u;
          out_rows[q * k + t] = row[j];
          out_scores[q * k + t] = s[j];
          out_obj[q * k + t] = fmaf(nl, d[j], l * s[j]);
          avail &= ~(1u << j);
        }
      }
    }
    __syncthreads();
    // 3: the similarity of every own candidate to the winner
    const int g = sh.gkey;
    const uint32_t shl = sh.shl, him = sh.himask;
    float acc[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) acc[j] = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const uint4 wv = sh.row[e];
      const uint32_t wu[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const uint32_t cu[4] = {r[j][e].x, r[j][e].y, r[j][e].z, r[j][e].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          acc[j] = fmaf(__uint_as_float(cu[c] << shl), __uint_as_float(wu[c] << 16), acc[j]);
          acc[j] = fmaf(__uint_as_float(cu[c] & him), __uint_as_float(wu[c] & 0xffff0000u), acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      d[j] = fmaxf(d[j], acc[j]);
      gc[j] += (g != 0 && gk[j] == g) ? 1 : 0;
    }
  }
  // the empty rest of the list (t is the same in every thread)
  for (int p = t + tid; p < k; p += 256) {
    out_rows[q * k + p] = -1;
    out_scores[q * k + p] = -INFINITY;
    out_obj[q * k + p] = -INFINITY;
  }
}

}  // namespace
}  // namespace lthm

extern "C" int64_t lthm_retrieve_diversify_ws_bytes(int64_t Q, int64_t M, int32_t k) {
  if (Q < 1 || Q >= (1ll << 31) || M < 1 || M > RV_MMAX || k < 1 || k > RT_KMAX) return -1;
  return 0;  // the candidates' rows live in registers
}

extern "C" int lthm_retrieve_diversify(const void* items, int64_t N, const int32_t* rows, const float* scores, int64_t Q,
                                       int32_t M, int32_t k, const float* lam, const int32_t* groups, int32_t cap,
                                       int32_t* out_rows, float* out_scores, float* out_obj, void* workspace,
                                       int64_t ws_bytes, void* stream) {
  LTHM_REQUIRE(items && rows && scores && out_rows && out_scores && out_obj);
  LTHM_REQUIRE(N >= 1 && N < (1ll << 31));
  const int64_t need = lthm_retrieve_diversify_ws_bytes(Q, M, k);
  LTHM_REQUIRE(need >= 0 && ws_bytes >= need && (workspace || need == 0));
  LTHM_REQUIRE(!groups || cap >= 1);
  LTHM_REQUIRE(((uintptr_t)items & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
  LTHM_REQUIRE(((uintptr_t)rows & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)lam & 3) == 0 &&
               ((uintptr_t)groups & 3) == 0);
  LTHM_REQUIRE(((uintptr_t)out_rows & 3) == 0 && ((uintptr_t)out_scores & 3) == 0 && ((uintptr_t)out_obj & 3) == 0);
  hipStream_t s = (hipStream_t)stream;
  const bf16_t* it = (const bf16_t*)items;
  const dim3 grid((unsigned)Q), block(256);
  if (M <= 256)
    hipLaunchKernelGGL(retr_diversify_k<1>, grid, block, 0, s, it, N, rows, scores, (int)M, (int)k, lam, groups, (int)cap,
                       out_rows, out_scores, out_obj);
  else if (M <= 512)
    hipLaunchKernelGGL(retr_diversify_k<2>, grid, block, 0, s, it, N, rows, scores, (int)M, (int)k, lam, groups, (int)cap,
                       out_rows, out_scores, out_obj);
  else
    hipLaunchKernelGGL(retr_diversify_k<4>, grid, block, 0, s, it, N, rows, scores, (int)M, (int)k, lam, groups, (int)cap,
                       out_rows, out_scores, out_obj);
  LTHM_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- e4m3 catalogues: scan codes, re-score in bf16
// A row x[0..127] (bf16) with a = max |x_k| is stored as 128 OCP e4m3fn codes and one f32 scale:
// e = the largest integer with a 2^e <= 448 (clamped to [-64, 64]; 0 for a zero row), code_k =
// e4m3(x_k 2^e) (the product is exact in f32), scale = 2^-e.  The approximate score of a query
// (quantised the same way from the bf16 row that retr_prep_k forms) against a row is
//   s^[q, j] = acc (scale_q scale_j),   acc = sum_k cq_k c_jk  (f32 MFMA accumulation from zero),
// two explicit f32 multiplies by powers of two.
//   retr_q8_quant_k   16 lanes per row: amax by integer maximum of the bf16 magnitudes, the
//                     exponent from the f32 exponent and significand bits, cvt_pk_fp8_f32;
//   retr_q8_topk_k    retr_deep_topk_k<1, false>'s tile loop, keys-in-workspace selection, flagged
//                     bitonic prune and slab lists over 64 x 128 B images; the codes of a fragment
//                     become bf16 in registers (exactly: an e4m3 value has four significand bits) and
//                     feed the flat scan's eight v_mfma_f32_32x32x16_bf16 per wave and tile, whose
//                     accumulation is the f32 chain the contract names (the block-scaled
//                     v_mfma_scale_f32_32x32x64_f8f6f4 sums its 64 products more coarsely: measured
//                     2^-15.3 of sum|a b| against the chain's 2^-17); the 64 row
//                     scales of tile i + 1 ride with its image the way the bias words do; the slabs'
//                     lists go through retr_deep_merge_k;
//   retr_rescore_k    one block per query: 32 listed rows at a time as A rows gathered from the bf16
//                     catalogue, the query in every B column, the flat scan's eight-step
//                     v_mfma_f32_32x32x16_bf16 chain, keys sorted in LDS by retr_deep_sort.
// The queries go through retr_prep_k itself (no target) and then through retr_q8_quant_k: a query's
// codes are the catalogue's rule applied to the bf16 row, so no second prep kernel exists.
//
// The e4m3 image: chunk ch (16 B) of row r at r 128 + ((ch ^ ((r >> 1) & 7)) << 4).  A 256-B bank
// row holds two image rows of eight slots; the 16 lanes of one ds_read_b128 group read one chunk
// of the rows {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} (+ 32 for the upper lanes), whose even
// (and odd) members have eight distinct (r >> 1) & 7: 16 distinct slots, no conflict, for either
// chunk of a fragment.
namespace lthm {
namespace {

constexpr int RQ_ROWB = 128;  // bytes of a row of codes

// 16 e4m3 codes (four words) as two bf16 fragments of eight, in byte order: v_cvt_pk_f32_fp8 and
// v_cvt_pk_bf16_f32, both exact here
__device__ __forceinline__ void retr_q8_frags(const u32x4& c, bf16x8v& f0, bf16x8v& f1) {
  u32x4 w[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], true);
    w[i >> 1][2 * (i & 1)] = pack_bf16x2(lo[0], lo[1]);
    w[i >> 1][2 * (i & 1) + 1] = pack_bf16x2(hi[0], hi[1]);
  }
  f0 = __builtin_bit_cast(bf16x8v, w[0]);
  f1 = __builtin_bit_cast(bf16x8v, w[1]);
}

struct RetrQ8Shared {
  unsigned char img[2][RT_IT * RQ_ROWB];
  u64 sort[4][RD_CAP];  // one buffer per wave
  float tau[RT_QT];
  int cnt[RT_QT];
  int flag[3];
  alignas(16) float scl[2][RT_IT];
};
static_assert(sizeof(RetrQ8Shared) <= 96 * 1024, "LDS budget: the images, four sort buffers and change");

struct RetrQ8Args {
  const unsigned char* codes;  // [N, 128] e4m3fn
  const float* scale;          // [N]
  const unsigned char* cq;     // [Q, 128] the queries' codes
  const float* sq;             // [Q]
  u64* keys;                   // [nslab, Q, stride]
  const int* xs;               // [Q, xstride] ascending (EXCL)
  int64_t Q, N, slab_rows;
  int k, stride, xstride;
};

// 16 lanes per row, 8 contiguous elements per lane
__global__ __launch_bounds__(256) void retr_q8_quant_k(const bf16_t* __restrict__ x, int64_t R,
                                                       unsigned char* __restrict__ codes, float* __restrict__ scale) {
  const int sub = threadIdx.x & 15;
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool in = r0 < R;
  const int64_t r = in ? r0 : R - 1;  // every lane takes part in the group maximum
  const u32x4 w = *reinterpret_cast<const u32x4*>(x + r * RT_D + 8 * sub);
  // the magnitudes as integers: their order is the order of the values
  uint32_t am = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t lo = w[i] & 0x7fffu, hi = (w[i] >> 16) & 0x7fffu;
    am = am > lo ? am : lo;
    am = am > hi ? am : hi;
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)am, o, 64);
    am = am > other ? am : other;
  }
  // a = 1.f 2^(E - 127) = m 2^p with m = 1.f / 2, p = E - 126: m <= 0.875 iff the seven significand
  // bits are <= 0x60.  A subnormal a (E = 0) has p <= -126 and lands on the upper clamp.
  int e = 0;
  if (am != 0u) {
    const int E = (int)(am >> 7);
    e = ((am & 0x7fu) <= 0x60u ? 135 : 134) - E;
    if (E == 0) e = 64;
    e = e < -64 ? -64 : e > 64 ? 64 : e;
  }
  const float up = __uint_as_float((uint32_t)(127 + e) << 23);
  float v[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = fminf(fmaxf(__uint_as_float(w[i] << 16) * up, -448.f), 448.f);
    v[2 * i + 1] = fminf(fmaxf(__uint_as_float(w[i] & 0xffff0000u) * up, -448.f), 448.f);
  }
  u32x2 c;
  c[0] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
  c[0] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], (int)c[0], true);
  c[1] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], 0, false);
  c[1] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], (int)c[1], true);
  // two lanes' words side by side: the even lane writes 16 bytes
  u32x4 c4;
  c4[0] = c[0];
  c4[1] = c[1];
  c4[2] = (uint32_t)__shfl_xor((int)c[0], 1, 64);
  c4[3] = (uint32_t)__shfl_xor((int)c[1], 1, 64);
  if (in && !(sub & 1)) *reinterpret_cast<u32x4*>(codes + r * RQ_ROWB + 8 * sub) = c4;
  if (in && sub == 0) scale[r] = __uint_as_float((uint32_t)(127 - e) << 23);
}

// Wave w: queries 32 (w & 1) + (lane & 31) of the tile, image rows 32 (w >> 1) + 8 (v >> 2) +
// 4 (lane >> 5) + (v & 3), as in retr_deep_topk_k.  A lane holds row lane & 31, bytes 64 s +
// 32 (lane >> 5) .. + 31 for s = 0, 1 (chunks 4 s + 2 (lane >> 5) and the next one, two ds_read_b128);
// MFMA step 4 s + t takes bytes 8 t .. 8 t + 7 of them, for the item rows and the queries alike, so
// both lane halves together cover every k once and an A element meets the B element of its own k.
template <bool EXCL>
__global__ __launch_bounds__(256) void retr_q8_topk_k(RetrQ8Args a) {
  __shared__ __attribute__((aligned(16))) RetrQ8Shared sh;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5, ih = w >> 1;
  const int64_t q0 = (int64_t)blockIdx.x * RT_QT;
  const int slab = blockIdx.y;
  const int64_t row_lo = (int64_t)slab * a.slab_rows;
  const int64_t row_hi = row_lo + a.slab_rows < a.N ? row_lo + a.slab_rows : a.N;
  const int ntile = (int)((row_hi - row_lo + RT_IT - 1) / RT_IT);
  const int ql = 32 * (w & 1) + r32;
  const int64_t q = q0 + ql;
  const bool live = q < a.Q;
  const int stride = a.stride;

  if (tid < RT_QT) {
    sh.tau[tid] = q0 + tid < a.Q ? -INFINITY : INFINITY;  // a query past Q never passes the filter
    sh.cnt[tid] = 0;
  }
  if (tid < 3) sh.flag[tid] = 0;

  bf16x8v qf[8];
  float sq = 0.f;
  {
    const unsigned char* rp = a.cq + (live ? q : 0) * RQ_ROWB;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
      if (live) {
        lo = *reinterpret_cast<const u32x4*>(rp + 64 * s + 32 * hh);
        hi = *reinterpret_cast<const u32x4*>(rp + 64 * s + 32 * hh + 16);
      }
      retr_q8_frags(lo, qf[4 * s], qf[4 * s + 1]);
      retr_q8_frags(hi, qf[4 * s + 2], qf[4 * s + 3]);
    }
    if (live) sq = a.sq[q];
  }
  const int* xp = nullptr;
  int nx = INT_MAX;  // a query past Q excludes nothing and reads nothing
  if constexpr (EXCL) {
    if (live) {
      const int* xl = a.xs + q * a.xstride;
      int lo = 0, hi = a.xstride - 1;  // xl[hi] = INT_MAX >= row_lo
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xl[mid] < row_lo) lo = mid + 1;
        else hi = mid;
      }
      xp = xl + lo;
      nx = *xp;
    }
  }
  // a lane that is not live never appends (its tau is +inf)
  u64* const kbuf = a.keys + ((int64_t)slab * a.Q + (live ? q : 0)) * stride;
  int roff[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int R = 32 * ih + r32, ch = 4 * (c >> 1) + 2 * hh + (c & 1);
    roff[c] = R * RQ_ROWB + ((ch ^ ((R >> 1) & 7)) << 4);
  }

  // wave w stages rows 16 w .. 16 w + 15 of an image with two DMAs of 8 rows x 128 B (lane l: row
  // 16 w + 8 j + l / 8, slot l % 8, source chunk slot ^ ((row >> 1) & 7) = slot ^ (l / 16) ^ 4 j);
  // rows at or past row_hi come from the zero row
  const int srow = 16 * w + (lane >> 3), sch = (lane & 7) ^ (lane >> 4);
  auto stage = [&](int t) {
    unsigned char* img = sh.img[t & 1];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t row = row_lo + (int64_t)RT_IT * t + srow + 8 * j;
      const void* src = row < row_hi ? (const void*)(a.codes + row * RQ_ROWB + ((sch ^ (4 * j)) << 4))
                                     : (const void*)(retr_zero_row + 16 * (lane & 7));
      glds16(src, img + (16 * w + 8 * j) * RQ_ROWB);
    }
    // wave 1, lane l: the scale of the image's row l; never a read at or past row_hi <= N
    if (w == 1) {
      const int64_t row = row_lo + (int64_t)RT_IT * t + lane;
      glds4(row < row_hi ? a.scale + row : &retr_zero_bias, sh.scl[t & 1]);
    }
  };
  retire_loads();
  stage(0);
  for (int i = 0; i < ntile; ++i) {
    // the key stores of tile i - 1 count in vmcnt like the DMA: this wait retires both
    wait_vm<0>();
    __syncthreads();  // image i landed; every wave is past tile i - 1 (its image and its appends)
    if (i + 1 < ntile) stage(i + 1);
    if (tid == 0) sh.flag[(i + 1) % 3] = 0;
    if (sh.flag[(i + 2) % 3]) {  // tile i - 1 pushed a query past the limit
      for (int pq = w; pq < RT_QT; pq += 4) {
        int n = sh.cnt[pq];
        if (n > RD_LIM) {
          n = n < stride ? n : stride;
          u64* g = a.keys + ((int64_t)slab * a.Q + q0 + pq) * stride;
          const int m = retr_deep_prune(g, sh.sort[w], n, a.k, false, lane);
          if (lane == 0) {
            sh.cnt[pq] = m;
            if (m == a.k) sh.tau[pq] = retr_key_score(sh.sort[w][a.k - 1]);
          }
        }
      }
      __syncthreads();
    }
    const unsigned char* img = sh.img[i & 1];
    // the lane's rows are four runs of four consecutive scale words (broadcast reads): element
    // 4 j + c is image row 32 ih + 4 hh + 8 j + c
    float4 s4[4];
    {
      const float4* sp = reinterpret_cast<const float4*>(sh.scl[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) s4[j] = sp[2 * j];
    }
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const u32x4 lo = *reinterpret_cast<const u32x4*>(img + roff[2 * s]);
      const u32x4 hi = *reinterpret_cast<const u32x4*>(img + roff[2 * s + 1]);
      bf16x8v af[4];
      retr_q8_frags(lo, af[0], af[1]);
      retr_q8_frags(hi, af[2], af[3]);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = mfma32(af[t], qf[4 * s + t], acc);
    }
    // the score from here on: acc (scale_q scale_j), two multiplies by powers of two
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float sj[4] = {s4[j].x, s4[j].y, s4[j].z, s4[j].w};
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[4 * j + c] = acc[4 * j + c] * (sq * sj[c]);
    }
    const int64_t rb = row_lo + (int64_t)RT_IT * i + 32 * ih + 4 * hh;
    if (row_lo + (int64_t)RT_IT * (i + 1) > row_hi) {  // partial tile: the rows past the slab never pass
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (rb + 8 * (v >> 2) + (v & 3) >= row_hi) acc[v] = -INFINITY;
    }
    if constexpr (EXCL) {
      const int64_t tile_end = row_lo + (int64_t)RT_IT * (i + 1) < row_hi ? row_lo + (int64_t)RT_IT * (i + 1) : row_hi;
      unsigned xm = 0u;
      while (nx < tile_end) {
        const int64_t xrel = (int64_t)nx - rb;
        if (xrel >= 0 && xrel < 32 && !(xrel & 4)) xm |= 1u << (int)(((xrel >> 3) << 2) | (xrel & 3));
        nx = *++xp;
      }
      if (xm) {
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if ((xm >> v) & 1u) acc[v] = -INFINITY;
      }
    }
    float mx = acc[0];
#pragma unroll
    for (int v = 1; v < 16; ++v) mx = fmaxf(mx, acc[v]);
    const float tau = sh.tau[ql];
    if (mx >= tau) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float s = acc[v];
        if (s >= tau && s > -INFINITY) {
          const int slot = atomicAdd(&sh.cnt[ql], 1);
          if (live && slot < stride) kbuf[slot] = retr_key(s, (int)(rb + 8 * (v >> 2) + (v & 3)));
          if (slot >= RD_LIM) sh.flag[i % 3] = 1;
        }
      }
    }
  }
  __syncthreads();  // the last tile's appends have left their waves
  // the slab's k best of every query, sorted, in the first k of its slots; empty slots are key 0
  for (int pq = w; pq < RT_QT; pq += 4) {
    if (q0 + pq >= a.Q) break;
    int n = sh.cnt[pq];
    n = n < stride ? n : stride;
    u64* g = a.keys + ((int64_t)slab * a.Q + q0 + pq) * stride;
    retr_deep_prune(g, sh.sort[w], n, a.k, true, lane);
  }
}

// One block per query.  Wave w takes the list entries 32 t .. 32 t + 31 for t = w, w + 4, ..: entry
// 32 t + (lane & 31) is A row lane & 31 (an entry outside [0, N) reads row 0 and becomes key 0), the
// query is every B column, so every column of the accumulator holds the 32 scores; lane (r < 16, h)
// owns element r of its registers: entry 32 t + 8 (r >> 2) + 4 h + (r & 3).
//
// BIAS (lthm_retrieve_rescore_bias; the prior rides behind the plain arguments, so that <false> keeps
// the argument block and the text it always had): a listed row's score becomes fmaf(wq, bias[row],
// dot), one explicit fma on the MFMA's score.  With p.oids the low word of a key is not the row but
// the entry's rank among the list's entries under (p.oids[row] ascending, list position ascending)
// (one pass of P broadcast LDS reads per entry; entries that are no candidates rank behind every row),
// so that equal scores come out in id order, and the sorted keys are mapped back through the inverse.
struct RetrRescorePrior {
  const float* bias;    // [N] or null
  const float* bw;      // [Q] or null: 1 for everyone
  const int64_t* oids;  // [N] or null: ties by row
};
template <bool BIAS, class... Prior>
__global__ __launch_bounds__(256) void retr_rescore_k(const bf16_t* __restrict__ items, int64_t N,
                                                      const bf16_t* __restrict__ qn, const int* __restrict__ rows,
                                                      int M, int k, float* __restrict__ scores,
                                                      int* __restrict__ out_rows, Prior... prior) {
  __shared__ u64 keys[RD_KMAX];
  __shared__ int srow[RD_KMAX];
  __shared__ int64_t sid[BIAS ? RD_KMAX : 1];
  __shared__ int spos[BIAS ? RD_KMAX : 1], sinv[BIAS ? RD_KMAX : 1];
  RetrRescorePrior pr = {nullptr, nullptr, nullptr};
  if constexpr (BIAS) pr = (prior, ...);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5;
  const int64_t q = blockIdx.x;
  const int P = M <= 512 ? 512 : RD_KMAX;
  for (int i = tid; i < P; i += 256) {
    int r = -1;
    if (i < M) {
      r = rows[q * M + i];
      if (r < 0 || r >= N) r = -1;
    }
    srow[i] = r;
    keys[i] = 0ull;
  }
  bf16x8v qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s)
    qf[s] = __builtin_bit_cast(bf16x8v, *reinterpret_cast<const u32x4*>(qn + q * RT_D + 16 * s + 8 * hh));
  __syncthreads();
  float wq = 1.f;
  if constexpr (BIAS) {
    if (pr.bw) wq = pr.bw[q];
    if (pr.oids) {  // uniform
      for (int i = tid; i < P; i += 256) sid[i] = srow[i] >= 0 ? pr.oids[srow[i]] : INT64_MAX;
      __syncthreads();
      for (int i = tid; i < P; i += 256) {
        const int64_t mine = sid[i];
        int rk = 0;
        for (int j = 0; j < P; ++j) {
          const int64_t o = sid[j];
          rk += (o < mine || (o == mine && j < i)) ? 1 : 0;
        }
        spos[i] = rk;  // a permutation of 0..P-1
        sinv[rk] = i;
      }
      __syncthreads();
    }
  }
  const int ntile = (M + 31) / 32;
  for (int t = w; t < ntile; t += 4) {
    const int ar = srow[32 * t + r32];
    const bf16_t* rp = items + (int64_t)(ar < 0 ? 0 : ar) * RT_D + 8 * hh;
    u32x4 av[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) av[s] = *reinterpret_cast<const u32x4*>(rp + 16 * s);
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = mfma32(__builtin_bit_cast(bf16x8v, av[s]), qf[s], acc);
    float mine = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v)
      if (r32 == v) mine = acc[v];
    if (r32 < 16) {
      const int e = 32 * t + 8 * (r32 >> 2) + 4 * hh + (r32 & 3);
      const int er = srow[e];
      if constexpr (BIAS) {
        if (er >= 0) {
          const float sc = pr.bias ? __builtin_fmaf(wq, pr.bias[er], mine) : mine;
          keys[e] = retr_key(sc, pr.oids ? spos[e] : er);
        }
      } else {
        if (er >= 0) keys[e] = retr_key(mine, er);
      }
    }
  }
  __syncthreads();
  if (w == 0 && M > 1) retr_deep_sort(keys, P, lane);
  __syncthreads();
  for (int i = tid; i < k; i += 256) {
    const u64 key = keys[i];
    scores[q * k + i] = key ? retr_key_score(key) : -INFINITY;
    if constexpr (BIAS) {
      int r = key ? retr_key_row(key) : -1;
      if (key && pr.oids) r = srow[sinv[r]];  // the key's low word is a rank below P
      out_rows[q * k + i] = r;
    } else {
      out_rows[q * k + i] = key ? retr_key_row(key) : -1;
    }
  }
}

// the sizes both q8 entries share: rows per slab and slots per list, or false
inline bool retr_q8_plan(int64_t Q, int64_t N, int32_t M, int32_t slab_rows, int64_t* sr, int64_t* stride) {
  if (M < 1 || M > RD_KMAX || slab_rows < 0) return false;
  *sr = retr_slab_rows(Q, N, slab_rows, 4 * RD_KMAX);
  if (*sr < 0) return false;
  *stride = retr_deep_stride(*sr, M);
  return true;
}

}  // namespace
}  // namespace lthm

extern "C" int lthm_catalogue_quantize_q8(const void* items, int64_t N, uint8_t* codes, float* scale, void* stream) {
  LTHM_REQUIRE(items && codes && scale && N >= 1 && N < (1ll << 31));
  LTHM_REQUIRE(((uintptr_t)items & 15) == 0 && ((uintptr_t)codes & 15) == 0 && ((uintptr_t)scale & 3) == 0);
  hipLaunchKernelGGL(retr_q8_quant_k, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)items, N, codes, scale);
  LTHM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t lthm_retrieve_q8_ws_bytes(int64_t Q, int64_t N, int32_t M, int32_t slab_rows, int64_t X) {
  int64_t sr, stride;
  if (X < 0 || X > RT_XMAX || !retr_q8_plan(Q, N, M, slab_rows, &sr, &stride)) return -1;
  const int64_t nslab = (N + sr - 1) / sr;
  return up256(Q * RT_D * 2) + up256(Q * RQ_ROWB) + up256(Q * 4) + up256(nslab * Q * stride * 8) +
         (X ? up256(Q * (X + 1) * 4) : 0);
}

extern "C" int lthm_retrieve_q8_topk(const uint8_t* codes, const float* scale, int64_t N, const void* q, int32_t q_dtype,
                                     int32_t normalize_q, int64_t Q, int32_t M, int32_t slab_rows,
                                     const lthm_retrieve_excl* x, float* out_scores, int32_t* out_rows, void* workspace,
                                     int64_t ws_bytes, void* stream) {
  LTHM_REQUIRE(codes && scale && q && out_scores && out_rows && workspace);
  LTHM_REQUIRE(q_dtype == LTHM_F32 || q_dtype == LTHM_BF16);
  LTHM_REQUIRE(((uintptr_t)codes & 15) == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
  LTHM_REQUIRE(((uintptr_t)scale & 3) == 0 && ((uintptr_t)out_scores & 3) == 0 && ((uintptr_t)out_rows & 3) == 0);
  LTHM_REQUIRE(!x || (x->rows && x->X >= 1 && x->X <= RT_XMAX && ((uintptr_t)x->rows & 3) == 0));
  const int64_t need = lthm_retrieve_q8_ws_bytes(Q, N, M, slab_rows, x ? x->X : 0);
  LTHM_REQUIRE(need >= 0 && ws_bytes >= need);
  int64_t sr, stride;
  retr_q8_plan(Q, N, M, slab_rows, &sr, &stride);
  const int64_t nslab = (N + sr - 1) / sr;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  bf16_t* qn = (bf16_t*)ws;
  ws += up256(Q * RT_D * 2);
  unsigned char* cq = ws;
  ws += up256(Q * RQ_ROWB);
  float* sq = (float*)ws;
  ws += up256(Q * 4);
  u64* keys = (u64*)ws;
  ws += up256(nslab * Q * stride * 8);
  int* xs = (int*)ws;
  const unsigned pgrid = (unsigned)((Q + 15) / 16);
  // the flat call's query rows, then the catalogue's quantiser on them
  if (q_dtype == LTHM_BF16)
    hipLaunchKernelGGL((retr_prep_k<bf16_t>), dim3(pgrid), dim3(256), 0, s, (const bf16_t*)q, Q, normalize_q, qn,
                       (const bf16_t*)nullptr, N, (const int*)nullptr, (float*)nullptr, -INFINITY);
  else
    hipLaunchKernelGGL((retr_prep_k<float>), dim3(pgrid), dim3(256), 0, s, (const float*)q, Q, normalize_q, qn,
                       (const bf16_t*)nullptr, N, (const int*)nullptr, (float*)nullptr, -INFINITY);
  LTHM_CHECK_LAUNCH();
  hipLaunchKernelGGL(retr_q8_quant_k, dim3(pgrid), dim3(256), 0, s, (const bf16_t*)qn, Q, cq, sq);
  LTHM_CHECK_LAUNCH();
  RetrQ8Args a;
  a.codes = codes;
  a.scale = scale;
  a.cq = cq;
  a.sq = sq;
  a.keys = keys;
  a.xs = nullptr;
  a.Q = Q;
  a.N = N;
  a.slab_rows = sr;
  a.k = M;
  a.stride = (int)stride;
  a.xstride = 0;
  const dim3 tgrid((unsigned)((Q + RT_QT - 1) / RT_QT), (unsigned)nslab);
  if (x) {
    const int X = (int)x->X;
    int P = 1;
    while (P < X) P <<= 1;
    hipLaunchKernelGGL(retr_excl_prep_k, dim3((unsigned)Q), dim3(256), 0, s, x->rows, X, P, N, xs);
    LTHM_CHECK_LAUNCH();
    a.xs = xs;
    a.xstride = X + 1;
    hipLaunchKernelGGL(retr_q8_topk_k<true>, tgrid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(retr_q8_topk_k<false>, tgrid, dim3(256), 0, s, a);
  }
  LTHM_CHECK_LAUNCH();
  hipLaunchKernelGGL(retr_deep_merge_k, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, s, keys, (int)stride,
                     (const int*)nullptr, (const int*)nullptr, Q, N, (int)nslab, (int)M, out_scores, out_rows,
                     (int*)nullptr, (const float*)nullptr);
  LTHM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t lthm_retrieve_rescore_ws_bytes(int64_t Q, int32_t M, int32_t k) {
  if (Q < 1 || Q >= (1ll << 31) || M < 1 || M > RD_KMAX || k < 1 || k > M) return -1;
  return up256(Q * RT_D * 2);
}

// bias == NULL and order_ids == NULL is lthm_retrieve_rescore: retr_rescore_k<false>, as it always ran
extern "C" int lthm_retrieve_rescore_bias(const void* items, int64_t N, const void* q, int32_t q_dtype,
                                          int32_t normalize_q, int64_t Q, const int32_t* rows, int32_t M, int32_t k,
                                          const float* bias, const float* weight, const int64_t* order_ids,
                                          float* out_scores, int32_t* out_rows, void* workspace, int64_t ws_bytes,
                                          void* stream) {
  LTHM_REQUIRE(items && q && rows && out_scores && out_rows && workspace);
  LTHM_REQUIRE(N >= 1 && N < (1ll << 31));
  LTHM_REQUIRE(bias || !weight);
  LTHM_REQUIRE(((uintptr_t)bias & 3) == 0 && ((uintptr_t)weight & 3) == 0 && ((uintptr_t)order_ids & 7) == 0);
  LTHM_REQUIRE(q_dtype == LTHM_F32 || q_dtype == LTHM_BF16);
  LTHM_REQUIRE(((uintptr_t)items & 15) == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
  LTHM_REQUIRE(((uintptr_t)rows & 3) == 0 && ((uintptr_t)out_scores & 3) == 0 && ((uintptr_t)out_rows & 3) == 0);
  const int64_t need = lthm_retrieve_rescore_ws_bytes(Q, M, k);
  LTHM_REQUIRE(need >= 0 && ws_bytes >= need);
  hipStream_t s = (hipStream_t)stream;
  bf16_t* qn = (bf16_t*)workspace;
  const unsigned pgrid = (unsigned)((Q + 15) / 16);
  if (q_dtype == LTHM_BF16)
    hipLaunchKernelGGL((retr_prep_k<bf16_t>), dim3(pgrid), dim3(256), 0, s, (const bf16_t*)q, Q, normalize_q, qn,
                       (const bf16_t*)items, N, (const int*)nullptr, (float*)nullptr, -INFINITY);
  else
    hipLaunchKernelGGL((retr_prep_k<float>), dim3(pgrid), dim3(256), 0, s, (const float*)q, Q, normalize_q, qn,
                       (const bf16_t*)items, N, (const int*)nullptr, (float*)nullptr, -INFINITY);
  LTHM_CHECK_LAUNCH();
  if (bias || order_ids) {
    const RetrRescorePrior pr = {bias, weight, order_ids};
    hipLaunchKernelGGL((retr_rescore_k<true, RetrRescorePrior>), dim3((unsigned)Q), dim3(256), 0, s, (const bf16_t*)items,
                       N, (const bf16_t*)qn, rows, (int)M, (int)k, out_scores, out_rows, pr);
  } else {
    hipLaunchKernelGGL(retr_rescore_k<false>, dim3((unsigned)Q), dim3(256), 0, s, (const bf16_t*)items, N,
                       (const bf16_t*)qn, rows, (int)M, (int)k, out_scores, out_rows);
  }
  LTHM_CHECK_LAUNCH();
  return 0;
}

extern "C" int lthm_retrieve_rescore(const void* items, int64_t N, const void* q, int32_t q_dtype, int32_t normalize_q,
                                     int64_t Q, const int32_t* rows, int32_t M, int32_t k, float* out_scores,
                                     int32_t* out_rows, void* workspace, int64_t ws_bytes, void* stream) {
  return lthm_retrieve_rescore_bias(items, N, q, q_dtype, normalize_q, Q, rows, M, k, nullptr, nullptr, nullptr,
                                    out_scores, out_rows, workspace, ws_bytes, stream);
}

// ---------------------------------------------------------------- clustered e4m3 catalogues
// lthm_retrieve_ivf_q8_topk: retr_ivf_deep_topk_k's work unit and selection (the block, its list, its
// up to 64 pairs, the pairs' RD_CAP key slots in the workspace, the flagged bitonic prune, the final
// sort into the layout retr_shard_merge_k reads) over retr_q8_topk_k's tile body (64 x 128 B images of
// codes under its swizzle, the 64 row scales of tile i + 1 staged by wave 1, the codes of a fragment
// to bf16 in registers, its eight MFMA steps in its k order, acc (scale_q scale_j)).  The tag words of
// tile i + 1 ride with wave 0 as in retr_ivf_topk_k; the bias words with wave 2, since wave 1 carries
// the scales.  Order per tile: the score, the partial-tile mask, the prior, exclusion, tags, then the
// threshold and the appends: retr_ivf_deep_topk_k's order without a cursor.  A row at or past row_hi
// reads the zero row, the zero scale, the zero tag and the zero bias: acc 0 * 0, then -inf by the
// mask and fmaf(wq, 0, -inf) = -inf.  A tile starts at row_lo + 64 i, so a list that starts at any row
// has whole 128-byte rows as DMA sources (16-byte aligned whatever row_lo is) and only its last tile
// is partial.  The plan (retr_ivf_count_k / offsets / fill), the grid bound and the merge are the
// bf16 clustered call's; retr_ivf_q8_rows_k then names every merged id's clustered row by a binary
// search of the query's probed lists (ids ascend inside a list), for the re-scoring call.
namespace lthm {
namespace {

struct RetrIvfQ8Shared {
  unsigned char img[2][RT_IT * RQ_ROWB];
  u64 sort[4][RD_CAP];  // one buffer per wave
  float tau[RT_QT];
  int cnt[RT_QT];
  int pair[RT_QT];
  int flag[3];
  alignas(16) float scl[2][RT_IT];
  alignas(16) int tag[2][RT_IT];
  alignas(16) float bias[2][RT_IT];
};
static_assert(sizeof(RetrIvfQ8Shared) <= 96 * 1024, "LDS budget: the images, four sort buffers and change");

struct RetrIvfQ8Args {
  const unsigned char* codes;  // [N, 128] e4m3fn, list-major
  const float* scale;          // [N]
  const unsigned char* cq;     // [Q, 128] the queries' codes
  const float* sq;             // [Q]
  const int64_t* row_ids;      // [N]
  const int64_t* list_off;     // [L + 1]
  const int* tile_off;         // [L + 1]; tile_off[L]: the tiles there are
  const int4* tab;             // per tile: list, first slot in pair_idx, pairs (1..64)
  const int* pair_idx;         // [Q P] pairs grouped by list
  const int* xs;               // [Q, xstride] ascending rows or null: no exclusion
  const int* tags;             // TAGS: [N]
  const int* filt;             // TAGS: [Q, 3]
  const float* bias;           // [N] or null: no prior
  const float* bw;             // [Q] or null: 1 for everyone
  float* scores;               // [P, Q, k]
  int64_t* ids;                // [P, Q, k]
  u64* keys;                   // [Q P, RD_CAP]
  int64_t Q, N;
  int L, P, k, xstride;
};

template <bool TAGS>
__global__ __launch_bounds__(256) void retr_ivf_q8_topk_k(RetrIvfQ8Args a) {
  const int blk = blockIdx.x;
  if (blk >= a.tile_off[a.L]) return;  // past the tiles there are: before LDS and the DMA
  __shared__ __attribute__((aligned(16))) RetrIvfQ8Shared sh;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5, ih = w >> 1;
  const int4 tt = a.tab[blk];
  const int c = tt.x, pbase = tt.y, np = tt.z;
  // the caller's offsets, kept inside the catalogue whatever they hold
  int64_t row_lo = a.list_off[c], row_hi = a.list_off[c + 1];
  row_lo = row_lo < 0 ? 0 : row_lo > a.N ? a.N : row_lo;
  row_hi = row_hi < row_lo ? row_lo : row_hi > a.N ? a.N : row_hi;
  const int ntile = (int)((row_hi - row_lo + RT_IT - 1) / RT_IT);
  const int ql = 32 * (w & 1) + r32;
  const bool live = ql < np;
  const int pr = live ? a.pair_idx[pbase + ql] : 0;  // < Q P
  const int64_t q = pr / a.P;
  const bool hasb = a.bias != nullptr;  // uniform

  if (tid < RT_QT) {
    // a column without a pair never passes the filter
    sh.tau[tid] = tid < np ? -INFINITY : INFINITY;
    sh.cnt[tid] = 0;
    sh.pair[tid] = tid < np ? a.pair_idx[pbase + tid] : 0;
  }
  if (tid < 3) sh.flag[tid] = 0;

  bf16x8v qf[8];
  float sq = 0.f;
  {
    const unsigned char* rp = a.cq + q * RQ_ROWB;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
      if (live) {
        lo = *reinterpret_cast<const u32x4*>(rp + 64 * s + 32 * hh);
        hi = *reinterpret_cast<const u32x4*>(rp + 64 * s + 32 * hh + 16);
      }
      retr_q8_frags(lo, qf[4 * s], qf[4 * s + 1]);
      retr_q8_frags(hi, qf[4 * s + 2], qf[4 * s + 3]);
    }
    if (live) sq = a.sq[q];
  }
  const int* xp = nullptr;
  int nx = INT_MAX;  // no list, a column without a pair: excludes nothing and reads nothing
  if (live && a.xs != nullptr) {
    const int* xl = a.xs + q * a.xstride;
    int lo = 0, hi = a.xstride - 1;  // xl[hi] = INT_MAX >= row_lo
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (xl[mid] < row_lo) lo = mid + 1;
      else hi = mid;
    }
    xp = xl + lo;
    nx = *xp;
  }
  int fm = 0, fw = 0, fy = 0;
  int yz = 1;
  if constexpr (TAGS) {
    if (live) {
      const int* fp = a.filt + q * 3;
      const int fall = fp[0], fnone = fp[2];
      fy = fp[1];
      yz = fy == 0;
      fm = (fall & fnone) ? 0 : (fall | fnone);
      fw = (fall & fnone) ? 1 : fall;
    }
  }
  float wq = 0.f;
  if (live && hasb) wq = a.bw ? a.bw[q] : 1.f;
  // the pair's key slots; a column without a pair never appends (its tau is +inf)
  u64* const kbuf = a.keys + (int64_t)pr * RD_CAP;
  int roff[4];
#pragma unroll
  for (int ch4 = 0; ch4 < 4; ++ch4) {
    const int R = 32 * ih + r32, ch = 4 * (ch4 >> 1) + 2 * hh + (ch4 & 1);
    roff[ch4] = R * RQ_ROWB + ((ch ^ ((R >> 1) & 7)) << 4);
  }

  // retr_q8_topk_k's staging: wave w stages rows 16 w .. 16 w + 15 of an image with two DMAs of 8
  // rows x 128 B; rows at or past row_hi come from the zero row
  const int srow = 16 * w + (lane >> 3), sch = (lane & 7) ^ (lane >> 4);
  auto stage = [&](int t) {
    unsigned char* img = sh.img[t & 1];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t row = row_lo + (int64_t)RT_IT * t + srow + 8 * j;
      const void* src = row < row_hi ? (const void*)(a.codes + row * RQ_ROWB + ((sch ^ (4 * j)) << 4))
                                     : (const void*)(retr_zero_row + 16 * (lane & 7));
      glds16(src, img + (16 * w + 8 * j) * RQ_ROWB);
    }
    // lane l of one wave: the word of the image's row l; never a read at or past row_hi <= N
    const int64_t wrow = row_lo + (int64_t)RT_IT * t + lane;
    if (w == 1) glds4(wrow < row_hi ? a.scale + wrow : &retr_zero_bias, sh.scl[t & 1]);
    if constexpr (TAGS) {
      if (w == 0) glds4(wrow < row_hi ? a.tags + wrow : &retr_zero_tag, sh.tag[t & 1]);
    }
    if (hasb && w == 2) glds4(wrow < row_hi ? a.bias + wrow : &retr_zero_bias, sh.bias[t & 1]);
  };
  retire_loads();
  if (ntile > 0) stage(0);
  for (int i = 0; i < ntile; ++i) {
    // the key stores of tile i - 1 count in vmcnt like the DMA: this wait retires both
    wait_vm<0>();
    __syncthreads();  // image i landed; every wave is past tile i - 1 (its image and its appends)
    if (i + 1 < ntile) stage(i + 1);
    if (tid == 0) sh.flag[(i + 1) % 3] = 0;
    if (sh.flag[(i + 2) % 3]) {  // tile i - 1 pushed a pair past the limit
      for (int pq = w; pq < np; pq += 4) {
        int n = sh.cnt[pq];
        if (n > RD_LIM) {
          n = n < RD_CAP ? n : RD_CAP;
          u64* g = a.keys + (int64_t)sh.pair[pq] * RD_CAP;
          const int m = retr_deep_prune(g, sh.sort[w], n, a.k, false, lane);
          if (lane == 0) {
            sh.cnt[pq] = m;
            if (m == a.k) sh.tau[pq] = retr_key_score(sh.sort[w][a.k - 1]);
          }
        }
      }
      __syncthreads();
    }
    const unsigned char* img = sh.img[i & 1];
    // the lane's rows are four runs of four consecutive words (broadcast reads): element 4 j + e is
    // image row 32 ih + 4 hh + 8 j + e
    float4 s4[4];
    {
      const float4* sp = reinterpret_cast<const float4*>(sh.scl[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) s4[j] = sp[2 * j];
    }
    int4 t4[4];
    if constexpr (TAGS) {
      const int4* tp = reinterpret_cast<const int4*>(sh.tag[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) t4[j] = tp[2 * j];
    }
    float4 b4[4] = {};
    if (hasb) {
      const float4* bp = reinterpret_cast<const float4*>(sh.bias[i & 1] + 32 * ih + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) b4[j] = bp[2 * j];
    }
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const u32x4 lo = *reinterpret_cast<const u32x4*>(img + roff[2 * s]);
      const u32x4 hi = *reinterpret_cast<const u32x4*>(img + roff[2 * s + 1]);
      bf16x8v af[4];
      retr_q8_frags(lo, af[0], af[1]);
      retr_q8_frags(hi, af[2], af[3]);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = mfma32(af[t], qf[4 * s + t], acc);
    }
    // the approximate score: acc (scale_q scale_j), two multiplies by powers of two
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float sj[4] = {s4[j].x, s4[j].y, s4[j].z, s4[j].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[4 * j + e] = acc[4 * j + e] * (sq * sj[e]);
    }
    // first catalogue row of this lane's elements: element v is row rb + 8 (v >> 2) + (v & 3)
    const int64_t rb = row_lo + (int64_t)RT_IT * i + 32 * ih + 4 * hh;
    if (row_lo + (int64_t)RT_IT * (i + 1) > row_hi) {  // partial tile: the rows past the list never pass
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (rb + 8 * (v >> 2) + (v & 3) >= row_hi) acc[v] = -INFINITY;
    }
    if (hasb) {
      // the ranked score from here on; a row past the list is fmaf(wq, 0, -inf) = -inf
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bw4[4] = {b4[j].x, b4[j].y, b4[j].z, b4[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * j + e] = __builtin_fmaf(wq, bw4[e], acc[4 * j + e]);
      }
    }
    {
      const int64_t tile_end = row_lo + (int64_t)RT_IT * (i + 1) < row_hi ? row_lo + (int64_t)RT_IT * (i + 1) : row_hi;
      unsigned xm = 0u;
      while (nx < tile_end) {
        const int64_t xrel = (int64_t)nx - rb;
        if (xrel >= 0 && xrel < 32 && !(xrel & 4)) xm |= 1u << (int)(((xrel >> 3) << 2) | (xrel & 3));
        nx = *++xp;
      }
      if (xm) {
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if ((xm >> v) & 1u) acc[v] = -INFINITY;
      }
    }
    if constexpr (TAGS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int tw[4] = {t4[j].x, t4[j].y, t4[j].z, t4[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool bad = ((tw[e] & fm) != fw) | (((tw[e] & fy) | yz) == 0);
          acc[4 * j + e] = bad ? -INFINITY : acc[4 * j + e];
        }
      }
    }
    float mx = acc[0];
#pragma unroll
    for (int v = 1; v < 16; ++v) mx = fmaxf(mx, acc[v]);
    const float tau = sh.tau[ql];
    if (mx >= tau) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float s = acc[v];
        if (s >= tau && s > -INFINITY) {
          const int slot = atomicAdd(&sh.cnt[ql], 1);
          if (live && slot < RD_CAP) kbuf[slot] = retr_key(s, (int)(rb + 8 * (v >> 2) + (v & 3)));
          if (slot >= RD_LIM) sh.flag[i % 3] = 1;
        }
      }
    }
  }
  wait_vm<0>();
  __syncthreads();  // the last tile's appends have left their waves
  // every pair's k best of the list, sorted, as (score, id); empty slots are (-inf, 0)
  for (int pq = w; pq < np; pq += 4) {
    int n = sh.cnt[pq];
    n = n < RD_CAP ? n : RD_CAP;
    const int pp = sh.pair[pq];
    u64* buf = sh.sort[w];
    int PS = 512;
    while (PS < n) PS <<= 1;  // n <= RD_CAP
    const u64* g = a.keys + (int64_t)pp * RD_CAP;
    for (int idx = lane; idx < PS; idx += 64) buf[idx] = idx < n ? g[idx] : 0ull;
    __builtin_amdgcn_wave_barrier();
    if (n > 1) retr_deep_sort(buf, PS, lane);
    const int m = n < a.k ? n : a.k;
    const int64_t pq_q = pp / a.P, pq_s = pp - pq_q * a.P;
    const int64_t o = (pq_s * a.Q + pq_q) * a.k;
    for (int idx = lane; idx < a.k; idx += 64) {
      const bool has = idx < m;
      const u64 key = has ? buf[idx] : 0ull;  // idx < m <= PS
      a.scores[o + idx] = has ? retr_key_score(key) : -INFINITY;
      a.ids[o + idx] = has ? a.row_ids[retr_key_row(key)] : 0;
    }
    __builtin_amdgcn_wave_barrier();  // the buffer is read before the wave's next pair refills it
  }
}

// One thread per merged entry (q, j): the clustered row of ids[q, j], found in one of the query's
// probed lists (ids ascend inside a list: a lower bound over row_ids[row_lo, row_hi) on the scan's own
// clamped offsets), -1 for an empty slot.  A merged entry came from a probed list, so it is found.
__global__ __launch_bounds__(256) void retr_ivf_q8_rows_k(const float* __restrict__ scores, const int64_t* __restrict__ ids,
                                                          const int* __restrict__ probes, int64_t Q, int P, int k, int L,
                                                          int64_t N, const int64_t* __restrict__ list_off,
                                                          const int64_t* __restrict__ row_ids, int* __restrict__ out_rows) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= Q * k) return;
  const int64_t q = e / k;
  int row = -1;
  if (retr_image(scores[e]) > RS_EMPTY) {
    const int64_t id = ids[e];
    for (int s = 0; s < P && row < 0; ++s) {
      const int c = probes[q * P + s];
      if (c < 0 || c >= L) continue;
      int64_t row_lo = list_off[c], row_hi = list_off[c + 1];
      row_lo = row_lo < 0 ? 0 : row_lo > N ? N : row_lo;
      row_hi = row_hi < row_lo ? row_lo : row_hi > N ? N : row_hi;
      int64_t lo = row_lo, hi = row_hi;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row_ids[mid] < id) lo = mid + 1;
        else hi = mid;
      }
      if (lo < row_hi && row_ids[lo] == id) row = (int)lo;
    }
  }
  out_rows[e] = row;
}

// the deep clustered layout at k = M with the key slots whatever M is, then the queries' codes and
// scales and the merged ids
struct RetrIvfQ8Ws {
  RetrIvfWs ivf;
  int64_t cq, sq, mids, total;
};
bool retr_ivf_q8_ws(int64_t Q, int64_t N, int64_t L, int64_t P, int64_t M, int64_t X, RetrIvfQ8Ws* o) {
  if (!retr_ivf_ws(Q, N, L, P, M, X, &o->ivf, false, true)) return false;
  int64_t at = o->ivf.total;
  o->cq = at, at += up256(Q * RQ_ROWB);
  o->sq = at, at += up256(Q * 4);
  o->mids = at, at += up256(Q * M * 8);
  o->total = at;
  return true;
}

}  // namespace
}  // namespace lthm

extern "C" int64_t lthm_retrieve_ivf_q8_ws_bytes(int64_t Q, int64_t N, int64_t L, int32_t P, int32_t M, int64_t X) {
  RetrIvfQ8Ws w;
  return retr_ivf_q8_ws(Q, N, L, P, M, X, &w) ? w.total : -1;
}

extern "C" int lthm_retrieve_ivf_q8_topk(const uint8_t* codes, const float* scale, int64_t N, const int64_t* row_ids,
                                         const int64_t* list_off, int64_t L, const void* q, int32_t q_dtype,
                                         int32_t normalize_q, int64_t Q, const int32_t* probes, int32_t P, int32_t M,
                                         const lthm_retrieve_excl* x, const lthm_retrieve_tags* t,
                                         const lthm_retrieve_bias* b, float* out_scores, int32_t* out_rows,
                                         void* workspace, int64_t ws_bytes, void* stream) {
  LTHM_REQUIRE(codes && scale && row_ids && list_off && q && probes && out_scores && out_rows && workspace);
  LTHM_REQUIRE(!t || (t->tags && t->filter && ((uintptr_t)t->tags & 3) == 0 && ((uintptr_t)t->filter & 3) == 0));
  LTHM_REQUIRE(!b || (b->bias && ((uintptr_t)b->bias & 3) == 0 && ((uintptr_t)b->weight & 3) == 0));
  LTHM_REQUIRE(q_dtype == LTHM_F32 || q_dtype == LTHM_BF16);
  LTHM_REQUIRE(((uintptr_t)codes & 15) == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
  LTHM_REQUIRE(((uintptr_t)scale & 3) == 0 && ((uintptr_t)row_ids & 7) == 0 && ((uintptr_t)list_off & 7) == 0 &&
               ((uintptr_t)probes & 3) == 0);
  LTHM_REQUIRE(((uintptr_t)out_scores & 3) == 0 && ((uintptr_t)out_rows & 3) == 0);
  LTHM_REQUIRE(!x || (x->rows && x->X >= 1 && x->X <= RT_XMAX && ((uintptr_t)x->rows & 3) == 0));
  RetrIvfQ8Ws wq;
  LTHM_REQUIRE(retr_ivf_q8_ws(Q, N, L, P, M, x ? x->X : 0, &wq) && ws_bytes >= wq.total);
  const RetrIvfWs& wo = wq.ivf;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  bf16_t* qn = (bf16_t*)(ws + wo.qn);
  int* cnt = (int*)(ws + wo.cnt);
  int* fill = cnt + L;
  int* pair_off = (int*)(ws + wo.off);
  int* tile_off = pair_off + (L + 1);
  int* pair_idx = (int*)(ws + wo.pidx);
  int4* tab = (int4*)(ws + wo.tab);
  float* lscores = (float*)(ws + wo.scores);
  int64_t* lids = (int64_t*)(ws + wo.ids);
  unsigned char* cq = ws + wq.cq;
  float* sq = (float*)(ws + wq.sq);
  int64_t* mids = (int64_t*)(ws + wq.mids);
  const int64_t NP = Q * P;
  // 1: the flat e4m3 call's queries: its prep, then the catalogue's quantiser on the bf16 rows
  const unsigned pgrid = (unsigned)((Q + 15) / 16);
  if (q_dtype == LTHM_BF16)
    hipLaunchKernelGGL((retr_prep_k<bf16_t>), dim3(pgrid), dim3(256), 0, s, (const bf16_t*)q, Q, normalize_q, qn,
                       (const bf16_t*)nullptr, N, (const int*)nullptr, (float*)nullptr, -INFINITY);
  else
    hipLaunchKernelGGL((retr_prep_k<float>), dim3(pgrid), dim3(256), 0, s, (const float*)q, Q, normalize_q, qn,
                       (const bf16_t*)nullptr, N, (const int*)nullptr, (float*)nullptr, -INFINITY);
  LTHM_CHECK_LAUNCH();
  hipLaunchKernelGGL(retr_q8_quant_k, dim3(pgrid), dim3(256), 0, s, (const bf16_t*)qn, Q, cq, sq);
  LTHM_CHECK_LAUNCH();
  // 2: the clustered plan
  {
    const hipError_t e = hipMemsetAsync(cnt, 0, (size_t)(2 * L) * 4, s);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned ngrid = (unsigned)((NP + 255) / 256);
  hipLaunchKernelGGL(retr_ivf_count_k, dim3(ngrid), dim3(256), 0, s, probes, NP, (int)L, (int)P, Q, (int)M, cnt, lscores,
                     lids);
  LTHM_CHECK_LAUNCH();
  hipLaunchKernelGGL(retr_ivf_offsets_k<false>, dim3(1), dim3(256), 0, s, cnt, (int)L, pair_off, tile_off, RT_QT);
  LTHM_CHECK_LAUNCH();
  hipLaunchKernelGGL(retr_ivf_fill_k<false>, dim3(ngrid), dim3(256), 0, s, probes, NP, (int)L, cnt, pair_off, tile_off,
                     fill, pair_idx, tab, RT_QT);
  LTHM_CHECK_LAUNCH();
  // 3: the scan
  RetrIvfQ8Args a;
  a.codes = codes;
  a.scale = scale;
  a.cq = cq;
  a.sq = sq;
  a.row_ids = row_ids;
  a.list_off = list_off;
  a.tile_off = tile_off;
  a.tab = tab;
  a.pair_idx = pair_idx;
  a.xs = nullptr;
  a.xstride = 0;
  a.tags = t ? t->tags : nullptr;
  a.filt = t ? t->filter : nullptr;
  a.bias = b ? b->bias : nullptr;
  a.bw = b ? b->weight : nullptr;
  a.scores = lscores;
  a.ids = lids;
  a.keys = (u64*)(ws + wo.keys);
  a.Q = Q;
  a.N = N;
  a.L = (int)L;
  a.P = P;
  a.k = M;
  if (x) {
    int* xs = (int*)(ws + wo.xs);
    const int X = (int)x->X;
    int XP = 1;
    while (XP < X) XP <<= 1;
    hipLaunchKernelGGL(retr_excl_prep_k, dim3((unsigned)Q), dim3(256), 0, s, x->rows, X, XP, N, xs);
    LTHM_CHECK_LAUNCH();
    a.xs = xs;
    a.xstride = X + 1;
  }
  const dim3 grid((unsigned)wo.grid);
  if (t) hipLaunchKernelGGL(retr_ivf_q8_topk_k<true>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(retr_ivf_q8_topk_k<false>, grid, dim3(256), 0, s, a);
  LTHM_CHECK_LAUNCH();
  // 4: the merge of every query's P lists, then the merged ids' rows
  {
    const int e = lthm_retrieve_merge_shards(lscores, lids, nullptr, P, Q, M, out_scores, mids, nullptr, stream);
    if (e) return e;
  }
  hipLaunchKernelGGL(retr_ivf_q8_rows_k, dim3((unsigned)((Q * M + 255) / 256)), dim3(256), 0, s, (const float*)out_scores,
                     (const int64_t*)mids, probes, Q, (int)P, (int)M, (int)L, N, list_off, row_ids, out_rows);
  LTHM_CHECK_LAUNCH();
  return 0;
}

