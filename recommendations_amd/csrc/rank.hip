// Ranking stage around the ranker's forward (RankerModelWrapper.rank): the batch that the forward
// reads is assembled from (user rows, candidate lists), and the logits it returns are sorted per list
// (lthm_rank_assemble, lthm_rank_sort, include/lthm.h).  Neither kernel computes a logit: the values
// that reach the forward are exact copies, and the values that leave the sort are the forward's own.
//
// rank_assemble_k: output row q M + m = [query q's user columns | the item columns of rows[q, m]], for
// the dense f32 matrix and the int64 categorical matrix in one pass.  A row is cut into units and a
// thread moves one unit from its one source to its one place, so every output element is written
// once; consecutive lanes take consecutive units of a row, so a wave reads and writes whole rows.
// The unit is 16 bytes where both widths of a matrix allow it (Du and Di multiples of 4, Fu and Fi
// multiples of 2: every row segment then starts on a 16-byte boundary), and one element (4 / 8 bytes)
// otherwise: odd widths take the scalar path, they are not refused.  A row index outside [0, N) is a
// pad: it is never followed, and the item units of its row are written as zeros.  Element offsets are
// 64-bit; the row number q M + m itself stays below 2^31 (checked by the entry).
//
// rank_sort_k: one block per list, one thread per entry, the keys in LDS.  An entry travels as the
// 64-bit key of retrieve.hip, with the list position as the tie-break:
//   key = image(logit) << 32 | ~row      for a candidate (row >= 0 and the logit not NaN)
//   key = 0                              for everything else (pads, NaN, the slots behind M)
// image() is the order-preserving integer image of an f32 (logit + 0.f first, so -0.0 and +0.0 get one
// image; -inf and +inf are ordinary values with the smallest and the largest image), and ~row puts
// the lower row first among equal logits.  No candidate has the key 0: ~row >= 2^31 for a row >= 0.
// "a precedes b" in the total order (logit descending, row ascending, src ascending) is
//   key_a > key_b, or key_a == key_b and src_a < src_b,
// and an entry's rank is the number of entries that precede it: a permutation of 0..P-1 over the
// padded list, with every candidate ahead of every non-candidate.  So the thread of rank r < k writes
// slot r, each slot of the list is written exactly once (an empty one as (-inf, -1, -1)), and nothing
// depends on how the waves of the block were scheduled.  The ranks go through LDS, so that the three
// outputs leave as consecutive lanes' stores.  No global scratch, no atomics.  The score written is
// the logit as it came in (a -0.0 stays -0.0: it compares equal to +0.0).
#include "common.hpp"

#include <climits>
#include <cmath>

namespace lthm {
namespace {

typedef unsigned long long u64;

constexpr int RK_MAX = LTHM_RANK_MAX_LIST;  // longest list
constexpr int RA_THREADS = 256;
constexpr int RA_ROWS = 16;  // output rows per tile of the assemble kernel
static_assert(RK_MAX == 1024, "one thread per entry of a list, 1,024 threads per block at most");

struct RankAsmArgs {
  const void* user_dense;  // [Q, Du] f32
  const void* user_cat;    // [Q, Fu] int64
  const void* item_dense;  // [N, Di] f32
  const void* item_cat;    // [N, Fi] int64
  const int* rows;         // [Q, M]
  void* out_dense;         // [Q M, Du + Di]
  void* out_cat;           // [Q M, Fu + Fi]
  uint32_t du, di, fu, fi;  // the four widths in units of their matrix
  uint32_t M, N;
  uint32_t total;  // Q M
};

// UD, UC: the unit of the dense and of the categorical matrix
template <typename UD, typename UC>
__global__ __launch_bounds__(RA_THREADS) void rank_assemble_k(RankAsmArgs a) {
  const UD* __restrict__ ud = (const UD*)a.user_dense;
  const UD* __restrict__ id = (const UD*)a.item_dense;
  const UC* __restrict__ uc = (const UC*)a.user_cat;
  const UC* __restrict__ ic = (const UC*)a.item_cat;
  UD* __restrict__ od = (UD*)a.out_dense;
  UC* __restrict__ oc = (UC*)a.out_cat;
  const uint32_t wd = a.du + a.di, wc = a.fu + a.fi, W = wd + wc;  // units of one output row
  const uint32_t ntile = (a.total + RA_ROWS - 1) / RA_ROWS;
  for (uint32_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint32_t row0 = tile * RA_ROWS;
    const uint32_t nrow = a.total - row0 < (uint32_t)RA_ROWS ? a.total - row0 : (uint32_t)RA_ROWS;
    for (uint32_t u = threadIdx.x; u < nrow * W; u += RA_THREADS) {
      const uint32_t r = u / W;
      uint32_t c = u - r * W;
      const uint32_t row = row0 + r;  // < total
      const uint32_t q = row / a.M;
      if (c < a.du) {
        od[(int64_t)row * wd + c] = ud[(int64_t)q * a.du + c];
      } else if (c < wd) {
        const uint32_t idx = (uint32_t)a.rows[row];  // a pad (negative or >= N) is never followed
        UD v = {};
        if (idx < a.N) v = id[(int64_t)idx * a.di + (c - a.du)];
        od[(int64_t)row * wd + c] = v;
      } else if ((c -= wd) < a.fu) {
        oc[(int64_t)row * wc + c] = uc[(int64_t)q * a.fu + c];
      } else {
        const uint32_t idx = (uint32_t)a.rows[row];
        UC v = {};
        if (idx < a.N) v = ic[(int64_t)idx * a.fi + (c - a.fu)];
        oc[(int64_t)row * wc + c] = v;
      }
    }
  }
}

// the order-preserving integer image of a logit (retrieve.hip retr_image)
__device__ __forceinline__ uint32_t rank_image(float s) {
  uint32_t u = __float_as_uint(s + 0.f);  // -0 -> +0: equal logits get equal images
  u ^= (uint32_t)((int32_t)u >> 31) | 0x80000000u;
  return u;
}

// blockDim.x = P, the next power of two of M (64 at least); grid = Q
__global__ __launch_bounds__(RK_MAX) void rank_sort_k(const float* __restrict__ logits, const int* __restrict__ rows,
                                                       int M, int k, float* __restrict__ out_scores,
                                                       int* __restrict__ out_rows, int* __restrict__ out_src) {
  __shared__ __attribute__((aligned(16))) u64 key_s[RK_MAX];
  __shared__ float score_s[RK_MAX];
  __shared__ int row_s[RK_MAX];
  __shared__ int src_s[RK_MAX];
  const int tid = threadIdx.x;
  const int64_t in0 = (int64_t)blockIdx.x * M;
  float s = 0.f;
  int row = -1;
  u64 key = 0ull;
  if (tid < M) {
    s = logits[in0 + tid];
    row = rows[in0 + tid];
    if (row >= 0 && s == s) key = ((u64)rank_image(s) << 32) | (uint32_t)~row;
  }
  key_s[tid] = key;  // tid < P <= RK_MAX; the slots in M..P-1 hold 0
  __syncthreads();
  if (tid < M) {
    // the entries that precede this one; a slot j >= M holds the key 0 and j > tid, so it never counts
    // and the loop may run over whole groups of 8 (M8 <= P: P is a multiple of 64)
    const int M8 = (M + 7) & ~7;
    int rk = 0;
#pragma unroll 8
    for (int j = 0; j < M8; ++j) {
      const u64 kj = key_s[j];  // one address for the whole wave: a broadcast read
      rk += (kj > key ? 1 : 0) + (((kj == key) & (j < tid)) ? 1 : 0);
    }
    if (rk < k) {  // rk < M <= RK_MAX
      const bool cand = key != 0ull;
      score_s[rk] = cand ? s : -INFINITY;
      row_s[rk] = cand ? row : -1;
      src_s[rk] = cand ? tid : -1;
    }
  }
  __syncthreads();
  if (tid < k) {  // the ranks of the M entries are 0..M-1, k <= M: every slot below k was written
    const int64_t o = (int64_t)blockIdx.x * k + tid;
    out_scores[o] = score_s[tid];
    out_rows[o] = row_s[tid];
    out_src[o] = src_s[tid];
  }
}

inline bool rk_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace
}  // namespace lthm

using namespace lthm;

extern "C" int lthm_rank_assemble(const lthm_rank_assemble_desc* d, void* stream) {
  LTHM_REQUIRE(d != nullptr);
  const int64_t Q = d->Q, M = d->M, N = d->N, Du = d->Du, Di = d->Di, Fu = d->Fu, Fi = d->Fi;
  LTHM_REQUIRE(Q >= 1 && M >= 1 && M <= RK_MAX && Q * M <= INT_MAX && N >= 0 && N <= INT_MAX);
  LTHM_REQUIRE(Du >= 0 && Di >= 0 && Fu >= 0 && Fi >= 0);
  LTHM_REQUIRE(Du + Di <= (1 << 20) && Fu + Fi <= (1 << 20));
  LTHM_REQUIRE(d->rows != nullptr && rk_aligned(d->rows, 4));
  // a matrix of width 0 has no elements: its pointer is not read and may be NULL
  LTHM_REQUIRE(Du == 0 || d->user_dense != nullptr);
  LTHM_REQUIRE(Fu == 0 || d->user_cat != nullptr);
  LTHM_REQUIRE(Di == 0 || N == 0 || d->item_dense != nullptr);
  LTHM_REQUIRE(Fi == 0 || N == 0 || d->item_cat != nullptr);
  LTHM_REQUIRE(Du + Di == 0 || d->out_dense != nullptr);
  LTHM_REQUIRE(Fu + Fi == 0 || d->out_cat != nullptr);
  // 16-byte units where both widths of a matrix allow them, and then 16-byte aligned pointers
  const bool dv = Du % 4 == 0 && Di % 4 == 0, cv = Fu % 2 == 0 && Fi % 2 == 0;
  const uintptr_t da = dv ? 16 : 4, ca = cv ? 16 : 8;
  LTHM_REQUIRE(rk_aligned(d->user_dense, da) && rk_aligned(d->item_dense, da) && rk_aligned(d->out_dense, da));
  LTHM_REQUIRE(rk_aligned(d->user_cat, ca) && rk_aligned(d->item_cat, ca) && rk_aligned(d->out_cat, ca));
  if (Du + Di + Fu + Fi == 0) return 0;
  RankAsmArgs a;
  a.user_dense = d->user_dense;
  a.user_cat = d->user_cat;
  a.item_dense = d->item_dense;
  a.item_cat = d->item_cat;
  a.rows = d->rows;
  a.out_dense = d->out_dense;
  a.out_cat = d->out_cat;
  a.du = (uint32_t)(dv ? Du / 4 : Du);
  a.di = (uint32_t)(dv ? Di / 4 : Di);
  a.fu = (uint32_t)(cv ? Fu / 2 : Fu);
  a.fi = (uint32_t)(cv ? Fi / 2 : Fi);
  a.M = (uint32_t)M;
  a.N = (uint32_t)N;
  a.total = (uint32_t)(Q * M);
  // RA_ROWS (du + di + fu + fi) <= 2^25: the unit number inside a tile fits 32 bits
  const dim3 grid(grid_for(Q * M, RA_ROWS, cu_count() * 16)), block(RA_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (dv && cv) hipLaunchKernelGGL((rank_assemble_k<u32x4, u32x4>), grid, block, 0, st, a);
  else if (dv) hipLaunchKernelGGL((rank_assemble_k<u32x4, u64>), grid, block, 0, st, a);
  else if (cv) hipLaunchKernelGGL((rank_assemble_k<uint32_t, u32x4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((rank_assemble_k<uint32_t, u64>), grid, block, 0, st, a);
  LTHM_CHECK_LAUNCH();
  return 0;
}

extern "C" int lthm_rank_sort(const float* logits, const int32_t* rows, int64_t Q, int32_t M, int32_t k,
                              float* out_scores, int32_t* out_rows, int32_t* out_src, void* stream) {
  LTHM_REQUIRE(logits != nullptr && rows != nullptr && out_scores != nullptr && out_rows != nullptr &&
               out_src != nullptr);
  LTHM_REQUIRE(rk_aligned(logits, 4) && rk_aligned(rows, 4) && rk_aligned(out_scores, 4) &&
               rk_aligned(out_rows, 4) && rk_aligned(out_src, 4));
  LTHM_REQUIRE(Q >= 1 && Q <= INT_MAX && M >= 1 && M <= RK_MAX && k >= 1 && k <= M);
  int P = 64;
  while (P < M) P <<= 1;
  hipLaunchKernelGGL(rank_sort_k, dim3((unsigned)Q), dim3(P), 0, (hipStream_t)stream, logits, rows, (int)M, (int)k,
                     out_scores, out_rows, out_src);
  LTHM_CHECK_LAUNCH();
  return 0;
}
