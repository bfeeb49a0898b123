// Catalogue updates: upsert and remove rows of a list-major catalogue in one merge pass
// (lthm_catalogue_update, include/lthm.h; ItemCatalogue.update / ClusteredItemCatalogue.update).
//
// Per list the surviving old ids and the delta ids are two ascending sequences without a common id, so
// the output list is their merge.  Nothing is sorted and no output is written through an atomic: every
// output row finds its one source row by binary searches, so two runs give the same bytes.
//
//   live_before[p]  the old rows before p that survive: the exclusive prefix count of dead == 0, int32
//                   [N + 1] in the workspace, summed here from the flag (cat_upd_count_k, cat_upd_tiles_k,
//                   cat_upd_prefix_k: tile sums, their scan in one block, the rows of every tile)
//   out_off[c]    = live_before[old_off[c]] + delta_off[c]
//   ddst[d]       = live_before[lower_bound(old ids of d's list, delta_ids[d])] + d, the output row of delta
//                   row d: the survivors before its list and below its id in it, plus the delta rows before it
//   output row o of list c: with j the first delta row of the list whose ddst >= o, the source is delta row
//                   j where ddst[j] == o, and else the survivor number o - j of the whole catalogue, the
//                   last old row p with live_before[p] <= o - j
//
// Three more launches: cat_upd_plan_k (out_off and the chunk table, one block), cat_upd_delta_k (ddst) and
// cat_upd_merge_k, whose blocks walk the chunk table: chunk t is CU_CHUNK consecutive output rows of one
// list, so one list of 100k rows and 4,096 lists of a few hundred rows both give the device thousands of
// chunks, and the host never reads a list length.  A chunk first resolves its rows' sources (one thread per
// row, into LDS), then moves the 8- and 4-byte columns one element per lane and the embedding rows as 16
// lanes x 16 B, so every global access of a row is one full 256 B line.
//
// ids are compared as signed int64 everywhere.  Every source index is clamped into its array and every
// output index is checked against N_out, so offsets that break the contract give wrong rows, never an
// access outside the tensors.
#include "common.hpp"

namespace lthm {

constexpr int CU_CHUNK = LTHM_CATALOGUE_UPDATE_CHUNK;  // output rows per chunk = threads per block
constexpr int CU_SCAN = 1024;                          // threads of the plan kernel
constexpr int CU_ROW_U4 = 16;                          // a bf16 [128] row as 16 x 16 B
static_assert(CU_CHUNK == 256, "a chunk is one row per thread of a 256-thread block");

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// first index in [lo, hi) whose element is >= x (hi if none); a ascending
template <typename T>
__device__ __forceinline__ int64_t lower_bound_(const T* __restrict__ a, int64_t lo, int64_t hi, T x) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// first index in [lo, hi) whose element is > x (hi if none); a ascending
template <typename T>
__device__ __forceinline__ int64_t upper_bound_(const T* __restrict__ a, int64_t lo, int64_t hi, T x) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// inclusive prefix sum of one value per thread over a block of T threads; s is T words of LDS, free
// again after the caller's next barrier
template <int T>
__device__ __forceinline__ int32_t block_incl_scan(int32_t* s, int tid, int32_t n) {
  s[tid] = n;
  __syncthreads();
  for (int d = 1; d < T; d <<= 1) {
    const int32_t v = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  return s[tid];
}

// ---- live_before from the dead flag: tiles of CU_TILE positions, CU_PER consecutive ones per thread ----
constexpr int CU_PER = 8;
constexpr int CU_TILE = 256 * CU_PER;

__device__ __forceinline__ int32_t live_of_thread(const uint8_t* __restrict__ dead, int64_t p0, int64_t N) {
  int32_t n = 0;
#pragma unroll
  for (int i = 0; i < CU_PER; ++i)
    if (p0 + i < N) n += dead[p0 + i] == 0;
  return n;
}

// tile_sum[t]: the surviving rows of tile t
__global__ __launch_bounds__(256) void cat_upd_count_k(const uint8_t* __restrict__ dead, int64_t N,
                                                        int32_t* __restrict__ tile_sum) {
  __shared__ int32_t s[256];
  const int tid = threadIdx.x;
  const int32_t n = live_of_thread(dead, (int64_t)blockIdx.x * CU_TILE + tid * CU_PER, N);
  const int32_t incl = block_incl_scan<256>(s, tid, n);
  if (tid == 255) tile_sum[blockIdx.x] = incl;
}

// the tile sums become their exclusive prefix sum, in place, in one block
__global__ __launch_bounds__(CU_SCAN) void cat_upd_tiles_k(int32_t* __restrict__ tile_sum, int64_t tiles) {
  __shared__ int32_t s[CU_SCAN];
  const int tid = threadIdx.x;
  int32_t carry = 0;
  for (int64_t base = 0; base < tiles; base += CU_SCAN) {
    const int64_t t = base + tid;
    const int32_t n = t < tiles ? tile_sum[t] : 0;
    const int32_t incl = block_incl_scan<CU_SCAN>(s, tid, n);
    if (t < tiles) tile_sum[t] = carry + incl - n;
    carry += s[CU_SCAN - 1];
    __syncthreads();
  }
}

// live_before[0..N] from the tile offsets
__global__ __launch_bounds__(256) void cat_upd_prefix_k(const uint8_t* __restrict__ dead, int64_t N,
                                                         const int32_t* __restrict__ tile_off,
                                                         int32_t* __restrict__ live_before) {
  __shared__ int32_t s[256];
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * CU_TILE + tid * CU_PER;
  const int32_t n = live_of_thread(dead, p0, N);
  int32_t run = tile_off[blockIdx.x] + block_incl_scan<256>(s, tid, n) - n;
#pragma unroll
  for (int i = 0; i < CU_PER; ++i) {
    const int64_t p = p0 + i;
    if (p <= N) live_before[p] = run;
    if (p < N) run += dead[p] == 0;
  }
}

// out_off[0..L] and chunk_off[0..L], the exclusive prefix sum of every list's chunk count
__global__ __launch_bounds__(CU_SCAN) void cat_upd_plan_k(const int64_t* __restrict__ old_off,
                                                           const int64_t* __restrict__ delta_off,
                                                           const int32_t* __restrict__ live_before, int64_t N, int64_t M,
                                                           int64_t L, int64_t* __restrict__ out_off,
                                                           int32_t* __restrict__ chunk_off) {
  __shared__ int32_t s[CU_SCAN];
  const int tid = threadIdx.x;
  int32_t carry = 0;
  for (int64_t base = 0; base <= L; base += CU_SCAN) {
    const int64_t c = base + tid;
    int32_t n = 0;
    if (c <= L) {
      const int64_t o = live_before[clamp64(old_off[c], 0, N)] + clamp64(delta_off[c], 0, M);
      out_off[c] = o;
      if (c < L) {
        const int64_t o1 = live_before[clamp64(old_off[c + 1], 0, N)] + clamp64(delta_off[c + 1], 0, M);
        n = o1 > o ? (int32_t)((o1 - o + CU_CHUNK - 1) / CU_CHUNK) : 0;
      }
    }
    const int32_t incl = block_incl_scan<CU_SCAN>(s, tid, n);
    if (c <= L) chunk_off[c] = carry + incl - n;
    carry += s[CU_SCAN - 1];
    __syncthreads();
  }
}

// ddst[d], the output row of delta row d
__global__ __launch_bounds__(256) void cat_upd_delta_k(const int64_t* __restrict__ old_ids,
                                                        const int64_t* __restrict__ old_off,
                                                        const int32_t* __restrict__ live_before,
                                                        const int64_t* __restrict__ delta_ids,
                                                        const int64_t* __restrict__ delta_off, int64_t N, int64_t M,
                                                        int64_t L, int32_t* __restrict__ ddst) {
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < M; d += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = clamp64(upper_bound_<int64_t>(delta_off, 0, L + 1, d) - 1, 0, L - 1);
    const int64_t a0 = clamp64(old_off[c], 0, N), a1 = clamp64(old_off[c + 1], a0, N);
    const int64_t p = lower_bound_<int64_t>(old_ids, a0, a1, delta_ids[d]);
    ddst[d] = (int32_t)(live_before[p] + d);
  }
}

struct CatUpdCols {
  const int64_t* old_ids;
  const u32x4* old_emb;
  const uint32_t* old_col[3];  // tags, bias, groups as 4-byte words, or NULL
  const int64_t* delta_ids;
  const u32x4* delta_emb;
  const uint32_t* delta_col[3];
  int64_t* out_ids;
  u32x4* out_emb;
  uint32_t* out_col[3];
};

__global__ __launch_bounds__(CU_CHUNK) void cat_upd_merge_k(CatUpdCols k, const int64_t* __restrict__ old_off,
                                                            const int64_t* __restrict__ delta_off,
                                                            const int32_t* __restrict__ live_before,
                                                            const int64_t* __restrict__ out_off,
                                                            const int32_t* __restrict__ chunk_off,
                                                            const int32_t* __restrict__ ddst, int64_t N, int64_t M,
                                                            int64_t L, int64_t N_out) {
  __shared__ int32_t src_s[CU_CHUNK];  // >= 0: an old row; < 0: ~(a delta row)
  const int tid = threadIdx.x;
  const int32_t nchunk = chunk_off[L];
  for (int32_t t = (int32_t)blockIdx.x; t < nchunk; t += (int32_t)gridDim.x) {
    const int64_t c = clamp64(upper_bound_<int32_t>(chunk_off, 0, L + 1, t) - 1, 0, L - 1);
    const int64_t o_list = out_off[c];
    const int64_t o0 = o_list + (int64_t)(t - chunk_off[c]) * CU_CHUNK;
    int64_t o1 = out_off[c + 1];
    if (o1 > o0 + CU_CHUNK) o1 = o0 + CU_CHUNK;
    if (o1 > N_out) o1 = N_out;
    const int rows = o0 >= 0 && o1 > o0 ? (int)(o1 - o0) : 0;
    const int64_t a0 = clamp64(old_off[c], 0, N), a1 = clamp64(old_off[c + 1], a0, N);
    const int64_t b0 = clamp64(delta_off[c], 0, M), b1 = clamp64(delta_off[c + 1], b0, M);

    // the source of output row o0 + tid
    int32_t src = 0;
    if (tid < rows) {
      const int64_t o = o0 + tid;
      const int64_t j = lower_bound_<int32_t>(ddst, b0, b1, (int32_t)o);
      if (j < b1 && ddst[j] == (int32_t)o) {
        src = ~(int32_t)j;
      } else {
        const int64_t g = o - j;  // the survivor's number in the whole catalogue
        // p >= a0 + (g - live_before[a0]): at most one survivor per row
        const int64_t lo = clamp64(a0 + (g - live_before[a0]), a0, a1);
        const int64_t p = upper_bound_<int32_t>(live_before, lo, a1 + 1, (int32_t)g) - 1;
        src = (int32_t)clamp64(p, 0, N - 1);
      }
    }
    src_s[tid] = src;

    // ids and the 4-byte columns: one element per lane
    if (tid < rows) {
      const int64_t o = o0 + tid;
      k.out_ids[o] = src < 0 ? k.delta_ids[~src] : k.old_ids[src];
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (k.out_col[i] != nullptr) k.out_col[i][o] = src < 0 ? k.delta_col[i][~src] : k.old_col[i][src];
    }
    __syncthreads();

    // embedding rows: 16 lanes x 16 B per row, 16 rows per pass, four passes in flight
    const int lane = tid & (CU_ROW_U4 - 1), slot = tid >> 4;
    constexpr int PASS = CU_CHUNK / CU_ROW_U4;  // 16 rows
    for (int r0 = 0; r0 < rows; r0 += 4 * PASS) {
      u32x4 v[4] = {};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = r0 + u * PASS + slot;
        if (r < rows) {
          const int32_t sr = src_s[r];
          v[u] = sr < 0 ? k.delta_emb[(int64_t)(~sr) * CU_ROW_U4 + lane] : k.old_emb[(int64_t)sr * CU_ROW_U4 + lane];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = r0 + u * PASS + slot;
        if (r < rows) k.out_emb[(o0 + r) * CU_ROW_U4 + lane] = v[u];
      }
    }
    __syncthreads();  // src_s is rewritten by the next chunk
  }
}

}  // namespace lthm

using namespace lthm;

static inline int64_t cu_align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
static inline bool cu_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static inline int64_t cu_tiles(int64_t N) { return (N + 1 + CU_TILE - 1) / CU_TILE; }  // positions 0..N

extern "C" int64_t lthm_catalogue_update_ws_bytes(int64_t N, int64_t M, int64_t L) {
  if (N < 1 || M < 0 || N + M > 0x7fffffffLL - 1 || L < 1 || L > (1LL << 30)) return -1;
  return cu_align256((N + 1) * 4) + cu_align256(cu_tiles(N) * 4) + cu_align256((L + 1) * 4) +
         cu_align256((M > 0 ? M : 1) * 4);
}

extern "C" int lthm_catalogue_update(const lthm_catalogue_update_desc* d, void* stream) {
  LTHM_REQUIRE(d != nullptr);
  const int64_t N = d->N, M = d->M, L = d->L, N_out = d->N_out;
  LTHM_REQUIRE(N >= 1 && N <= 0x7fffffffLL - 1 && M >= 0 && L >= 1 && N_out >= 1 && N_out <= N + M &&
               N + M <= 0x7fffffffLL - 1);
  const int64_t need = lthm_catalogue_update_ws_bytes(N, M, L);
  LTHM_REQUIRE(need > 0 && d->workspace != nullptr && d->ws_bytes >= need && cu_aligned(d->workspace, 16));
  LTHM_REQUIRE(d->old_ids && d->old_emb && d->old_off && d->dead && d->delta_off);
  LTHM_REQUIRE(d->out_ids && d->out_emb && d->out_off);
  LTHM_REQUIRE(M == 0 || (d->delta_ids && d->delta_emb));
  LTHM_REQUIRE(cu_aligned(d->old_emb, 16) && cu_aligned(d->delta_emb, 16) && cu_aligned(d->out_emb, 16));
  const void* old_c[3] = {d->old_tags, d->old_bias, d->old_groups};
  const void* del_c[3] = {d->delta_tags, d->delta_bias, d->delta_groups};
  void* out_c[3] = {d->out_tags, d->out_bias, d->out_groups};
  CatUpdCols k;
  for (int i = 0; i < 3; ++i) {  // a column is carried by the old rows, the delta and the output, or by none
    LTHM_REQUIRE((old_c[i] != nullptr) == (out_c[i] != nullptr));
    LTHM_REQUIRE(M == 0 || (old_c[i] != nullptr) == (del_c[i] != nullptr));
    k.old_col[i] = (const uint32_t*)old_c[i];
    k.delta_col[i] = (const uint32_t*)del_c[i];
    k.out_col[i] = (uint32_t*)out_c[i];
  }
  k.old_ids = d->old_ids;
  k.old_emb = (const u32x4*)d->old_emb;
  k.delta_ids = d->delta_ids;
  k.delta_emb = (const u32x4*)d->delta_emb;
  k.out_ids = d->out_ids;
  k.out_emb = (u32x4*)d->out_emb;
  const int64_t tiles = cu_tiles(N);
  char* ws = (char*)d->workspace;
  int32_t* live_before = (int32_t*)ws;
  int32_t* tile_off = (int32_t*)(ws += cu_align256((N + 1) * 4));
  int32_t* chunk_off = (int32_t*)(ws += cu_align256(tiles * 4));
  int32_t* ddst = (int32_t*)(ws += cu_align256((L + 1) * 4));
  hipStream_t st = (hipStream_t)stream;

  hipLaunchKernelGGL(cat_upd_count_k, dim3((unsigned)tiles), dim3(256), 0, st, d->dead, N, tile_off);
  LTHM_CHECK_LAUNCH();
  hipLaunchKernelGGL(cat_upd_tiles_k, dim3(1), dim3(CU_SCAN), 0, st, tile_off, tiles);
  LTHM_CHECK_LAUNCH();
  hipLaunchKernelGGL(cat_upd_prefix_k, dim3((unsigned)tiles), dim3(256), 0, st, d->dead, N, tile_off, live_before);
  LTHM_CHECK_LAUNCH();

  hipLaunchKernelGGL(cat_upd_plan_k, dim3(1), dim3(CU_SCAN), 0, st, d->old_off, d->delta_off, live_before, N, M, L,
                     d->out_off, chunk_off);
  LTHM_CHECK_LAUNCH();
  if (M > 0) {
    hipLaunchKernelGGL(cat_upd_delta_k, dim3(grid_for(M, 256)), dim3(256), 0, st, d->old_ids, d->old_off,
                       live_before, d->delta_ids, d->delta_off, N, M, L, ddst);
    LTHM_CHECK_LAUNCH();
  }
  // at most N_out / CU_CHUNK + L chunks; the blocks read the true count from the table
  const int64_t most = N_out / CU_CHUNK + L;
  hipLaunchKernelGGL(cat_upd_merge_k, dim3(grid_for(most, 1, cu_count() * 8)), dim3(CU_CHUNK), 0, st, k, d->old_off,
                     d->delta_off, live_before, d->out_off, chunk_off, ddst, N, M, L, N_out);
  LTHM_CHECK_LAUNCH();
  return 0;
}
