// Fused encoder MLP for gfx950: _MLP (commons/transformers/layers.py:279-284)
//
//   out = res1 [+ res2] + c_proj( GELU( c_fc(x) ) )      x = ln_2 output, bf16
//
// with the [M, 4d] hidden never written to HBM.  The forward keeps it in
// registers; the backward recomputes it (two kernels, below).  All three kernels
// share one structure:
//
//  * v_mfma_f32_32x32x16_bf16 throughout; a wave owns 32 token rows (dX-style
//    kernels) or 32 hidden units (the weight-gradient kernel);
//  * the hidden dimension is walked in chunks of 32 units.  A chunk's first
//    product is computed TRANSPOSED (pre^T = W1_j . x^T: hidden on the
//    accumulator's registers, token rows on its lanes), so the accumulator,
//    packed to bf16, is directly the A operand of the second product, which sums
//    over the hidden index (cdna_hip_programming.md §3, accumulator as operand):
//    no LDS round trip, no transpose;
//  * the weights stream through LDS in [32 x d] chunk images (c_fc.weight rows
//    and c_proj.weight^T rows, both contiguous 32 x d blocks), double-buffered
//    by LDS-DMA (global_load_lds_dwordx4), one barrier per chunk.  The same
//    image serves row reads (ds_read_b128: the chunk as an A operand over d) and
//    transposed reads (ds_read_b64_tr_b16: the chunk as a B operand over the
//    permuted hidden index of the packed accumulator); the XOR swizzle
//    ch ^ ((r & 3) << 2 | (r >> 2) & 3) makes both conflict-free.
//
// Per token row and layer the forward moves x (2d B), res1 (4d B) and out (4d B)
// instead of the unfused chain's 4d-wide bf16 hidden + GELU' aux writes and their
// re-reads (2 x 2 x 4d B written, read twice more in the backward).
#include <algorithm>

#include "mfma.hpp"

namespace lthm {

struct MlpArgs {
  const bf16_t* X;    // [M, D] ln_2 output (bf16)
  const bf16_t* W1;   // [HID, D] c_fc.weight (bf16)
  const bf16_t* W2T;  // [HID, D] c_proj.weight^T (bf16)
  const float* b1;    // [HID] or null
  const float* b2;    // [D] or null
  const float* res1;  // [M, D] f32 or null
  const float* res2;  // [M, D] f32 or null
  float* out;         // [M, D] f32
  int64_t M;
  int HID;
  int ntiles;
  // ln_2 fused in the prologue (ln_w non-null): X is unused, the input rows are LN(x32)
  const float* x32;   // [M, D] f32 (the block's x1; usually also res1)
  const float* ln_w;  // [D]
  const float* ln_b;  // [D] or null
  bf16_t* h_out;      // [M, D] bf16: the LN output, saved for the backward (or null)
  float* mean;        // [M] (or null)
  float* rstd;        // [M] (or null)
};

struct MlpBwdArgs {
  const bf16_t* X;    // [M, D] ln_2 output (bf16)
  const bf16_t* dY;   // [M, D] gradient of the MLP output (bf16)
  const bf16_t* W1;   // [HID, D] c_fc.weight (bf16)
  const bf16_t* W2T;  // [HID, D] c_proj.weight^T (bf16)
  const float* b1;    // [HID] or null
  bf16_t* G;          // [M, HID] GELU(pre) (bf16)
  bf16_t* dP;         // [M, HID] d pre (bf16)
  float* dXf;         // [M, D] dX (f32), or
  bf16_t* dXb;        // [M, D] dX (bf16)
  int dx_f32;
  int64_t M;
  int HID;
};

// The weight-gradient kernel (mlp_wgrad_k): per (token slice, hidden group) partial slabs
struct MlpWgArgs {
  const bf16_t* X;    // [M, D] ln_2 output (bf16)
  const bf16_t* dY;   // [M, D] gradient of the MLP output (bf16)
  const bf16_t* W1;   // [HID, D] c_fc.weight (bf16)
  const bf16_t* W2T;  // [HID, D] c_proj.weight^T (bf16)
  const float* b1;    // [HID] or null
  float* dW1p;        // [nslice][HID][D] partial dW1 = dpre^T x
  float* dW2Tp;       // [nslice][HID][D] partial dW2^T = g^T dy
  float* db1p;        // [nslice][HID] partial colsum dpre (or null)
  int64_t M;
  int HID;
  int nslice;         // token slices
  int ngroup;         // hidden groups (HID / (32 NW))
};

// [rows][D] bf16 images as 8-row x 32-column subtiles of 512 B (cdna_hip_programming.md T10,
// layout (a)): byte offset of 16-B chunk c (8 columns) of row r.  Every offset is a per-lane
// base plus a multiple of 512 in the chunk's high bits, so an unrolled loop over k-steps or
// output tiles needs two base registers, not one per read.  Conflict-free for the 32x32x16
// row reads (ds_read_b128) and the transposed reads (ds_read_b64_tr_b16) alike.
template <int D>
__device__ __forceinline__ int mlp_off(int r, int c) {
  return (16 * D) * (r >> 3) + 512 * (c >> 2) + 64 * (r & 7) + 16 * ((c & 3) ^ ((r >> 2) & 3));
}

// LDS-DMA of a [32 x D] bf16 block (rows contiguous, row stride D) into a mlp_off image:
// the DMA writes 16-B slot base + lane of each wave-instruction, so the layout is applied
// to the source address (slot -> row, chunk by inverting mlp_off).
template <int D, int NTH>
__device__ __forceinline__ void mlp_dma32(unsigned char* img, const bf16_t* P, int tid) {
  constexpr int SLOTS = 32 * D / 8;
  static_assert(SLOTS % NTH == 0, "image slots must divide over the workgroup");
  const int wbase = tid & ~63;
#pragma unroll
  for (int m = 0; m < SLOTS / NTH; ++m) {
    const int o = (m * NTH + tid) * 16;
    const int r1 = o % (16 * D);
    const int r = 8 * (o / (16 * D)) + (r1 % 512) / 64;
    const int c = 4 * (r1 / 512) + (((r1 % 64) / 16) ^ ((r >> 2) & 3));
    glds16(P + (int64_t)r * D + c * 8, img + (m * NTH + wbase) * 16);
  }
}

// mlp_dma32 of the rows row0 .. row0 + 31 of a [M, D] tensor, rows past nvalid read as row
// row0 + nvalid - 1 (in bounds; the kernel zeroes their contributions)
template <int D, int NTH>
__device__ __forceinline__ void mlp_dma32c(unsigned char* img, const bf16_t* P, int64_t row0, int nvalid, int tid) {
  constexpr int SLOTS = 32 * D / 8;
  static_assert(SLOTS % NTH == 0, "image slots must divide over the workgroup");
  const int wbase = tid & ~63;
#pragma unroll
  for (int m = 0; m < SLOTS / NTH; ++m) {
    const int o = (m * NTH + tid) * 16;
    const int r1 = o % (16 * D);
    const int r = 8 * (o / (16 * D)) + (r1 % 512) / 64;
    const int c = 4 * (r1 / 512) + (((r1 % 64) / 16) ^ ((r >> 2) & 3));
    glds16(P + (row0 + min(r, nvalid - 1)) * D + c * 8, img + (m * NTH + wbase) * 16);
  }
}

// mlp_dma32 with the per-thread source offsets precomputed (MlpDmaPlan) and the destination given
// as an LDS byte address: per piece one 64-bit add and the DMA
template <int D, int NTH>
struct MlpDmaPlan {
  static constexpr int PIECES = 32 * D / 8 / NTH;
  int off[PIECES];  // element offset of piece m's 16 source bytes within a [32 x D] block
  __device__ __forceinline__ void init(int tid) {
#pragma unroll
    for (int m = 0; m < PIECES; ++m) {
      const int o = (m * NTH + tid) * 16;
      const int r1 = o % (16 * D);
      const int r = 8 * (o / (16 * D)) + (r1 % 512) / 64;
      const int c = 4 * (r1 / 512) + (((r1 % 64) / 16) ^ ((r >> 2) & 3));
      off[m] = r * D + c * 8;
    }
  }
  // block P (32 rows of D, row stride D) into the image at LDS byte address lds (wave-uniform base
  // of the image + the wave's 1-KiB slice: lds_img + (tid & ~63) * 16)
  __device__ __forceinline__ void issue(const bf16_t* P, uint32_t lds_wave) const {
#pragma unroll
    for (int m = 0; m < PIECES; ++m) glds16_m0(P + off[m], lds_wave + m * NTH * 16);
  }
};

// A operand of 32x32x16 from a [32][D] image: lane (r = l & 31, h = l >> 5) row r, k 16 ks + 8 h ..
template <int D>
__device__ __forceinline__ bf16x8v mlp_row_frag(const unsigned char* img, int lane, int ks) {
  return frag_at(img + mlp_off<D>(lane & 31, 2 * ks + (lane >> 5)));
}

// B operand of 32x32x16 over the PERMUTED k order of a packed accumulator (k-step s2 of a
// 32-row block of the image, output columns 32 t ..): element e of lane half h is image row
// 16 s2 + 8 (e >> 2) + 4 h + (e & 3), column 32 t + (lane & 31) -- two transposed reads.
template <int D>
__device__ __forceinline__ bf16x8v mlp_tr_frag(const unsigned char* img, int lane, int s2, int t) {
  const int h = lane >> 5, q = (lane >> 2) & 3, p = lane & 3, g1 = (lane >> 4) & 1;
  const int c = 4 * t + 2 * g1 + (p >> 1);
  const int r0 = 16 * s2 + 4 * h + q;
  return tr_frag(tr_half(img + mlp_off<D>(r0, c) + 8 * (p & 1)), tr_half(img + mlp_off<D>(r0 + 8, c) + 8 * (p & 1)));
}

// ---------------------------------------------------------------- forward
// Workgroup = NW waves, persistent over a contiguous range of token rows, in tiles of 32 NW
// rows (a wave owns 32).  The hidden chunks of consecutive tiles form ONE stream c = 0, 1, ...
// (chunk c % NC of the WG's tile c / NC); step c of the software pipeline is
//   S'  = W1_{c+1} . x^T            phase 1 of the NEXT chunk (A: W1 image rows; B: x in registers)
//   Hp  = bf16(GELU(S + b1_c))      issued between those MFMAs (independent VALU)
//   Y  += Hp . W2T_c                phase 2 of this chunk (B: W2T image, transposed reads)
// W1 and W2T images ride separate 2-slot rings: step c consumes W2T_c and W1_{c+1} and its
// LDS-DMAs fetch W2T_{c+1} and W1_{c+2} into the slots step c - 1 released; one barrier per
// step.  The residual (+ b2) is loaded INTO the accumulator when a tile starts, so the
// epilogue only stores (LDS-restaged 16-B rows, no load after a store on the in-order vmcnt);
// the next tile's x rows are loaded one step before the tile's last phase 1 needs them.
// out[row, :] = acc + b2 + res1 [+ res2] for the wave's rows rb .. min(rb + 32, lim): each
// 32-column tile t of the accumulator goes through the wave's 4-KiB LDS strip (C layout in,
// 128-B rows out), then every lane finishes four 16-B pieces with vector loads / stores; the
// residual pieces of tile t are loaded before the tile is restaged.
template <int D, int NT, int NRES>
__device__ __forceinline__ void mlp_fwd_epi(const MlpArgs& a, const f32x16 (&acc)[NT], const float* b2s,
                                            float* stg, int64_t rb, int64_t lim, int lane) {
  const int r32 = lane & 31, h = lane >> 5;
  const int pr = lane >> 3, pc = 4 * (lane & 7);  // piece m: row pr + 8 m, columns pc .. pc + 3
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4 rv[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {  // in flight while the tile is restaged
      const int64_t o = min(rb + pr + 8 * m, lim - 1) * D + 32 * t + pc;
      rv[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (NRES >= 1) rv[m] = *reinterpret_cast<const f32x4*>(a.res1 + o);
      if constexpr (NRES >= 2) rv[m] += *reinterpret_cast<const f32x4*>(a.res2 + o);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) stg[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r32] = acc[t][i];
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    const f32x4 bias = *reinterpret_cast<const f32x4*>(b2s + 32 * t + pc);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int64_t row = rb + pr + 8 * m;
      f32x4 v = *reinterpret_cast<const f32x4*>(stg + (pr + 8 * m) * 32 + pc);
      v += bias + rv[m];
      if (row < lim) *reinterpret_cast<f32x4*>(a.out + row * D + 32 * t + pc) = v;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
  }
}

template <int D, int KS>
__device__ __forceinline__ void mlp_load_x(const bf16_t* X, int64_t row, bool ok, int h, bf16x8v (&xf)[KS]) {
  const bf16_t* p = X + (ok ? row : 0) * D + 8 * h;
#pragma unroll
  for (int s = 0; s < KS; ++s)
    xf[s] = __builtin_bit_cast(bf16x8v, ok ? *reinterpret_cast<const u32x4*>(p + 16 * s) : u32x4{0u, 0u, 0u, 0u});
}

// ln_2 in the prologue: lane (row r, half h) holds columns 16 s + 8 h .. + 7 of its row (the B
// operand layout); the row's statistics combine the two halves through one lane exchange.
// Same two-pass arithmetic as ln_fwd_v4_k (mean, then the mean squared deviation, eps 1e-5).
template <int D, int KS>
__device__ __forceinline__ void mlp_ld8f(const float* p, bool ok, float (&v)[8]) {
  const f32x4 lo = ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 hi = ok ? *reinterpret_cast<const f32x4*>(p + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}
// ln_2 in the prologue: lane (row r, half h) holds columns 16 s + 8 h .. + 7 of its row (the B
// operand layout); the row's statistics combine the two halves through one lane exchange.
// Same two-pass arithmetic as ln_fwd_v4_k (mean, then the mean squared deviation, eps 1e-5);
// the lane's half-row is streamed three times (sum, deviations, normalise: L1 / L2 hits after
// the first) instead of held in 128 registers.
template <int D, int KS>
__device__ __forceinline__ void mlp_load_ln(const MlpArgs& a, const float* lw, const float* lb, int64_t row, bool ok,
                                            int h, bf16x8v (&xf)[KS]) {
  const float* p = a.x32 + (ok ? row : 0) * D + 8 * h;
  float s = 0.f;
#pragma unroll 4
  for (int k = 0; k < KS; ++k) {
    float v[8];
    mlp_ld8f<D, KS>(p + 16 * k, ok, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
  }
  s += __shfl_xor(s, 32, 64);
  const float mu = s / (float)D;
  float q = 0.f;
#pragma unroll 4
  for (int k = 0; k < KS; ++k) {
    float v[8];
    mlp_ld8f<D, KS>(p + 16 * k, ok, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float dd = v[e] - mu;
      q += dd * dd;
    }
  }
  q += __shfl_xor(q, 32, 64);
  const float rs = 1.f / sqrtf(q / (float)D + 1e-5f);
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    float v[8], y[8];
    mlp_ld8f<D, KS>(p + 16 * k, ok, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = 16 * k + 8 * h + e;
      y[e] = (v[e] - mu) * rs * lw[c] + (lb ? lb[c] : 0.f);
    }
    u32x4 w4;
#pragma unroll
    for (int i = 0; i < 4; ++i) w4[i] = pack_bf16x2(y[2 * i], y[2 * i + 1]);
    xf[k] = __builtin_bit_cast(bf16x8v, w4);
    if (ok && a.h_out) *reinterpret_cast<u32x4*>(a.h_out + row * D + 16 * k + 8 * h) = w4;
  }
  if (ok && h == 0) {
    if (a.mean) a.mean[row] = mu;
    if (a.rstd) a.rstd[row] = rs;
  }
}

// Weight chunks ride a 3-slot LDS-DMA ring that prefetches two chunks ahead.
template <int D, int NW>
__global__ __launch_bounds__(64 * NW, 1) void mlp_fwd_k(MlpArgs a) {
  constexpr int NS = 3, DIST = 2;
  constexpr int NTH = 64 * NW, IMG = 32 * D * 2, KS = D / 16, NT = D / 32, TR = 32 * NW;
  constexpr int DPC = 2 * (32 * D / 8) / NTH;  // DMAs per thread and chunk (both images)
  __shared__ __attribute__((aligned(16))) unsigned char img[NS][2][IMG];  // [slot][W1_j, W2T_j]
  __shared__ __attribute__((aligned(16))) float stg_all[NW][32 * 32];    // per-wave epilogue strips
  extern __shared__ float b1s[];                                         // [HID] b1, [D] b2, [D] ln w, [D] ln b
  float* b2s = b1s + a.HID;
  float* lws = b2s + D;
  float* lbs = lws + D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int NC = a.HID / 32;
  const int64_t rs = a.M * blockIdx.x / gridDim.x, re = a.M * (blockIdx.x + 1) / gridDim.x;
  if (rs >= re) return;  // uniform
  for (int i = tid; i < a.HID; i += NTH) b1s[i] = a.b1 ? a.b1[i] : 0.f;
  for (int i = tid; i < D; i += NTH) b2s[i] = a.b2 ? a.b2[i] : 0.f;
  if (a.ln_w)
    for (int i = tid; i < D; i += NTH) {
      lws[i] = a.ln_w[i];
      lbs[i] = a.ln_b ? a.ln_b[i] : 0.f;
    }
  float* stg = stg_all[wave];
  retire_loads();
  const int64_t ntile_wg = (re - rs + TR - 1) / TR;
  // chunks 0 .. DIST - 1 of the stream (chunk c: index c % NC of tile c / NC)
#pragma unroll
  for (int c = 0; c < DIST; ++c)
    if (c / NC < ntile_wg) {
      mlp_dma32<D, NTH>(img[c][0], a.W1 + (int64_t)(c % NC) * 32 * D, tid);
      mlp_dma32<D, NTH>(img[c][1], a.W2T + (int64_t)(c % NC) * 32 * D, tid);
    }
  __syncthreads();  // b1s / b2s / ln
  // S^T = W1_j . x^T (hidden units of chunk j on the registers, the token on the lane)
  auto s_phase = [&](const unsigned char* w1, const bf16x8v(&xf)[KS]) {
    // LDS reads one step ahead of their MFMA; the compiler fences keep the unrolled loops
    // from hoisting every read (register pressure: 2 waves per SIMD)
    f32x16 S = f32x16{};
    bf16x8v fa = mlp_row_frag<D>(w1, lane, 0);
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const bf16x8v fn = mlp_row_frag<D>(w1, lane, k + 1 < KS ? k + 1 : k);
      S = mfma32(fa, xf[k], S);
      fa = fn;
      asm volatile("" ::: "memory");
    }
    return S;
  };
  // H = bf16(GELU(S + b1_j)), Y += H . W2T_j
  auto gelu_out = [&](const f32x16& S, int j, const unsigned char* w2, f32x16(&acc)[NT]) {
    float hv[16];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const f32x4 bb = *reinterpret_cast<const f32x4*>(b1s + 32 * j + 8 * m + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) hv[4 * m + e] = gelu_tanh(S[4 * m + e] + bb[e]);
    }
    const bf16x8v hf0 = pack_frag(hv, 0), hf1 = pack_frag(hv, 8);
    bf16x8v b0 = mlp_tr_frag<D>(w2, lane, 0, 0), b1 = mlp_tr_frag<D>(w2, lane, 1, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int tn = t + 1 < NT ? t + 1 : t;
      const bf16x8v n0 = mlp_tr_frag<D>(w2, lane, 0, tn), n1 = mlp_tr_frag<D>(w2, lane, 1, tn);
      acc[t] = mfma32(hf0, b0, acc[t]);
      acc[t] = mfma32(hf1, b1, acc[t]);
      b0 = n0;
      b1 = n1;
      asm volatile("" ::: "memory");
    }
  };
  int g = 0;
  int64_t tix = 0;
  bool fed = true;  // the previous step issued the DMAs of a further chunk (workgroup-uniform)
  for (int64_t t0 = rs; t0 < re; t0 += TR, ++tix) {
    const int64_t lim = min(t0 + TR, re), rb = t0 + 32 * wave;
    const bool active = rb < lim;  // wave-uniform: a wave past the tile's rows only streams weights
    bf16x8v xf[KS];
    if (a.ln_w) mlp_load_ln<D, KS>(a, lws, a.ln_b ? lbs : nullptr, rb + r32, rb + r32 < lim, h, xf);
    else mlp_load_x<D, KS>(a.X, rb + r32, rb + r32 < lim, h, xf);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
    for (int j = 0; j < NC; ++j, ++g) {
      // retire chunk g; at prefetch distance 2 chunk g + 1 stays in flight (a tile's first step
      // drains: the x / residual / output accesses were issued behind the DMAs)
      // vmcnt(DPC) retires chunk g only while the DPC newest operations are chunk g + 1's DMAs,
      // issued by the previous step.  The stream's last step follows a step that issued none
      // (chunk g + 1 does not exist): the newest DPC operations are then chunk g's own, which
      // vmcnt(DPC) would leave in flight before the LDS reads below, so that step drains too
      // (NC >= 3; at NC <= 2 the last step's chunk was retired by a tile's first step)
      if (j == 0 || !fed) wait_vm<0>();
      else wait_vm<DPC>();
      __syncthreads();  // chunk g landed everywhere; every wave is done with chunk g + DIST - NS
      asm volatile("" ::: "memory");
      {
        // chunk g + DIST: of this tile, or the next tile's (same weights, chunk index wraps)
        const int64_t cg = (int64_t)j + DIST;
        fed = tix + cg / NC < ntile_wg;
        if (fed) {
          const int jn = (int)(cg % NC);
          unsigned char* dst = img[(g + DIST) % NS][0];
          mlp_dma32<D, NTH>(dst, a.W1 + (int64_t)jn * 32 * D, tid);
          mlp_dma32<D, NTH>(dst + IMG, a.W2T + (int64_t)jn * 32 * D, tid);
        }
      }
      if (!active) continue;
      const f32x16 Sj = s_phase(img[g % NS][0], xf);
      gelu_out(Sj, j, img[g % NS][1], acc);
    }
    if (active) {
      if (a.res1 && a.res2) mlp_fwd_epi<D, NT, 2>(a, acc, b2s, stg, rb, lim, lane);
      else if (a.res1) mlp_fwd_epi<D, NT, 1>(a, acc, b2s, stg, rb, lim, lane);
      else mlp_fwd_epi<D, NT, 0>(a, acc, b2s, stg, rb, lim, lane);
    }
  }
}

// ---------------------------------------------------------------- backward (recompute)
// The training backward of the fused MLP: the hidden is recomputed, never read from HBM.
// Per token row x (ln_2 output, bf16) and upstream gradient dy (bf16):
//   pre  = x W1^T + b1        g = GELU(pre)          (hidden unit i: c_fc row i)
//   dH   = dy W2              dpre = dH * GELU'(pre)
//   dX   = dpre W1                                    (-> the ln_2 backward)
// and the two [M, HID] operands of the weight gradients, g (for dW2 = dy^T g) and dpre
// (for dW1 = dpre^T x, db1 = colsum dpre), are written once (bf16).  Same structure as
// the forward: a wave owns 32 token rows with x and dy held in registers as B operands,
// the hidden is walked in 32-unit chunks whose W1 / W2T images ride a 2-slot LDS-DMA
// ring; per chunk
//   S^T  = W1_j . x^T,  dH^T = W2T_j . dy^T        (hidden on registers, tokens on lanes)
//   dp   = dH * GELU'(S + b1), g = GELU(S + b1)     (one v_exp + v_rcp per element)
//   dX  += dp . W1_j                                (dp packed to bf16 IS the A operand; B:
//                                                    transposed reads of the same W1_j image)
// g and dp leave through the wave's LDS strip as 64-B row pieces.  One wave per SIMD (the
// x / dy fragments and the dX accumulator are 256 registers).
template <int D, int NW, bool GH>
__global__ __launch_bounds__(64 * NW, 1) void mlp_bwd_k(MlpBwdArgs a) {
  constexpr int NTH = 64 * NW, IMG = 32 * D * 2, KS = D / 16, NT = D / 32, TR = 32 * NW;
  __shared__ __attribute__((aligned(16))) unsigned char img[2][2][IMG];  // [stage][W1_j, W2T_j]
  __shared__ __attribute__((aligned(16))) float stg_all[NW][32 * 32];    // per-wave strips
  __shared__ float b1s[8192];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int NC = a.HID / 32;
  const int64_t rs = a.M * blockIdx.x / gridDim.x, re = a.M * (blockIdx.x + 1) / gridDim.x;
  if (rs >= re) return;  // uniform
  for (int i = tid; i < a.HID; i += NTH) b1s[i] = a.b1 ? a.b1[i] : 0.f;
  float* stg = stg_all[wave];
  bf16_t* stb = reinterpret_cast<bf16_t*>(stg);  // bf16 view: [32 rows][32 units] g, then dp
  retire_loads();
  mlp_dma32<D, NTH>(img[0][0], a.W1, tid);
  mlp_dma32<D, NTH>(img[0][1], a.W2T, tid);
  __syncthreads();  // b1s
  int g = 0;
  for (int64_t t0 = rs; t0 < re; t0 += TR) {
    const int64_t lim = min(t0 + TR, re), rb = t0 + 32 * wave;
    const bool active = rb < lim;  // wave-uniform
    bf16x8v xf[KS], df[KS];
    mlp_load_x<D, KS>(a.X, rb + r32, rb + r32 < lim, h, xf);
    mlp_load_x<D, KS>(a.dY, rb + r32, rb + r32 < lim, h, df);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
    const bool more_tiles = t0 + TR < re;
    for (int j = 0; j < NC; ++j, ++g) {
      wait_vm<0>();
      __syncthreads();  // chunk j landed everywhere; every wave is done with chunk j - 1's stage
      asm volatile("" ::: "memory");
      if (j + 1 < NC || more_tiles) {
        const int jn = j + 1 < NC ? j + 1 : 0;
        mlp_dma32<D, NTH>(img[(g + 1) & 1][0], a.W1 + (int64_t)jn * 32 * D, tid);
        mlp_dma32<D, NTH>(img[(g + 1) & 1][1], a.W2T + (int64_t)jn * 32 * D, tid);
      }
      if (!active) continue;
      const unsigned char* w1 = img[g & 1][0];
      const unsigned char* w2 = img[g & 1][1];
      f32x16 S = f32x16{}, dH = f32x16{};
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        S = mfma32(mlp_row_frag<D>(w1, lane, k), xf[k], S);
        dH = mfma32(mlp_row_frag<D>(w2, lane, k), df[k], dH);
        __builtin_amdgcn_sched_barrier(0);
      }
      // g straight into the strip (8-B writes of 4 consecutive units), dp kept for the MFMA
      float dp[16];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const f32x4 bb = *reinterpret_cast<const f32x4*>(b1s + 32 * j + 8 * m + 4 * h);
        float gv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float gd;
          gv[e] = gelu_tanh_and_grad(S[4 * m + e] + bb[e], gd);
          dp[4 * m + e] = dH[4 * m + e] * gd;
        }
        if constexpr (GH)
          *reinterpret_cast<uint2*>(stb + r32 * 32 + 8 * (m ^ ((r32 >> 2) & 3)) + 4 * h) =
              uint2{pack_bf16x2(gv[0], gv[1]), pack_bf16x2(gv[2], gv[3])};
      }
      const bf16x8v d0 = pack_frag(dp, 0), d1 = pack_frag(dp, 8);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[t] = mfma32(d0, mlp_tr_frag<D>(w1, lane, 0, t), acc[t]);
        acc[t] = mfma32(d1, mlp_tr_frag<D>(w1, lane, 1, t), acc[t]);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (!GH) continue;  // dX only (the weight gradients come from mlp_wgrad_k)
      // g and dp of the chunk: [32 tokens][32 units] bf16 through the strip (8-B writes of
      // 4 consecutive units), then 16-B row pieces: lane -> row l / 4 (+ 16), piece l % 4
#pragma unroll
      for (int m = 0; m < 4; ++m)
        *reinterpret_cast<uint2*>(stb + 1024 + r32 * 32 + 8 * (m ^ ((r32 >> 2) & 3)) + 4 * h) =
            uint2{pack_bf16x2(dp[4 * m], dp[4 * m + 1]), pack_bf16x2(dp[4 * m + 2], dp[4 * m + 3])};
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int rl = (lane >> 2) + 16 * q, pc = 8 * (lane & 3);
        const int64_t row = rb + rl;
        const u32x4 vg = *reinterpret_cast<const u32x4*>(stb + rl * 32 + (pc ^ (8 * ((rl >> 2) & 3))));
        const u32x4 vd = *reinterpret_cast<const u32x4*>(stb + 1024 + rl * 32 + (pc ^ (8 * ((rl >> 2) & 3))));
        if (row < lim) {
          *reinterpret_cast<u32x4*>(a.G + row * a.HID + 32 * j + pc) = vg;
          *reinterpret_cast<u32x4*>(a.dP + row * a.HID + 32 * j + pc) = vd;
        }
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
    }
    if (!active) continue;
    // dX [32 tokens][D]: each 32-column tile through the strip, 16-B pieces out
    const int pr = lane >> 3, pc = 4 * (lane & 7);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int i = 0; i < 16; ++i) stg[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r32] = acc[t][i];
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int64_t row = rb + pr + 8 * m;
        const f32x4 v = *reinterpret_cast<const f32x4*>(stg + (pr + 8 * m) * 32 + pc);
        if (row < lim) {
          if (a.dx_f32) {
            *reinterpret_cast<f32x4*>(a.dXf + row * D + 32 * t + pc) = v;
          } else {
            *reinterpret_cast<uint2*>(a.dXb + row * D + 32 * t + pc) =
                uint2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
    }
  }
}

// dX alone, software-pipelined (round 5; the weight gradients come from mlp_wgrad_k, so neither
// G nor dP is written).  One wave per SIMD, a wave owns 32 token rows (x and dy in registers as B
// operands, the dX sum in the accumulator registers); the hidden chunks' W1_j / W2T_j images ride
// a 4-slot LDS-DMA ring.  Step j of a tile is ONE interleaved loop of KS iterations; iteration k
// issues
//   S'^T += W1_{j+1} . x^T, dH'^T += W2T_{j+1} . dy^T   k-step k (2 MFMAs; row reads one step ahead)
//   dX   += dp_{j-1} . W1_{j-1}                          output tile k / 2, k-half k % 2 (1 MFMA)
//   GELU' element(s) of chunk j from its S^T / dH^T      (the VALU in those MFMAs' issue gaps)
// so the vector work of a chunk spreads over all 48 of its MFMAs.  The chunk stream runs on across
// tiles (chunk index wraps); a tile's first step adds dp = 0 (exact zeros), its last step's S' / dH'
// (of the next tile's first chunk image, with this tile's x / dy) are discarded.
template <int D, int NW>
__global__ __launch_bounds__(64 * NW, 1) void mlp_bwdx_k(MlpBwdArgs a) {
  constexpr int NTH = 64 * NW, IMG = 32 * D * 2, KS = D / 16, NT = D / 32, TR = 32 * NW, NS = 4;
  static_assert(KS == 2 * NT, "one dX MFMA per k-step");
  constexpr int EPK = 16 / KS;  // GELU' elements per iteration
  __shared__ __attribute__((aligned(16))) unsigned char img[NS][2][IMG];  // [slot][W1_j, W2T_j]
  __shared__ __attribute__((aligned(16))) float stg_all[NW][32 * 32];    // per-wave epilogue strips
  __shared__ __attribute__((aligned(16))) float b1s[4096];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int NC = a.HID / 32;
  const int64_t rs = a.M * blockIdx.x / gridDim.x, re = a.M * (blockIdx.x + 1) / gridDim.x;
  if (rs >= re) return;  // uniform
  for (int i = tid; i < a.HID; i += NTH) b1s[i] = a.b1 ? a.b1[i] : 0.f;
  float* stg = stg_all[wave];
  retire_loads();
  const int64_t ntile = (re - rs + TR - 1) / TR;
  const int nchunk = (int)(ntile * NC);  // the workgroup's chunk stream
  MlpDmaPlan<D, NTH> plan;
  plan.init(tid);
  const uint32_t lds0 = lds_addr(img[0][0]) + (uint32_t)(tid & ~63) * 16u;  // this wave's slice of slot 0
  int sjn = 0;  // hidden chunk index of the next chunk to stage (the stream's index mod NC)
  auto stage = [&](int c) {  // chunk c of the stream, hidden chunk sjn
    const uint32_t d = lds0 + (uint32_t)(c & (NS - 1)) * (2u * IMG);
    plan.issue(a.W1 + (int64_t)sjn * 32 * D, d);
    plan.issue(a.W2T + (int64_t)sjn * 32 * D, d + IMG);
    if (++sjn == NC) sjn = 0;
  };
  stage(0);
  if (nchunk > 1) stage(1);
  int g = 0;  // chunk index of the current step in the workgroup's stream
  for (int64_t t0 = rs; t0 < re; t0 += TR) {
    // every wave computes (a wave past the tile's rows reads the clamped first row and stores
    // nothing): no wave-dependent branch around the accumulator updates
    const int64_t lim = min(t0 + TR, re), rb = t0 + 32 * wave;
    const bool active = rb < lim;  // wave-uniform
    bf16x8v xf[KS], df[KS];
    mlp_load_x<D, KS>(a.X, rb + r32, rb + r32 < lim, h, xf);
    mlp_load_x<D, KS>(a.dY, rb + r32, rb + r32 < lim, h, df);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
    // chunk g (the tile's first) landed everywhere (also: the x / dy loads above)
    wait_vm<0>();
    __syncthreads();
    f32x16 S = f32x16{}, H = f32x16{};
    {
      const unsigned char* w1 = img[g & (NS - 1)][0];
      const unsigned char* w2 = img[g & (NS - 1)][1];
      bf16x8v fa = mlp_row_frag<D>(w1, lane, 0), fb = mlp_row_frag<D>(w2, lane, 0);
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        const int kn = k + 1 < KS ? k + 1 : k;
        const bf16x8v na = mlp_row_frag<D>(w1, lane, kn), nb = mlp_row_frag<D>(w2, lane, kn);
        S = mfma32(fa, xf[k], S);
        H = mfma32(fb, df[k], H);
        fa = na;
        fb = nb;
        asm volatile("" ::: "memory");
      }
    }
    u32x4 dp0 = {0u, 0u, 0u, 0u}, dp1 = dp0;  // packed dp of the previous chunk (zero before the first)
    for (int j = 0; j < NC; ++j, ++g) {
      if (j > 0) {
        // every wave is done with step j - 1 (the slot of chunk g - 2 is free); chunk g + 1 landed
        wait_vm<0>();
        __syncthreads();
        asm volatile("" ::: "memory");
      }
      // chunk g + 2 into the slot of chunk g - 2 (last read by step g - 1: every wave passed this
      // step's barrier, or the tile's opening one at j = 0)
      if (g + 2 < nchunk) stage(g + 2);
      const unsigned char* w1p = img[(j > 0 ? g - 1 : g) & (NS - 1)][0];  // dX: chunk g - 1's W1 (or dp = 0)
      const unsigned char* w1n = img[(g + 1) & (NS - 1)][0];              // S' / dH' of chunk g + 1
      const unsigned char* w2n = img[(g + 1) & (NS - 1)][1];
      const bf16x8v d0 = __builtin_bit_cast(bf16x8v, dp0), d1 = __builtin_bit_cast(bf16x8v, dp1);
      f32x16 Sn = f32x16{}, Hn = f32x16{};
      float dl = 0.f;
      f32x4 bb = *reinterpret_cast<const f32x4*>(b1s + 32 * j + 4 * h);
      // LDS fragments two iterations ahead (one iteration is 3 MFMAs, ~100 cycles: less than an LDS
      // read's latency under load)
      bf16x8v fa = mlp_row_frag<D>(w1n, lane, 0), fb = mlp_row_frag<D>(w2n, lane, 0);
      bf16x8v bt = mlp_tr_frag<D>(w1p, lane, 0, 0);
      bf16x8v fa1 = mlp_row_frag<D>(w1n, lane, 1), fb1 = mlp_row_frag<D>(w2n, lane, 1);
      bf16x8v bt1 = mlp_tr_frag<D>(w1p, lane, 1, 0);
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        const int kn = k + 2 < KS ? k + 2 : KS - 1;
        const bf16x8v na = mlp_row_frag<D>(w1n, lane, kn), nb = mlp_row_frag<D>(w2n, lane, kn);
        const bf16x8v nt_ = mlp_tr_frag<D>(w1p, lane, kn & 1, kn >> 1);
        Sn = mfma32(fa, xf[k], Sn);
        acc[k >> 1] = mfma32((k & 1) ? d1 : d0, bt, acc[k >> 1]);
        Hn = mfma32(fb, df[k], Hn);
#pragma unroll
        for (int ee = 0; ee < EPK; ++ee) {
          const int e = k * EPK + ee;  // register e: unit 8 (e >> 2) + 4 h + (e & 3) of chunk j
          if ((e & 3) == 0 && e > 0) bb = *reinterpret_cast<const f32x4*>(b1s + 32 * j + 8 * (e >> 2) + 4 * h);
          const float dk = H[e] * gelu_tanh_grad(S[e] + bb[e & 3]);
          if (e & 1) {
            uint32_t dw = pack_bf16x2(dl, dk);
            asm volatile("" : "+v"(dw)::"memory");  // element e's VALU stays beside these MFMAs
            if (e < 8) dp0[(e >> 1) & 3] = dw;
            else dp1[(e >> 1) & 3] = dw;
          } else {
            dl = dk;
            asm volatile("" : "+v"(dl)::"memory");
          }
        }
        fa = fa1;
        fb = fb1;
        bt = bt1;
        fa1 = na;
        fb1 = nb;
        bt1 = nt_;
      }
      S = Sn;
      H = Hn;
    }
    {  // dX of the tile's last chunk (g - 1)
      const unsigned char* w1p = img[(g - 1) & (NS - 1)][0];
      const bf16x8v d0 = __builtin_bit_cast(bf16x8v, dp0), d1 = __builtin_bit_cast(bf16x8v, dp1);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[t] = mfma32(d0, mlp_tr_frag<D>(w1p, lane, 0, t), acc[t]);
        acc[t] = mfma32(d1, mlp_tr_frag<D>(w1p, lane, 1, t), acc[t]);
      }
    }
    // dX [32 tokens][D]: each 32-column tile through the strip, 16-B pieces out
    const int pr = lane >> 3, pc = 4 * (lane & 7);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int i = 0; i < 16; ++i) stg[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r32] = acc[t][i];
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int64_t row = rb + pr + 8 * m;
        const f32x4 v = *reinterpret_cast<const f32x4*>(stg + (pr + 8 * m) * 32 + pc);
        if (active && row < lim) {
          if (a.dx_f32) {
            *reinterpret_cast<f32x4*>(a.dXf + row * D + 32 * t + pc) = v;
          } else {
            *reinterpret_cast<uint2*>(a.dXb + row * D + 32 * t + pc) =
                uint2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
    }
  }
}

// The split backward: the same recompute without the dX accumulator (dX = dP W1 then runs on
// the GEMM), so the x / dy fragments (128 registers) leave room for two waves per SIMD.
template <int D, int NW>
__global__ __launch_bounds__(64 * NW, 1) void mlp_bwdp_k(MlpBwdArgs a) {
  constexpr int NTH = 64 * NW, IMG = 32 * D * 2, KS = D / 16, TR = 32 * NW;
  __shared__ __attribute__((aligned(16))) unsigned char img[2][2][IMG];  // [stage][W1_j, W2T_j]
  // per-wave g / dp strips: 32 rows x four 16-B chunks, chunk c of row r at c ^ ((r >> 2) & 3) (the
  // C-layout b64 writes 2-way instead of 8-way bank-conflicted, the 16-B row reads conflict-free)
  __shared__ __attribute__((aligned(16))) bf16_t stb_all[NW][2 * 32 * 32];
  __shared__ float b1s[4096];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int NC = a.HID / 32;
  const int64_t rs = a.M * blockIdx.x / gridDim.x, re = a.M * (blockIdx.x + 1) / gridDim.x;
  if (rs >= re) return;  // uniform
  for (int i = tid; i < a.HID; i += NTH) b1s[i] = a.b1 ? a.b1[i] : 0.f;
  bf16_t* stb = stb_all[wave];
  retire_loads();
  mlp_dma32<D, NTH>(img[0][0], a.W1, tid);
  mlp_dma32<D, NTH>(img[0][1], a.W2T, tid);
  __syncthreads();  // b1s
  int g = 0;
  // the previous step issued its 4 G / dP stores AFTER the DMA of this step's chunk: a full-tile
  // wave retires the DMA with vmcnt 4, leaving its stores in flight (vmcnt retires in order)
  bool st4 = false;
  for (int64_t t0 = rs; t0 < re; t0 += TR) {
    const int64_t lim = min(t0 + TR, re), rb = t0 + 32 * wave;
    const bool active = rb < lim;  // wave-uniform
    const bool full = rb + 32 <= lim;
    bf16x8v xf[KS], df[KS];
    mlp_load_x<D, KS>(a.X, rb + r32, rb + r32 < lim, h, xf);
    mlp_load_x<D, KS>(a.dY, rb + r32, rb + r32 < lim, h, df);
    const bool more_tiles = t0 + TR < re;
    for (int j = 0; j < NC; ++j, ++g) {
      if (st4) wait_vm<4>();
      else wait_vm<0>();
      st4 = false;
      __syncthreads();  // chunk j landed everywhere; every wave is done with chunk j - 1's stage
      asm volatile("" ::: "memory");
      if (j + 1 < NC || more_tiles) {
        const int jn = j + 1 < NC ? j + 1 : 0;
        mlp_dma32<D, NTH>(img[(g + 1) & 1][0], a.W1 + (int64_t)jn * 32 * D, tid);
        mlp_dma32<D, NTH>(img[(g + 1) & 1][1], a.W2T + (int64_t)jn * 32 * D, tid);
      }
      if (!active) continue;
      const unsigned char* w1 = img[g & 1][0];
      const unsigned char* w2 = img[g & 1][1];
      f32x16 S = f32x16{}, dH = f32x16{};
      bf16x8v fa = mlp_row_frag<D>(w1, lane, 0), fb = mlp_row_frag<D>(w2, lane, 0);
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        const int kn = k + 1 < KS ? k + 1 : k;
        const bf16x8v na = mlp_row_frag<D>(w1, lane, kn), nb = mlp_row_frag<D>(w2, lane, kn);
        S = mfma32(fa, xf[k], S);
        dH = mfma32(fb, df[k], dH);
        fa = na;
        fb = nb;
        asm volatile("" ::: "memory");
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const f32x4 bb = *reinterpret_cast<const f32x4*>(b1s + 32 * j + 8 * m + 4 * h);
        float gv[4], dv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float gd;
          gv[e] = gelu_tanh_and_grad(S[4 * m + e] + bb[e], gd);
          dv[e] = dH[4 * m + e] * gd;
        }
        *reinterpret_cast<uint2*>(stb + r32 * 32 + 8 * (m ^ ((r32 >> 2) & 3)) + 4 * h) = uint2{pack_bf16x2(gv[0], gv[1]), pack_bf16x2(gv[2], gv[3])};
        *reinterpret_cast<uint2*>(stb + 1024 + r32 * 32 + 8 * (m ^ ((r32 >> 2) & 3)) + 4 * h) =
            uint2{pack_bf16x2(dv[0], dv[1]), pack_bf16x2(dv[2], dv[3])};
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int rl = (lane >> 2) + 16 * q, pc = 8 * (lane & 3);
        const int64_t row = rb + rl;
        const u32x4 vg = *reinterpret_cast<const u32x4*>(stb + rl * 32 + (pc ^ (8 * ((rl >> 2) & 3))));
        const u32x4 vd = *reinterpret_cast<const u32x4*>(stb + 1024 + rl * 32 + (pc ^ (8 * ((rl >> 2) & 3))));
        if (row < lim) {
          *reinterpret_cast<u32x4*>(a.G + row * a.HID + 32 * j + pc) = vg;
          *reinterpret_cast<u32x4*>(a.dP + row * a.HID + 32 * j + pc) = vd;
        }
      }
      st4 = full;  // every lane stored: exactly 4 store instructions issued
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
    }
  }
}

// ---------------------------------------------------------------- weight gradients (recompute)
// dW1 = dpre^T x, dW2^T = g^T dy, db1 = colsum dpre with g / dpre recomputed per token tile and
// never written: the loop order is the transpose of the kernels above.  A wave OWNS 32 hidden
// units j (its W1_j / W2T_j rows live in registers as B operands) and its dW1_j / dW2^T_j
// [32 x D] sums live in the accumulator registers for the whole kernel; the workgroup (NW
// waves, NW * 32 hidden units = one hidden group) walks the token tiles of its slice, each
// [32 x D] x and dy tile staged once into LDS by LDS-DMA (3-slot ring) and read by every wave:
//   S  = x . W1_j^T,  dH = dy . W2T_j^T      (tokens on the accumulator registers, hidden units
//                                             on the lanes: 2 x D / 16 MFMAs)
//   g  = GELU(S + b1), dp = dH GELU'(S + b1)  (one v_exp + one v_rcp per element)
//   dW1_j   += dp^T . x,  dW2^T_j += g^T . dy (the packed accumulators ARE the A operands over
//                                             the permuted token order; B = transposed reads of
//                                             the staged tiles: 2 x D / 16 MFMAs)
// so per token tile and wave 4 D / 16 MFMAs, no HBM traffic beyond x and dy (read once per
// hidden group; the groups of one slice run on one XCD, so the repeats are L2 hits).  The slabs
// [nslice][HID][D] are folded in slice order by mlp_wgrad_fold_k (no atomics, deterministic).
template <int D, int NW, bool FULL>
__global__ __launch_bounds__(64 * NW, 1) void mlp_wgrad_k(MlpWgArgs a) {
  constexpr int NTH = 64 * NW, IMG = 32 * D * 2, KS = D / 16, NT = D / 32, NS = 3;
  constexpr int DPT = 2 * (32 * D / 8) / NTH;  // DMAs per thread and tile (both images)
  // 3-slot ring of (x, dy) tiles + each wave's W2T_j image: 160 KiB at D = 256.  The dW sums take
  // the 256 accumulator registers and W1_j's B operands 64 of the 256 others, so W2T_j's B
  // operands are read from LDS (a second ds_read_b128 in the dH MFMA gaps)
  __shared__ __attribute__((aligned(16))) unsigned char img[NS][2][IMG];  // [slot][x, dy]
  __shared__ __attribute__((aligned(16))) unsigned char wimg[NW][IMG];    // W2T_j per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  // XCD-contiguous logical order: the hidden groups of one slice share an XCD's L2
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int slice = lid / a.ngroup, grp = lid - slice * a.ngroup;
  const int64_t ntile_all = (a.M + 31) / 32;
  const int64_t t_lo = ntile_all * slice / a.nslice, t_hi = ntile_all * (slice + 1) / a.nslice;
  const int j0 = (grp * NW + wave) * 32;  // this wave's hidden units j0 .. j0 + 31
  // B operands over d of the wave's W1 rows: lane -> unit j0 + r32, k 16 k + 8 h ..
  bf16x8v w1f[KS];
  {
    const bf16_t* p1 = a.W1 + (int64_t)(j0 + r32) * D + 8 * h;
#pragma unroll
    for (int k = 0; k < KS; ++k) w1f[k] = __builtin_bit_cast(bf16x8v, *reinterpret_cast<const u32x4*>(p1 + 16 * k));
  }
  unsigned char* w2i = wimg[wave];
  const float bj = a.b1 ? a.b1[j0 + r32] : 0.f;
  f32x16 acc1[NT], acc2[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc1[t] = acc2[t] = f32x16{};
  float dbs = 0.f;
  retire_loads();
  const int nt = (int)(t_hi - t_lo);
  MlpDmaPlan<D, NTH> plan;
  plan.init(tid);
  const uint32_t lds0 = lds_addr(img[0][0]) + (uint32_t)(tid & ~63) * 16u;  // this wave's slice of slot 0
  auto stage = [&](int64_t ti, int slot) {
    const int64_t r0 = ti * 32;
    if (FULL) {  // every tile whole: the precomputed plan
      const uint32_t d = lds0 + (uint32_t)slot * (2u * IMG);
      plan.issue(a.X + r0 * D, d);
      plan.issue(a.dY + r0 * D, d + IMG);
    } else {
      const int nv = (int)min((int64_t)32, a.M - r0);
      mlp_dma32c<D, NTH>(img[slot][0], a.X, r0, nv, tid);
      mlp_dma32c<D, NTH>(img[slot][1], a.dY, r0, nv, tid);
    }
  };
  // Software pipeline, one wave per SIMD (the dW sums hold the 256 accumulator registers): step i
  // runs
  //   phase B: dW += of tile i - 1 (32 MFMAs; transposed tile reads one pair ahead)  ||  GELU of
  //            tile i from its S / dH registers (the VALU in the MFMA issue gaps), packed to bf16
  //   barrier; LDS-DMA of tile i + 2 into the slot of tile i - 1 (free now)
  //   phase A: S / dH of tile i + 1 (32 MFMAs)
  // so only one S / dH pair and two packed operand sets are live.  Tile i + 1 was staged during
  // step i - 1 (after its barrier); tile i is not read by step i at all.
  mlp_dma32<D, 64>(w2i, a.W2T + (int64_t)j0 * D, lane);  // the wave's own image (retired with tile 0)
  if (nt > 0) stage(t_lo, 0);
  if (nt > 1) stage(t_lo + 1, 1);
  f32x16 S = f32x16{}, H = f32x16{};
  auto phase_a = [&](const unsigned char* xn, const unsigned char* yn) {
    bf16x8v fa = mlp_row_frag<D>(xn, lane, 0), fb = mlp_row_frag<D>(yn, lane, 0), fw = mlp_row_frag<D>(w2i, lane, 0);
    S = f32x16{};
    H = f32x16{};
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int kn = k + 1 < KS ? k + 1 : k;
      const bf16x8v na = mlp_row_frag<D>(xn, lane, kn), nb = mlp_row_frag<D>(yn, lane, kn);
      const bf16x8v nw = mlp_row_frag<D>(w2i, lane, kn);
      S = mfma32(fa, w1f[k], S);
      H = mfma32(fb, fw, H);
      fa = na;
      fb = nb;
      fw = nw;
      asm volatile("" ::: "memory");
    }
  };
  if (nt > 0) {
    if (nt > 1) wait_vm<DPT>();
    else wait_vm<0>();
    __syncthreads();
    phase_a(img[0][0], img[0][1]);
  }
  // packed operands of the previous tile (zero before tile 0: phase B of step 0 adds exact zeros
  // from tile 0's finite rows)
  u32x4 gp0 = {0u, 0u, 0u, 0u}, gp1 = gp0, dp0 = gp0, dp1 = gp0;
  for (int i = 0; i < nt; ++i) {
    // ---- phase B: dW of tile i - 1 || GELU of tile i
    {
      const int ip = i > 0 ? i - 1 : 0;
      const unsigned char* xi = img[ip % NS][0];
      const unsigned char* yi = img[ip % NS][1];
      const int nv = (int)min((int64_t)32, a.M - (t_lo + i) * 32);  // valid token rows of tile i
      const bf16x8v d0 = __builtin_bit_cast(bf16x8v, dp0), d1 = __builtin_bit_cast(bf16x8v, dp1);
      const bf16x8v g0 = __builtin_bit_cast(bf16x8v, gp0), g1 = __builtin_bit_cast(bf16x8v, gp1);
      float gl = 0.f, dl = 0.f;
      bf16x8v b0 = mlp_tr_frag<D>(xi, lane, 0, 0), b1 = mlp_tr_frag<D>(xi, lane, 1, 0);
#pragma unroll
      for (int k = 0; k < 2 * NT; ++k) {  // step k: output tile t = k / 2, half u = k % 2 (dW1, dW2^T)
        const int t = k >> 1, u = k & 1, tn = t + 1 < NT ? t + 1 : t;
        const unsigned char* nimg = u == 0 ? yi : xi;
        const int nt_ = u == 0 ? t : tn;
        const bf16x8v n0 = mlp_tr_frag<D>(nimg, lane, 0, nt_), n1 = mlp_tr_frag<D>(nimg, lane, 1, nt_);
        if (u == 0) {
          acc1[t] = mfma32(d0, b0, acc1[t]);
          acc1[t] = mfma32(d1, b1, acc1[t]);
        } else {
          acc2[t] = mfma32(g0, b0, acc2[t]);
          acc2[t] = mfma32(g1, b1, acc2[t]);
        }
        // GELU elements of tile i beside this step's MFMAs: 16 / (2 NT) per step (register e: token
        // row 8 (e >> 2) + 4 h + (e & 3))
        constexpr int EPS = 16 / (2 * NT);
#pragma unroll
        for (int ee = 0; ee < EPS; ++ee) {
          const int e = k * EPS + ee;
          float gd;
          const float gg = gelu_tanh_and_grad(S[e] + bj, gd);
          const bool ok = FULL || 8 * (e >> 2) + 4 * h + (e & 3) < nv;  // token rows past M
          const float gk = ok ? gg : 0.f, dk = ok ? H[e] * gd : 0.f;
          dbs += dk;
          if (e & 1) {
            uint32_t gw = pack_bf16x2(gl, gk), dw = pack_bf16x2(dl, dk);
            // pins element e's VALU into this step's scheduling region, beside its MFMAs
            asm volatile("" : "+v"(gw), "+v"(dw), "+v"(dbs)::"memory");
            const int q = (e >> 1) & 3;
            if (e < 8) {
              gp0[q] = gw;
              dp0[q] = dw;
            } else {
              gp1[q] = gw;
              dp1[q] = dw;
            }
          } else {
            gl = gk;
            dl = dk;
            asm volatile("" : "+v"(gl), "+v"(dl), "+v"(dbs)::"memory");
          }
        }
        b0 = n0;
        b1 = n1;
      }
    }
    // ---- every wave is done with tile i - 1's slot; tile i + 1 landed everywhere
    wait_vm<0>();
    __syncthreads();
    asm volatile("" ::: "memory");
    if (i + 2 < nt) stage(t_lo + i + 2, (int)((i + 2) % NS));
    // ---- phase A: S / dH of tile i + 1 (past the last tile: a stale slot, results unused)
    phase_a(img[(i + 1) % NS][0], img[(i + 1) % NS][1]);
  }
  if (nt > 0) {  // phase B of the last tile
    const unsigned char* xi = img[(nt - 1) % NS][0];
    const unsigned char* yi = img[(nt - 1) % NS][1];
    const bf16x8v d0 = __builtin_bit_cast(bf16x8v, dp0), d1 = __builtin_bit_cast(bf16x8v, dp1);
    const bf16x8v g0 = __builtin_bit_cast(bf16x8v, gp0), g1 = __builtin_bit_cast(bf16x8v, gp1);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc1[t] = mfma32(d0, mlp_tr_frag<D>(xi, lane, 0, t), acc1[t]);
      acc1[t] = mfma32(d1, mlp_tr_frag<D>(xi, lane, 1, t), acc1[t]);
      acc2[t] = mfma32(g0, mlp_tr_frag<D>(yi, lane, 0, t), acc2[t]);
      acc2[t] = mfma32(g1, mlp_tr_frag<D>(yi, lane, 1, t), acc2[t]);
    }
  }
  // partial slabs: register v of tile t is unit j0 + 8 (v >> 2) + 4 h + (v & 3), column 32 t + r32
  float* p1 = a.dW1p + ((int64_t)slice * a.HID + j0) * D;
  float* p2 = a.dW2Tp + ((int64_t)slice * a.HID + j0) * D;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t o = (int64_t)(8 * (v >> 2) + 4 * h + (v & 3)) * D + 32 * t + r32;
      p1[o] = acc1[t][v];
      p2[o] = acc2[t][v];
    }
  dbs += __shfl_xor(dbs, 32, 64);
  if (a.db1p && h == 0) a.db1p[(int64_t)slice * a.HID + j0 + r32] = dbs;
}

// dW1 [HID][D] = sum over slices of dW1p; dW2 [D][HID] = (sum of dW2Tp)^T; db1 = sum of db1p --
// the slices in order 0, 1, ... (deterministic).  One block per 32 x 32 (unit, column) tile;
// the transposed dW2 goes out through an LDS tile.
__global__ __launch_bounds__(256) void mlp_wgrad_fold_k(const float* __restrict__ dW1p, const float* __restrict__ dW2Tp,
                                                        const float* __restrict__ db1p, int nslice, int HID, int D,
                                                        float* __restrict__ dW1, float* __restrict__ dW2,
                                                        float* __restrict__ db1) {
  __shared__ float tl[32][33];
  const int u0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 8 rows of 32 per pass
  const int64_t sl = (int64_t)HID * D;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int u = u0 + ty + 8 * q;
    const int64_t o = (int64_t)u * D + c0 + tx;
    float s1 = 0.f, s2 = 0.f;
    for (int s = 0; s < nslice; ++s) {
      s1 += dW1p[s * sl + o];
      s2 += dW2Tp[s * sl + o];
    }
    dW1[o] = s1;
    tl[ty + 8 * q][tx] = s2;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = c0 + ty + 8 * q;
    dW2[(int64_t)c * HID + u0 + tx] = tl[tx][ty + 8 * q];
  }
  if (db1 && blockIdx.x == 0 && threadIdx.x < 32) {
    float s = 0.f;
    for (int sidx = 0; sidx < nslice; ++sidx) s += db1p[(int64_t)sidx * HID + u0 + threadIdx.x];
    db1[u0 + threadIdx.x] = s;
  }
}

}  // namespace lthm

using namespace lthm;

// waves per workgroup of each kernel (a wave owns 32 token rows; the weight-gradient kernel: 32
// hidden units, one wave per SIMD: the two [32 x D] sums are 2 D / 2 registers)
constexpr int MLP_FWD_NW = 8, MLP_BWD_NW = 4, MLP_BWDP_NW = 8, MLP_BWDX_NW = 4, MLP_WG_NW = 4;

// The launch geometry of every entry point, on the host alone (include/lthm.h).  The LDS sums
// restate the kernels' __shared__ arrays (IMG = 32 x D bf16, a 4-KiB strip per wave: keep them in
// step with the kernels); tests/test_mlp_host.py holds the plan to a restatement of these rules.
extern "C" int lthm_mlp_plan(int32_t entry, int64_t M, int32_t D, int32_t HID, int32_t cus, lthm_mlp_plan_out* p) {
  LTHM_REQUIRE(p != nullptr && cus >= 1 && M >= 0);
  LTHM_REQUIRE((D == 128 || D == 256) && HID >= 32 && HID % 32 == 0 && HID <= 8192);
  *p = lthm_mlp_plan_out{};
  const int64_t img = 32 * (int64_t)D * 2, strip = 32 * 32 * 4;
  int nw = 0;
  switch (entry) {
    case LTHM_MLP_FWD:
    case LTHM_MLP_FWD_LN:  // 3-slot ring of (W1_j, W2T_j), strips; dynamic: b1, b2, ln w, ln b
      nw = MLP_FWD_NW;
      p->lds_static = 3 * 2 * img + nw * strip;
      p->lds_dynamic = ((int64_t)HID + 3 * D) * 4;
      break;
    case LTHM_MLP_BWD:  // 2-slot ring, strips, b1s[8192]
      nw = MLP_BWD_NW;
      p->lds_static = 2 * 2 * img + nw * strip + 8192 * 4;
      break;
    case LTHM_MLP_BWD_HIDDEN:  // 2-slot ring, bf16 g / dp strips, b1s[4096]
      LTHM_REQUIRE(HID <= 4096);
      nw = MLP_BWDP_NW;
      p->lds_static = 2 * 2 * img + nw * strip + 4096 * 4;
      break;
    case LTHM_MLP_BWD_DX:  // 4-slot ring, strips, b1s[4096]
      LTHM_REQUIRE(HID <= 4096);
      nw = MLP_BWDX_NW;
      p->lds_static = 4 * 2 * img + nw * strip + 4096 * 4;
      break;
    case LTHM_MLP_WGRAD:  // 3-slot ring of (x, dy) tiles, each wave's W2T_j image
      LTHM_REQUIRE(HID % (32 * MLP_WG_NW) == 0);
      nw = MLP_WG_NW;
      p->lds_static = 3 * 2 * img + nw * img;
      break;
    default:
      return (int)hipErrorInvalidValue;
  }
  LTHM_REQUIRE(p->lds_static + p->lds_dynamic <= LTHM_MLP_LDS_MAX);
  p->waves = nw;
  if (entry == LTHM_MLP_WGRAD) {
    p->tile_rows = 32;
    p->ntiles = (M + 31) / 32;
    p->ngroup = HID / (32 * nw);
    // one workgroup per CU: slices x groups ~ the CU count, at least one token tile per slice
    const int ns = std::max(1, cus / std::max(1, p->ngroup));
    p->nslice = (int)std::max<int64_t>(1, std::min<int64_t>(ns, p->ntiles));
    p->full = M % 32 == 0;
    p->ws_bytes = (int64_t)p->nslice * HID * (2 * (int64_t)D + 1) * 4;
    p->grid = M > 0 ? p->nslice * p->ngroup : 0;
    p->max_tiles = (int)((p->ntiles + p->nslice - 1) / p->nslice);
    return 0;
  }
  // persistent over contiguous row ranges: workgroup b owns rows M b / grid .. M (b + 1) / grid
  p->tile_rows = 32 * nw;
  p->ntiles = (M + p->tile_rows - 1) / p->tile_rows;
  p->grid = (int)std::min<int64_t>(p->ntiles, (int64_t)cus);
  if (p->grid > 0) {
    const int64_t rows = (M + p->grid - 1) / p->grid;  // the longest range
    p->max_tiles = (int)((rows + p->tile_rows - 1) / p->tile_rows);
  }
  return 0;
}

extern "C" int lthm_mlp_supported(int32_t D, int32_t HID) {
  // what both the forward and the backward take: at D = 256 the forward's dynamic LDS (b1) ends
  // this at HID = 7,424
  lthm_mlp_plan_out p;
  return lthm_mlp_plan(LTHM_MLP_FWD, 0, D, HID, 1, &p) == 0 && lthm_mlp_plan(LTHM_MLP_BWD, 0, D, HID, 1, &p) == 0;
}

static int mlp_fwd_launch(MlpArgs a, int D, const lthm_mlp_plan_out& pl, void* stream);

extern "C" int lthm_mlp_fwd_ln(const float* x, const float* ln_w, const float* ln_b, int64_t M, int32_t D,
                               int32_t HID, const void* W1, const float* b1, const void* W2T, const float* b2,
                               const float* res1, const float* res2, float* out, void* h_out, float* mean,
                               float* rstd, void* stream) {
  lthm_mlp_plan_out pl;
  if (const int rc = lthm_mlp_plan(LTHM_MLP_FWD_LN, M, D, HID, cu_count(), &pl)) return rc;
  if (M == 0) return 0;  // nothing to do: an empty tensor's pointers may be null
  LTHM_REQUIRE(x && ln_w && W1 && W2T && out);
  LTHM_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)W1 % 16) == 0 && ((uintptr_t)W2T % 16) == 0 &&
               ((uintptr_t)b1 % 16) == 0 && ((uintptr_t)h_out % 16) == 0);
  MlpArgs a{};
  a.X = nullptr; a.W1 = (const bf16_t*)W1; a.W2T = (const bf16_t*)W2T;
  a.b1 = b1; a.b2 = b2; a.res1 = res1; a.res2 = res2; a.out = out;
  a.M = M; a.HID = HID;
  a.x32 = x; a.ln_w = ln_w; a.ln_b = ln_b; a.h_out = (bf16_t*)h_out; a.mean = mean; a.rstd = rstd;
  return mlp_fwd_launch(a, D, pl, stream);
}

extern "C" int lthm_mlp_fwd(const void* X, int64_t M, int32_t D, int32_t HID, const void* W1, const float* b1,
                            const void* W2T, const float* b2, const float* res1, const float* res2, float* out,
                            void* stream) {
  lthm_mlp_plan_out pl;
  if (const int rc = lthm_mlp_plan(LTHM_MLP_FWD, M, D, HID, cu_count(), &pl)) return rc;
  if (M == 0) return 0;  // nothing to do: an empty tensor's pointers may be null
  LTHM_REQUIRE(X && W1 && W2T && out);
  LTHM_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)W1 % 16) == 0 && ((uintptr_t)W2T % 16) == 0 &&
               ((uintptr_t)b1 % 16) == 0);
  MlpArgs a{};
  a.X = (const bf16_t*)X; a.W1 = (const bf16_t*)W1; a.W2T = (const bf16_t*)W2T;
  a.b1 = b1; a.b2 = b2; a.res1 = res1; a.res2 = res2; a.out = out;
  a.M = M; a.HID = HID;
  return mlp_fwd_launch(a, D, pl, stream);
}

static int mlp_fwd_launch(MlpArgs a, int D, const lthm_mlp_plan_out& pl, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const size_t dyn = (size_t)pl.lds_dynamic;
  // 8 waves: one workgroup per CU, 256-row tiles
  constexpr int NW = MLP_FWD_NW;
  a.ntiles = (int)pl.ntiles;
  const int grid = pl.grid;
  if (D == 256) hipLaunchKernelGGL((mlp_fwd_k<256, NW>), dim3(grid), dim3(64 * NW), dyn, s, a);
  else hipLaunchKernelGGL((mlp_fwd_k<128, NW>), dim3(grid), dim3(64 * NW), dyn, s, a);
  LTHM_CHECK_LAUNCH();
  return 0;
}

extern "C" int lthm_mlp_bwd(const void* X, const void* dY, int64_t M, int32_t D, int32_t HID, const void* W1,
                            const float* b1, const void* W2T, void* dX, int32_t dx_dtype, void* G, void* dP,
                            void* stream) {
  lthm_mlp_plan_out pl;
  if (const int rc = lthm_mlp_plan(LTHM_MLP_BWD, M, D, HID, cu_count(), &pl)) return rc;
  if (M == 0) return 0;  // nothing to do: an empty tensor's pointers may be null
  LTHM_REQUIRE(X && dY && W1 && W2T && dX && G && dP && (dx_dtype == LTHM_F32 || dx_dtype == LTHM_BF16));
  LTHM_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)dY % 16) == 0 && ((uintptr_t)W1 % 16) == 0 &&
               ((uintptr_t)W2T % 16) == 0 && ((uintptr_t)b1 % 16) == 0 && ((uintptr_t)dX % 16) == 0 &&
               ((uintptr_t)G % 16) == 0 && ((uintptr_t)dP % 16) == 0);
  MlpBwdArgs a;
  a.X = (const bf16_t*)X; a.dY = (const bf16_t*)dY; a.W1 = (const bf16_t*)W1; a.W2T = (const bf16_t*)W2T;
  a.b1 = b1; a.G = (bf16_t*)G; a.dP = (bf16_t*)dP;
  a.dx_f32 = dx_dtype == LTHM_F32;
  a.dXf = (float*)dX; a.dXb = (bf16_t*)dX;
  a.M = M; a.HID = HID;
  hipStream_t s = (hipStream_t)stream;
  constexpr int NW = MLP_BWD_NW;
  const int grid = pl.grid;
  if (D == 256) hipLaunchKernelGGL((mlp_bwd_k<256, NW, true>), dim3(grid), dim3(64 * NW), 0, s, a);
  else hipLaunchKernelGGL((mlp_bwd_k<128, NW, true>), dim3(grid), dim3(64 * NW), 0, s, a);
  LTHM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t lthm_mlp_wgrad_ws_bytes(int64_t M, int32_t D, int32_t HID) {
  lthm_mlp_plan_out pl;
  if (lthm_mlp_plan(LTHM_MLP_WGRAD, M, D, HID, cu_count(), &pl)) return -1;
  return pl.ws_bytes;
}

extern "C" int lthm_mlp_wgrad(const void* X, const void* dY, int64_t M, int32_t D, int32_t HID, const void* W1,
                              const float* b1, const void* W2T, float* dW1, float* dW2, float* db1, void* workspace,
                              int64_t ws_bytes, void* stream) {
  lthm_mlp_plan_out pl;
  if (const int rc = lthm_mlp_plan(LTHM_MLP_WGRAD, M, D, HID, cu_count(), &pl)) return rc;
  LTHM_REQUIRE((M == 0 || (X && dY)) && W1 && W2T && dW1 && dW2 && workspace);  // M == 0: zeros
  LTHM_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)dY % 16) == 0 && ((uintptr_t)W1 % 16) == 0 &&
               ((uintptr_t)W2T % 16) == 0 && ((uintptr_t)workspace % 16) == 0);
  LTHM_REQUIRE(ws_bytes >= pl.ws_bytes);
  hipStream_t s = (hipStream_t)stream;
  const int ns = pl.nslice, ng = pl.ngroup;
  MlpWgArgs a{};
  a.X = (const bf16_t*)X; a.dY = (const bf16_t*)dY; a.W1 = (const bf16_t*)W1; a.W2T = (const bf16_t*)W2T;
  a.b1 = b1;
  a.dW1p = (float*)workspace;
  a.dW2Tp = a.dW1p + (int64_t)ns * HID * D;
  a.db1p = db1 ? a.dW2Tp + (int64_t)ns * HID * D : nullptr;
  a.M = M; a.HID = HID; a.nslice = ns; a.ngroup = ng;
  if (M > 0) {
    // every token tile full (M % 32 == 0, C2's 528,384 rows): no per-element row mask
    const bool full = pl.full != 0;
    if (D == 256) {
      if (full) hipLaunchKernelGGL((mlp_wgrad_k<256, MLP_WG_NW, true>), dim3(ns * ng), dim3(64 * MLP_WG_NW), 0, s, a);
      else hipLaunchKernelGGL((mlp_wgrad_k<256, MLP_WG_NW, false>), dim3(ns * ng), dim3(64 * MLP_WG_NW), 0, s, a);
    } else {
      if (full) hipLaunchKernelGGL((mlp_wgrad_k<128, MLP_WG_NW, true>), dim3(ns * ng), dim3(64 * MLP_WG_NW), 0, s, a);
      else hipLaunchKernelGGL((mlp_wgrad_k<128, MLP_WG_NW, false>), dim3(ns * ng), dim3(64 * MLP_WG_NW), 0, s, a);
    }
    LTHM_CHECK_LAUNCH();
  } else {
    LTHM_REQUIRE(hipMemsetAsync(workspace, 0, (size_t)pl.ws_bytes, s) == hipSuccess);
  }
  hipLaunchKernelGGL(mlp_wgrad_fold_k, dim3(D / 32, HID / 32), dim3(256), 0, s, (const float*)a.dW1p,
                     (const float*)a.dW2Tp, (const float*)a.db1p, ns, HID, D, dW1, dW2, db1);
  LTHM_CHECK_LAUNCH();
  return 0;
}

extern "C" int lthm_mlp_bwd_dx(const void* X, const void* dY, int64_t M, int32_t D, int32_t HID, const void* W1,
                               const float* b1, const void* W2T, void* dX, int32_t dx_dtype, void* stream) {
  lthm_mlp_plan_out pl;
  if (const int rc = lthm_mlp_plan(LTHM_MLP_BWD_DX, M, D, HID, cu_count(), &pl)) return rc;
  if (M == 0) return 0;  // nothing to do: an empty tensor's pointers may be null
  LTHM_REQUIRE(X && dY && W1 && W2T && dX && (dx_dtype == LTHM_F32 || dx_dtype == LTHM_BF16));
  LTHM_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)dY % 16) == 0 && ((uintptr_t)W1 % 16) == 0 &&
               ((uintptr_t)W2T % 16) == 0 && ((uintptr_t)b1 % 16) == 0 && ((uintptr_t)dX % 16) == 0);
  MlpBwdArgs a{};
  a.X = (const bf16_t*)X; a.dY = (const bf16_t*)dY; a.W1 = (const bf16_t*)W1; a.W2T = (const bf16_t*)W2T;
  a.b1 = b1;
  a.dx_f32 = dx_dtype == LTHM_F32;
  a.dXf = (float*)dX; a.dXb = (bf16_t*)dX;
  a.M = M; a.HID = HID;
  hipStream_t s = (hipStream_t)stream;
  constexpr int NW = MLP_BWDX_NW;
  const int grid = pl.grid;
  if (D == 256) hipLaunchKernelGGL((mlp_bwdx_k<256, NW>), dim3(grid), dim3(64 * NW), 0, s, a);
  else hipLaunchKernelGGL((mlp_bwdx_k<128, NW>), dim3(grid), dim3(64 * NW), 0, s, a);
  LTHM_CHECK_LAUNCH();
  return 0;
}

extern "C" int lthm_mlp_bwd_hidden(const void* X, const void* dY, int64_t M, int32_t D, int32_t HID, const void* W1,
                                   const float* b1, const void* W2T, void* G, void* dP, void* stream) {
  lthm_mlp_plan_out pl;
  if (const int rc = lthm_mlp_plan(LTHM_MLP_BWD_HIDDEN, M, D, HID, cu_count(), &pl)) return rc;
  if (M == 0) return 0;  // nothing to do: an empty tensor's pointers may be null
  LTHM_REQUIRE(X && dY && W1 && W2T && G && dP);
  LTHM_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)dY % 16) == 0 && ((uintptr_t)W1 % 16) == 0 &&
               ((uintptr_t)W2T % 16) == 0 && ((uintptr_t)b1 % 16) == 0 && ((uintptr_t)G % 16) == 0 &&
               ((uintptr_t)dP % 16) == 0);
  MlpBwdArgs a{};
  a.X = (const bf16_t*)X; a.dY = (const bf16_t*)dY; a.W1 = (const bf16_t*)W1; a.W2T = (const bf16_t*)W2T;
  a.b1 = b1; a.G = (bf16_t*)G; a.dP = (bf16_t*)dP;
  a.M = M; a.HID = HID;
  hipStream_t s = (hipStream_t)stream;
  constexpr int NW = MLP_BWDP_NW;
  const int grid = pl.grid;
  if (D == 256) hipLaunchKernelGGL((mlp_bwdp_k<256, NW>), dim3(grid), dim3(64 * NW), 0, s, a);
  else hipLaunchKernelGGL((mlp_bwdp_k<128, NW>), dim3(grid), dim3(64 * NW), 0, s, a);
  LTHM_CHECK_LAUNCH();
  return 0;
}
