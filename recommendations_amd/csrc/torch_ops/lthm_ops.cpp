// TORCH_LIBRARY(lthm) — the scriptable op layer over the C ABI of include/lthm.h.
//
// the reference's boundary is the PyTorch module API, and its offline
// caller scripts the item-embedding module (embedding_module_gen.py:191-192,
// `torch.jit.script(final_model)`) and the LTHM encoder loads it again
// (models/lthm/sequence/encoder.py:29).  The ctypes path in kernels.py cannot be
// compiled by TorchScript; these dispatcher ops can.  Each op checks its operands on
// the host (TORCH_CHECK -> RuntimeError, the reference's error style), allocates its
// outputs through the torch caching allocator and launches the same gfx950 kernel the
// eager path launches, on torch's current HIP stream.  Only the CUDA (= HIP on ROCm)
// and Autograd dispatch keys are implemented: a CPU tensor raises (no CPU fallback).
//
//   lthm::kshift        KShiftEmbedding.forward     commons/layers.py:152-172 (+ dense backward)
//   lthm::kshift_rows   KShiftEmbedding.get_row_idx commons/layers.py:174-185
//   lthm::gather_pool   the C3 row-sharded pool     
//   lthm::mlp_chain     MLP + QuickGELU             commons/layers.py:65-81 (+ backward)
//   lthm::activation    QuickGELU / GELU(tanh)      commons/layers.py:9-11 (+ backward)
//   lthm::item_artifact ModelWrapper.forward        embedding_module_gen.py:32-41 (fused)
//   lthm::retrieve_topk full-catalogue top-K        (build-defined, csrc/retrieve.hip; forward only)
//   lthm::retrieve_topk_excl  the same without each query's listed rows
//   lthm::retrieve_topk_group the same for users of several queries, by the best score over them
//   lthm::retrieve_topk_tags  any of the above among the rows whose tag word passes the query's filter
//   lthm::retrieve_topk_after any of the above strictly behind a (score, row) cursor per query
//   lthm::retrieve_topk_bias  any of the above on the score fma(weight[q], bias[row], dot)
//   lthm::retrieve_topk_deep  any of the above with k up to 1024, from one scan of the catalogue
//   lthm::retrieve_merge_shards  the k first of the union of S sorted (score, id) lists per query
//   lthm::retrieve_ivf_topk_shards the scan of S clustered catalogues of one device in one call, merged
//   lthm::retrieve_ivf_topk      the scan of a clustered catalogue: each query visits the lists it probes
//   lthm::retrieve_ivf_topk_filt the same with a tag filter, a score prior and an (score, id) cursor per query
//   lthm::retrieve_ivf_topk_deep the same with k up to 1,024 (lthm_retrieve_ivf_topk_deep)
//   lthm::retrieve_ivf_topk_group retrieve_ivf_topk_filt for users of G <= 8 queries each: the best score over them
//   lthm::retrieve_diversify     greedy MMR selection of k out of a pool per query, with a cap per group
//   lthm::quantize_catalogue_q8, lthm::retrieve_q8_topk, lthm::retrieve_rescore
//                                an e4m3 catalogue, its shortlist scan and the exact re-scoring of a list
#include <ATen/hip/HIPContext.h>
#include <torch/autograd.h>
#include <torch/library.h>

#include <tuple>
#include <vector>

#include "../../../include/lthm.h"

namespace {

using at::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::tensor_list;

void* cur_stream() { return reinterpret_cast<void*>(at::hip::getCurrentHIPStream().stream()); }

int32_t dcode(const Tensor& t) {
  if (t.scalar_type() == at::kFloat) return LTHM_F32;
  if (t.scalar_type() == at::kBFloat16) return LTHM_BF16;
  TORCH_CHECK(false, "lthm ops take float32 or bfloat16 tensors, got ", t.scalar_type());
}

void on_gpu(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "lthm ops run only on an MI355X (gfx950) device; ", name, " is on ", t.device(),
              ". The CPU restatement lives in oracle/ and is test infrastructure only.");
}

void hip_ok(int rc, const char* fn) { TORCH_CHECK(rc == 0, fn, " failed with hip error ", rc); }

const void* cptr(const c10::optional<Tensor>& t) { return t.has_value() && t->defined() ? t->data_ptr() : nullptr; }

Tensor cast_to(const Tensor& x, at::ScalarType dt) {
  if (x.scalar_type() == dt) return x;
  auto xc = x.contiguous();
  auto out = at::empty(xc.sizes(), xc.options().dtype(dt));
  hip_ok(lthm_cast(xc.data_ptr(), dcode(xc), out.data_ptr(), dcode(out), xc.numel(), cur_stream()), "lthm_cast");
  return out;
}

// ---------------------------------------------------------------- KShift
void check_kshift(const Tensor& ids, const Tensor& weight, int64_t P, int64_t K, int64_t F) {
  on_gpu(ids, "ids");
  on_gpu(weight, "weight");
  TORCH_CHECK(ids.scalar_type() == at::kLong, "ids must be int64, got ", ids.scalar_type());
  TORCH_CHECK(P > 0 && K > 0 && K <= 64 && F >= 1, "bad KShift config P=", P, " K=", K, " F=", F);
  TORCH_CHECK(weight.dim() == 2 && weight.size(0) == F * P, "weight must be [F*P, D] = [", F * P, ", D], got ",
              weight.sizes());
  TORCH_CHECK(ids.numel() % F == 0, "ids.numel()=", ids.numel(), " is not a multiple of F=", F);
  TORCH_CHECK(weight.is_contiguous(), "weight must be contiguous");
}

std::tuple<Tensor, Tensor> kshift_fwd_impl(const Tensor& ids_, const Tensor& weight, int64_t P, int64_t K,
                                           int64_t mode, int64_t F, c10::optional<at::ScalarType> out_dtype,
                                           bool want_norms) {
  check_kshift(ids_, weight, P, K, F);
  auto ids = ids_.contiguous();
  const int64_t D = weight.size(1);
  auto shape = ids.sizes().vec();
  shape.push_back(D);
  auto out = at::empty(shape, weight.options().dtype(out_dtype.value_or(weight.scalar_type())));
  Tensor norms;
  if (mode == LTHM_KSHIFT_NORMALIZE && want_norms) norms = at::empty(ids.sizes(), weight.options().dtype(at::kFloat));
  hip_ok(lthm_kshift_fwd_multi(ids.data_ptr<int64_t>(), ids.numel() / F, (int32_t)F, weight.data_ptr(), dcode(weight),
                               P, (int32_t)D, (int32_t)K, (int32_t)mode, out.data_ptr(), dcode(out),
                               norms.defined() ? norms.data_ptr<float>() : nullptr, cur_stream()),
         "lthm_kshift_fwd_multi");
  return {out, norms};
}

Tensor kshift_cuda(const Tensor& ids, const Tensor& weight, int64_t P, int64_t K, int64_t mode, int64_t F,
                   c10::optional<at::ScalarType> out_dtype) {
  return std::get<0>(kshift_fwd_impl(ids, weight, P, K, mode, F, out_dtype, false));
}

class KShiftFunction : public torch::autograd::Function<KShiftFunction> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& ids, const Tensor& weight, int64_t P, int64_t K,
                        int64_t mode, int64_t F, c10::optional<at::ScalarType> out_dtype) {
    at::AutoDispatchBelowADInplaceOrView guard;
    auto [out, norms] = kshift_fwd_impl(ids, weight, P, K, mode, F, out_dtype, true);
    ctx->save_for_backward({ids.contiguous(), mode == LTHM_KSHIFT_NORMALIZE ? out : Tensor(), norms});
    ctx->saved_data["P"] = P;
    ctx->saved_data["K"] = K;
    ctx->saved_data["mode"] = mode;
    ctx->saved_data["F"] = F;
    ctx->saved_data["rows"] = weight.size(0);
    ctx->saved_data["D"] = weight.size(1);
    ctx->saved_data["wdtype"] = weight.scalar_type();
    return out;
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
    auto saved = ctx->get_saved_variables();
    const Tensor& ids = saved[0];
    const Tensor& out = saved[1];
    const Tensor& norms = saved[2];
    const int64_t P = ctx->saved_data["P"].toInt(), K = ctx->saved_data["K"].toInt();
    const int64_t mode = ctx->saved_data["mode"].toInt(), F = ctx->saved_data["F"].toInt();
    const int64_t rows = ctx->saved_data["rows"].toInt(), D = ctx->saved_data["D"].toInt();
    const auto wdt = ctx->saved_data["wdtype"].toScalarType();
    auto gy = grads[0].contiguous();
    TORCH_CHECK(gy.numel() == ids.numel() * D, "grad has ", gy.numel(), " elements, expected ", ids.numel() * D);
    auto dW = at::empty({rows, D}, gy.options().dtype(at::kFloat));
    hip_ok(lthm_fill_f32(dW.data_ptr<float>(), 0.f, dW.numel(), cur_stream()), "lthm_fill_f32");
    hip_ok(lthm_kshift_bwd_dense(ids.data_ptr<int64_t>(), ids.numel() / F, (int32_t)F, gy.data_ptr(), dcode(gy),
                                 out.defined() ? out.data_ptr() : nullptr, out.defined() ? dcode(out) : LTHM_F32,
                                 norms.defined() ? norms.data_ptr<float>() : nullptr, P, (int32_t)D, (int32_t)K,
                                 (int32_t)mode, dW.data_ptr<float>(), cur_stream()),
           "lthm_kshift_bwd_dense");
    if (wdt != at::kFloat) dW = cast_to(dW, wdt);
    return {Tensor(), dW, Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor kshift_autograd(const Tensor& ids, const Tensor& weight, int64_t P, int64_t K, int64_t mode, int64_t F,
                       c10::optional<at::ScalarType> out_dtype) {
  return KShiftFunction::apply(ids, weight, P, K, mode, F, out_dtype);
}

Tensor kshift_rows_cuda(const Tensor& ids_, int64_t P, int64_t K) {
  on_gpu(ids_, "ids");
  TORCH_CHECK(ids_.scalar_type() == at::kLong, "ids must be int64");
  TORCH_CHECK(P > 0 && K > 0 && K <= 64, "bad KShift config P=", P, " K=", K);
  auto ids = ids_.contiguous();
  auto shape = ids.sizes().vec();
  shape.push_back(K);
  auto rows = at::empty(shape, ids.options());
  hip_ok(lthm_kshift_rows(ids.data_ptr<int64_t>(), ids.numel(), P, (int32_t)K, rows.data_ptr<int64_t>(),
                          cur_stream()),
         "lthm_kshift_rows");
  return rows;
}

Tensor gather_pool_cuda(const Tensor& rows_, const Tensor& W, int64_t mode, at::ScalarType out_dtype) {
  on_gpu(rows_, "rows");
  on_gpu(W, "W");
  TORCH_CHECK(rows_.scalar_type() == at::kLong && rows_.dim() == 2, "rows must be int64 [n, K]");
  TORCH_CHECK(W.dim() == 2 && W.is_contiguous(), "W must be a contiguous [R, D] table");
  const int64_t n = rows_.size(0), K = rows_.size(1), D = W.size(1);
  TORCH_CHECK(K > 0 && K <= 64, "K must be in 1..64");
  auto rows = rows_.contiguous();
  auto out = at::empty({n, D}, W.options().dtype(out_dtype));
  hip_ok(lthm_gather_pool(rows.data_ptr<int64_t>(), n, (int32_t)K, W.data_ptr(), dcode(W), W.size(0), (int32_t)D,
                          (int32_t)mode, out.data_ptr(), dcode(out), nullptr, cur_stream()),
         "lthm_gather_pool");
  return out;
}

// ---------------------------------------------------------------- GEMM chain (MLP)
// split-K factor of kernels._splits_for (same kernel choice => same summation order as eager)
int64_t splits_for(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  if (tiles >= 256 || K < 4096) return 1;
  const int64_t s = std::max<int64_t>(1, std::min<int64_t>(512 / tiles, K / 2048));
  const int64_t tiles256 = ((M + 255) / 256) * ((N + 255) / 256);
  return std::max(s, std::min<int64_t>(256 / tiles256, K / 256));
}

// C = epi(A . B) with A [M, K] (a_kc) or [K, M]; B [N, K] (b_kc) or [K, N]; all bf16, C out_dtype.
Tensor gemm(const Tensor& A, const Tensor& B, int64_t M, int64_t N, int64_t K, bool a_kc, bool b_kc,
            at::ScalarType out_dtype, const Tensor& bias, int32_t act, const Tensor& aux, const Tensor& aux_out,
            int64_t splits = 1) {
  auto C = at::empty({M, N}, A.options().dtype(out_dtype));
  lthm_gemm_desc d{};
  d.A = A.data_ptr();
  d.B = B.data_ptr();
  d.C = C.data_ptr();
  d.M = M;
  d.N = N;
  d.K = K;
  d.lda = a_kc ? K : M;
  d.ldb = b_kc ? K : N;
  d.ldc = N;
  d.sA = d.sB = 0;
  d.sC = M * N;
  d.batch = 1;
  d.a_kcontig = a_kc;
  d.b_kcontig = b_kc;
  d.out_dtype = dcode(C);
  d.alpha = 1.f;
  d.act = act;
  d.bias = bias.defined() ? bias.data_ptr<float>() : nullptr;
  d.aux = aux.defined() ? aux.data_ptr() : nullptr;
  d.aux_out = aux_out.defined() ? aux_out.data_ptr() : nullptr;
  d.ldaux = N;
  d.res1_dtype = d.res2_dtype = LTHM_F32;
  d.ldr1 = d.ldr2 = N;
  d.splits = (int32_t)splits;
  Tensor ws;
  if (splits > 1) {
    ws = at::empty({splits * M * N}, A.options().dtype(at::kFloat));
    d.workspace = ws.data_ptr<float>();
    d.workspace_bytes = (size_t)ws.numel() * 4;
  }
  d.ab_dtype = LTHM_BF16;
  hip_ok(lthm_gemm(&d, cur_stream()), "lthm_gemm");
  return C;
}

int32_t act_grad_of(int64_t act) {
  if (act == LTHM_ACT_GELU) return LTHM_ACT_GELU_GRAD;
  if (act == LTHM_ACT_QGELU) return LTHM_ACT_QGELU_GRAD;
  return LTHM_ACT_NONE;
}

void check_chain(const Tensor& x, const std::vector<Tensor>& ws, const std::vector<c10::optional<Tensor>>& bs,
                 const std::vector<int64_t>& acts) {
  on_gpu(x, "x");
  TORCH_CHECK(!ws.empty() && ws.size() == bs.size() && ws.size() == acts.size(),
              "mlp_chain: weights, biases and acts must have one entry per Linear");
  int64_t din = x.size(-1);
  for (size_t i = 0; i < ws.size(); ++i) {
    on_gpu(ws[i], "weight");
    TORCH_CHECK(ws[i].dim() == 2 && ws[i].size(1) == din, "Linear ", i, ": weight ", ws[i].sizes(),
                " does not take ", din, " inputs");
    if (bs[i].has_value() && bs[i]->defined())
      TORCH_CHECK(bs[i]->numel() == ws[i].size(0) && bs[i]->scalar_type() == at::kFloat, "Linear ", i,
                  ": bias must be f32 [", ws[i].size(0), "]");
    TORCH_CHECK(acts[i] == LTHM_ACT_NONE || acts[i] == LTHM_ACT_GELU || acts[i] == LTHM_ACT_QGELU,
                "mlp_chain: act must be none, GELU or QuickGELU");
    din = ws[i].size(0);
  }
}

// forward of kernels.MLPChainFn: bf16 operands, bias + act fused, last layer f32 (out_f32) or bf16
Tensor mlp_chain_fwd(const Tensor& x, const std::vector<Tensor>& ws, const std::vector<c10::optional<Tensor>>& bs,
                     const std::vector<int64_t>& acts, bool out_f32, std::vector<Tensor>* hs, std::vector<Tensor>* pres,
                     std::vector<Tensor>* wsb) {
  check_chain(x, ws, bs, acts);
  const int64_t din = x.size(-1), M = x.numel() / din;
  Tensor h = cast_to(x.contiguous().view({M, din}), at::kBFloat16);
  const size_t n = ws.size();
  for (size_t i = 0; i < n; ++i) {
    const bool last = i + 1 == n;
    Tensor wb = cast_to(ws[i].detach().contiguous(), at::kBFloat16);
    const int64_t N = wb.size(0), K = wb.size(1);
    Tensor pre;
    if (acts[i] != LTHM_ACT_NONE) pre = at::empty({M, N}, h.options().dtype(at::kBFloat16));
    Tensor b = (bs[i].has_value() && bs[i]->defined()) ? bs[i]->detach().contiguous() : Tensor();
    if (hs) hs->push_back(h);
    h = gemm(h, wb, M, N, K, true, true, (last && out_f32) ? at::kFloat : at::kBFloat16, b, (int32_t)acts[i],
             Tensor(), pre);
    if (pres) pres->push_back(pre);
    if (wsb) wsb->push_back(wb);
  }
  auto shape = x.sizes().vec();
  shape.back() = h.size(1);
  return h.view(shape);
}

std::vector<c10::optional<Tensor>> opt_list(at::TensorList biases) {
  std::vector<c10::optional<Tensor>> bs;
  for (const auto& b : biases) bs.push_back(b);
  return bs;
}

Tensor mlp_chain_cuda(const Tensor& x, at::TensorList weights, at::TensorList biases, at::IntArrayRef acts,
                      bool out_f32) {
  auto bs = opt_list(biases);
  return mlp_chain_fwd(x, weights.vec(), bs, acts.vec(), out_f32, nullptr, nullptr, nullptr);
}

class MLPChainFunction : public torch::autograd::Function<MLPChainFunction> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& x, at::TensorList weights, at::TensorList biases,
                        at::IntArrayRef acts, bool out_f32) {
    at::AutoDispatchBelowADInplaceOrView guard;
    auto bs = opt_list(biases);
    std::vector<Tensor> hs, pres, wsb;
    Tensor y = mlp_chain_fwd(x, weights.vec(), bs, acts.vec(), out_f32, &hs, &pres, &wsb);
    const size_t n = weights.size();
    std::vector<Tensor> save;
    for (auto& t : hs) save.push_back(t);
    for (auto& t : pres) save.push_back(t);
    for (auto& t : wsb) save.push_back(t);
    ctx->save_for_backward(save);
    std::vector<int64_t> has_b;
    for (auto& b : bs) has_b.push_back(b.has_value() && b->defined());
    ctx->saved_data["n"] = (int64_t)n;
    ctx->saved_data["acts"] = acts.vec();
    ctx->saved_data["has_b"] = has_b;
    ctx->saved_data["xdt"] = x.scalar_type();
    ctx->saved_data["xshape"] = x.sizes().vec();
    return y;
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
    auto saved = ctx->get_saved_variables();
    const int64_t n = ctx->saved_data["n"].toInt();
    const auto acts = ctx->saved_data["acts"].toIntVector();
    const auto has_b = ctx->saved_data["has_b"].toIntVector();
    const auto xdt = ctx->saved_data["xdt"].toScalarType();
    const auto xshape = ctx->saved_data["xshape"].toIntVector();
    std::vector<Tensor> hs(saved.begin(), saved.begin() + n), pres(saved.begin() + n, saved.begin() + 2 * n),
        wsb(saved.begin() + 2 * n, saved.begin() + 3 * n);
    Tensor g = grads[0].contiguous();
    const int64_t M = hs[0].size(0);
    Tensor gb = cast_to(g.view({M, g.size(-1)}), at::kBFloat16);
    std::vector<Tensor> dW(n), db(n);
    Tensor dx;
    for (int64_t i = n - 1; i >= 0; --i) {
      const int64_t N = wsb[i].size(0), K = wsb[i].size(1);
      // dW = gb^T h  (both K-strided over the M token rows), f32 [N, K]
      dW[i] = gemm(gb, hs[i], N, K, M, false, false, at::kFloat, Tensor(), LTHM_ACT_NONE, Tensor(), Tensor(),
                   splits_for(N, K, M));
      if (has_b[i]) {
        db[i] = at::empty({N}, gb.options().dtype(at::kFloat));
        hip_ok(lthm_colsum(gb.data_ptr(), LTHM_BF16, M, N, N, db[i].data_ptr<float>(), 0, cur_stream()),
               "lthm_colsum");
      }
      if (i > 0) {
        gb = gemm(gb, wsb[i], M, K, N, true, false, at::kBFloat16, Tensor(), act_grad_of(acts[i - 1]), pres[i - 1],
                  Tensor());
      } else {
        dx = gemm(gb, wsb[0], M, K, N, true, false, xdt == at::kFloat ? at::kFloat : at::kBFloat16, Tensor(),
                  LTHM_ACT_NONE, Tensor(), Tensor());
      }
    }
    // one gradient slot per input variable: x, each weight, each bias (TensorLists expand), acts, out_f32
    tensor_list out{dx.view(xshape)};
    for (auto& t : dW) out.push_back(t);
    for (int64_t i = 0; i < n; ++i) out.push_back(has_b[i] ? db[i] : Tensor());
    out.push_back(Tensor());
    out.push_back(Tensor());
    return out;
  }
};

Tensor mlp_chain_autograd(const Tensor& x, at::TensorList weights, at::TensorList biases, at::IntArrayRef acts,
                          bool out_f32) {
  return MLPChainFunction::apply(x, weights, biases, acts, out_f32);
}

// ---------------------------------------------------------------- elementwise activation (QuickGELU / GELU)
Tensor activation_impl(const Tensor& x_, const Tensor& dy_, int64_t act) {
  on_gpu(x_, "x");
  TORCH_CHECK(act == LTHM_ACT_GELU || act == LTHM_ACT_QGELU, "activation: act must be GELU (1) or QuickGELU (2)");
  auto x = x_.contiguous();
  Tensor dy = dy_.defined() ? cast_to(dy_.contiguous(), x.scalar_type()) : Tensor();
  auto y = at::empty_like(x);
  hip_ok(lthm_activation(x.data_ptr(), dy.defined() ? dy.data_ptr() : nullptr, y.data_ptr(), dcode(x), x.numel(),
                         (int32_t)act, cur_stream()),
         "lthm_activation");
  return y;
}

Tensor activation_cuda(const Tensor& x, int64_t act) { return activation_impl(x, Tensor(), act); }

class ActivationFunction : public torch::autograd::Function<ActivationFunction> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& x, int64_t act) {
    at::AutoDispatchBelowADInplaceOrView guard;
    ctx->save_for_backward({x});
    ctx->saved_data["act"] = act;
    return activation_impl(x, Tensor(), act);
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
    auto x = ctx->get_saved_variables()[0];
    return {activation_impl(x, grads[0], ctx->saved_data["act"].toInt()), Tensor()};
  }
};

Tensor activation_autograd(const Tensor& x, int64_t act) { return ActivationFunction::apply(x, act); }

// ---------------------------------------------------------------- fused item artifact (forward only)
Tensor item_artifact_cuda(const Tensor& ids_, const Tensor& W, int64_t K, int64_t mode, const Tensor& Wm, int64_t Km,
                          const Tensor& W1, const Tensor& b1, const Tensor& w2, const Tensor& b2,
                          at::ScalarType out_dtype) {
  for (auto* t : {&ids_, &W, &Wm, &W1, &b1, &w2, &b2}) on_gpu(*t, "operand");
  TORCH_CHECK(ids_.scalar_type() == at::kLong, "ids must be int64");
  TORCH_CHECK(W.dim() == 2 && Wm.dim() == 2 && W.is_contiguous() && Wm.is_contiguous(), "tables must be contiguous 2-D");
  TORCH_CHECK(Wm.scalar_type() == at::kFloat && W1.scalar_type() == at::kFloat && b1.scalar_type() == at::kFloat &&
                  w2.scalar_type() == at::kFloat && b2.scalar_type() == at::kFloat,
              "mask model tensors must be f32");
  const int64_t Dm = Wm.size(1), H1 = W1.size(0);
  TORCH_CHECK(Dm % 4 == 0 && Dm <= 16 && H1 <= 256 && W1.size(1) == Dm && b1.numel() == H1 && w2.numel() == H1 &&
                  b2.numel() == 1,
              "mask model must be KShift(Dm % 4 == 0, Dm <= 16) -> Linear(Dm, H1 <= 256) -> Linear(H1, 1)");
  TORCH_CHECK(K > 0 && K <= 64 && Km > 0 && Km <= 64, "num_shifts must be in 1..64");
  auto ids = ids_.contiguous();
  const int64_t D = W.size(1);
  auto shape = ids.sizes().vec();
  shape.push_back(D);
  auto out = at::empty(shape, W.options().dtype(out_dtype));
  auto W1c = W1.contiguous(), b1c = b1.contiguous(), w2c = w2.contiguous(), b2c = b2.contiguous();
  hip_ok(lthm_item_artifact_fwd(ids.data_ptr<int64_t>(), ids.numel(), W.data_ptr(), dcode(W), W.size(0), (int32_t)D,
                                (int32_t)K, (int32_t)mode, Wm.data_ptr<float>(), Wm.size(0), (int32_t)Dm, (int32_t)Km,
                                W1c.data_ptr<float>(), b1c.data_ptr<float>(), (int32_t)H1, w2c.data_ptr<float>(),
                                b2c.data_ptr<float>(), out.data_ptr(), dcode(out), cur_stream()),
         "lthm_item_artifact_fwd");
  return out;
}

// ---------------------------------------------------------------- full-catalogue top-K (forward only)
// Every scan op.  q [U, G, 128]: an item's score is its best over the user's G <= 8 queries (the ops
// unsqueeze a 2-D q to groups of one); exclude_rows is one list per user (int32 [U, X]) or None;
// tags (int32 [N]) and filter (int32 [U, 3]) are both null or both given, as are the cursor's two
std::tuple<Tensor, Tensor> retrieve_topk_group_impl(const Tensor& q_, const Tensor& items_, int64_t k, bool normalize_q,
                                                    const c10::optional<Tensor>& exclude_rows, const Tensor* tags_,
                                                    const Tensor* filter_, const Tensor* after_scores_ = nullptr,
                                                    const Tensor* after_rows_ = nullptr, const Tensor* bias_ = nullptr,
                                                    const Tensor* bias_weight_ = nullptr, bool deep = false) {
  on_gpu(q_, "q");
  on_gpu(items_, "items");
  TORCH_CHECK(items_.dim() == 2 && items_.size(1) == 128 && items_.scalar_type() == at::kBFloat16,
              "items must be a bf16 [N, 128] catalogue");
  TORCH_CHECK(q_.dim() == 3 && q_.size(2) == 128, "q must be [Q, 128] or [U, G, 128]");
  TORCH_CHECK(q_.size(1) >= 1 && q_.size(1) <= 8, "retrieve_topk_group takes 1..8 queries per user, got ", q_.size(1));
  // the k cap is the op's: 1024 for the deep op, 128 for the others
  TORCH_CHECK(k >= 1 && k <= (deep ? 1024 : 128), "k must be in 1..", deep ? 1024 : 128, ", got ", k);
  TORCH_CHECK(items_.size(0) >= 1 && q_.size(0) >= 1, "retrieve_topk_group takes a non-empty catalogue and user set");
  auto q = q_.contiguous(), items = items_.contiguous();
  const int64_t U = q.size(0), G = q.size(1), N = items.size(0);
  Tensor xr;
  const bool excl = exclude_rows.has_value() && exclude_rows->defined();
  if (excl) {
    on_gpu(*exclude_rows, "exclude_rows");
    TORCH_CHECK(exclude_rows->scalar_type() == at::kInt && exclude_rows->dim() == 2 && exclude_rows->size(0) == U,
                "exclude_rows must be int32 [Q, X], one list per query (per user for a 3-D q)");
    TORCH_CHECK(exclude_rows->size(1) >= 1 && exclude_rows->size(1) <= 1024,
                "exclude_rows takes 1..1024 rows per query (per user for a 3-D q), got ", exclude_rows->size(1));
    TORCH_CHECK(exclude_rows->device() == q.device(), "exclude_rows must be on the queries' device");
    xr = exclude_rows->contiguous();
  }
  Tensor tg, tf;
  if (tags_) {
    on_gpu(*tags_, "tags");
    on_gpu(*filter_, "tag_filter");
    TORCH_CHECK(tags_->scalar_type() == at::kInt && tags_->dim() == 1 && tags_->size(0) == N,
                "tags must be int32 [N], one word per catalogue row");
    TORCH_CHECK(filter_->scalar_type() == at::kInt && filter_->dim() == 2 && filter_->size(0) == U && filter_->size(1) == 3,
                "tag_filter must be int32 [Q, 3] = (all, any, none), one row per query (per user for a 3-D q)");
    TORCH_CHECK(tags_->device() == items.device() && filter_->device() == items.device(),
                "tags and tag_filter must be on the catalogue's device");
    tg = tags_->contiguous();
    tf = filter_->contiguous();
  }
  Tensor cs, cr;
  if (after_scores_) {
    on_gpu(*after_scores_, "after_scores");
    on_gpu(*after_rows_, "after_rows");
    TORCH_CHECK(after_scores_->scalar_type() == at::kFloat && after_scores_->dim() == 1 && after_scores_->size(0) == U,
                "after_scores must be f32 [Q], one cursor per query (per user for a 3-D q)");
    TORCH_CHECK(after_rows_->scalar_type() == at::kInt && after_rows_->dim() == 1 && after_rows_->size(0) == U,
                "after_rows must be int32 [Q], one cursor per query (per user for a 3-D q)");
    TORCH_CHECK(after_scores_->device() == q.device() && after_rows_->device() == q.device(),
                "after_scores and after_rows must be on the queries' device");
    cs = after_scores_->contiguous();
    cr = after_rows_->contiguous();
  }
  Tensor bs, bw;
  if (bias_) {
    on_gpu(*bias_, "bias");
    TORCH_CHECK(bias_->scalar_type() == at::kFloat && bias_->dim() == 1 && bias_->size(0) == N,
                "bias must be f32 [N], one word per catalogue row");
    TORCH_CHECK(bias_->device() == items.device(), "bias must be on the catalogue's device");
    bs = bias_->contiguous();
    if (bias_weight_) {
      on_gpu(*bias_weight_, "bias_weight");
      TORCH_CHECK(bias_weight_->scalar_type() == at::kFloat && bias_weight_->dim() == 1 && bias_weight_->size(0) == U,
                  "bias_weight must be f32 [Q], one weight per query (per user for a 3-D q)");
      TORCH_CHECK(bias_weight_->device() == q.device(), "bias_weight must be on the queries' device");
      bw = bias_weight_->contiguous();
    }
  }
  const int64_t need = lthm_retrieve_deep_ws_bytes(U, (int32_t)G, N, (int32_t)k, 0, excl ? xr.size(1) : 0);
  TORCH_CHECK(need >= 0, "retrieve_topk_group: unsupported sizes U=", U, " G=", G, " N=", N);
  auto scores = at::empty({U, k}, q.options().dtype(at::kFloat));
  auto rows = at::empty({U, k}, q.options().dtype(at::kInt));
  auto ws = at::empty({need}, q.options().dtype(at::kByte));
  lthm_retrieve_desc d = {};
  d.items = items.data_ptr();
  d.q = q.data_ptr();
  d.scores = scores.data_ptr<float>();
  d.rows = rows.data_ptr<int32_t>();
  d.workspace = ws.data_ptr();
  d.ws_bytes = need;
  d.Q = U;
  d.N = N;
  d.k = (int32_t)k;
  d.q_dtype = dcode(q);
  d.normalize_q = normalize_q ? 1 : 0;
  // one call, lthm_retrieve_topk_deep, with the parts that are present: it picks the kernels by k and G
  lthm_retrieve_excl x = {};
  if (excl) {
    x.rows = xr.data_ptr<int32_t>();
    x.X = xr.size(1);
  }
  lthm_retrieve_group g = {};
  g.G = (int32_t)G;
  lthm_retrieve_tags t = {};
  if (tags_) {
    t.tags = tg.data_ptr<int32_t>();
    t.filter = tf.data_ptr<int32_t>();
  }
  lthm_retrieve_cursor c = {};
  if (after_scores_) {
    c.after_score = cs.data_ptr<float>();
    c.after_row = cr.data_ptr<int32_t>();
  }
  lthm_retrieve_bias b = {};
  if (bias_) {
    b.bias = bs.data_ptr<float>();
    b.weight = bias_weight_ ? bw.data_ptr<float>() : nullptr;
  }
  hip_ok(lthm_retrieve_topk_deep(&d, excl ? &x : nullptr, &g, tags_ ? &t : nullptr, after_scores_ ? &c : nullptr,
                                 bias_ ? &b : nullptr, cur_stream()),
         "lthm_retrieve_topk_deep");
  return std::make_tuple(scores, rows);
}

std::tuple<Tensor, Tensor> retrieve_topk_group_cuda(const Tensor& q, const Tensor& items, int64_t k, bool normalize_q,
                                                    const c10::optional<Tensor>& exclude_rows) {
  return retrieve_topk_group_impl(q, items, k, normalize_q, exclude_rows, nullptr, nullptr);
}

// q [Q, 128]: a group of one query
std::tuple<Tensor, Tensor> retrieve_topk_cuda(const Tensor& q, const Tensor& items, int64_t k, bool normalize_q) {
  TORCH_CHECK(q.dim() == 2, "q must be [Q, 128]");
  return retrieve_topk_group_impl(q.unsqueeze(1), items, k, normalize_q, c10::nullopt, nullptr, nullptr);
}

std::tuple<Tensor, Tensor> retrieve_topk_excl_cuda(const Tensor& q, const Tensor& items, int64_t k, bool normalize_q,
                                                   const Tensor& exclude_rows) {
  TORCH_CHECK(q.dim() == 2, "q must be [Q, 128]");
  return retrieve_topk_group_impl(q.unsqueeze(1), items, k, normalize_q, exclude_rows, nullptr, nullptr);
}

// q [Q, 128] or [U, G, 128]; a 2-D q is a group of one query
std::tuple<Tensor, Tensor> retrieve_topk_tags_cuda(const Tensor& q, const Tensor& items, int64_t k, bool normalize_q,
                                                   const c10::optional<Tensor>& exclude_rows, const Tensor& tags,
                                                   const Tensor& tag_filter) {
  TORCH_CHECK(q.dim() == 2 || q.dim() == 3, "q must be [Q, 128] or [U, G, 128]");
  return retrieve_topk_group_impl(q.dim() == 2 ? q.unsqueeze(1) : q, items, k, normalize_q, exclude_rows, &tags,
                                  &tag_filter);
}

// the same behind a cursor per query (per user for a 3-D q); tags and tag_filter are both given or
// both None; k in 1..128 (a longer list is several calls, each behind the last column of the one
// before)
std::tuple<Tensor, Tensor> retrieve_topk_after_cuda(const Tensor& q, const Tensor& items, int64_t k, bool normalize_q,
                                                    const c10::optional<Tensor>& exclude_rows,
                                                    const c10::optional<Tensor>& tags,
                                                    const c10::optional<Tensor>& tag_filter, const Tensor& after_scores,
                                                    const Tensor& after_rows) {
  TORCH_CHECK(q.dim() == 2 || q.dim() == 3, "q must be [Q, 128] or [U, G, 128]");
  const bool has_tags = tags.has_value() && tags->defined(), has_filter = tag_filter.has_value() && tag_filter->defined();
  TORCH_CHECK(has_tags == has_filter, "retrieve_topk_after takes tags and tag_filter together or neither");
  return retrieve_topk_group_impl(q.dim() == 2 ? q.unsqueeze(1) : q, items, k, normalize_q, exclude_rows,
                                  has_tags ? &*tags : nullptr, has_tags ? &*tag_filter : nullptr, &after_scores,
                                  &after_rows);
}

// the same on the score fma(bias_weight[q], bias[row], dot); tags and tag_filter, and after_scores
// and after_rows, are both given or both None; bias_weight None is 1 for every query
std::tuple<Tensor, Tensor> retrieve_topk_bias_cuda(const Tensor& q, const Tensor& items, int64_t k, bool normalize_q,
                                                   const c10::optional<Tensor>& exclude_rows,
                                                   const c10::optional<Tensor>& tags,
                                                   const c10::optional<Tensor>& tag_filter,
                                                   const c10::optional<Tensor>& after_scores,
                                                   const c10::optional<Tensor>& after_rows, const Tensor& bias,
                                                   const c10::optional<Tensor>& bias_weight) {
  TORCH_CHECK(q.dim() == 2 || q.dim() == 3, "q must be [Q, 128] or [U, G, 128]");
  const bool has_tags = tags.has_value() && tags->defined(), has_filter = tag_filter.has_value() && tag_filter->defined();
  TORCH_CHECK(has_tags == has_filter, "retrieve_topk_bias takes tags and tag_filter together or neither");
  const bool has_cs = after_scores.has_value() && after_scores->defined();
  const bool has_cr = after_rows.has_value() && after_rows->defined();
  TORCH_CHECK(has_cs == has_cr, "retrieve_topk_bias takes after_scores and after_rows together or neither");
  const bool has_w = bias_weight.has_value() && bias_weight->defined();
  return retrieve_topk_group_impl(q.dim() == 2 ? q.unsqueeze(1) : q, items, k, normalize_q, exclude_rows,
                                  has_tags ? &*tags : nullptr, has_tags ? &*tag_filter : nullptr,
                                  has_cs ? &*after_scores : nullptr, has_cs ? &*after_rows : nullptr, &bias,
                                  has_w ? &*bias_weight : nullptr);
}

// k in 1..1024 from one scan of the catalogue; every optional tensor may be None (tags with
// tag_filter, after_scores with after_rows, bias_weight only with bias)
std::tuple<Tensor, Tensor> retrieve_topk_deep_cuda(const Tensor& q, const Tensor& items, int64_t k, bool normalize_q,
                                                   const c10::optional<Tensor>& exclude_rows,
                                                   const c10::optional<Tensor>& tags,
                                                   const c10::optional<Tensor>& tag_filter,
                                                   const c10::optional<Tensor>& after_scores,
                                                   const c10::optional<Tensor>& after_rows,
                                                   const c10::optional<Tensor>& bias,
                                                   const c10::optional<Tensor>& bias_weight) {
  TORCH_CHECK(q.dim() == 2 || q.dim() == 3, "q must be [Q, 128] or [U, G, 128]");
  const bool has_tags = tags.has_value() && tags->defined(), has_filter = tag_filter.has_value() && tag_filter->defined();
  TORCH_CHECK(has_tags == has_filter, "retrieve_topk_deep takes tags and tag_filter together or neither");
  const bool has_cs = after_scores.has_value() && after_scores->defined();
  const bool has_cr = after_rows.has_value() && after_rows->defined();
  TORCH_CHECK(has_cs == has_cr, "retrieve_topk_deep takes after_scores and after_rows together or neither");
  const bool has_b = bias.has_value() && bias->defined();
  const bool has_w = bias_weight.has_value() && bias_weight->defined();
  TORCH_CHECK(has_b || !has_w, "retrieve_topk_deep takes a bias_weight only with a bias");
  return retrieve_topk_group_impl(q.dim() == 2 ? q.unsqueeze(1) : q, items, k, normalize_q, exclude_rows,
                                  has_tags ? &*tags : nullptr, has_tags ? &*tag_filter : nullptr,
                                  has_cs ? &*after_scores : nullptr, has_cs ? &*after_rows : nullptr,
                                  has_b ? &*bias : nullptr, has_w ? &*bias_weight : nullptr, true);
}

// scores f32 [S, Q, k], ids int64 [S, Q, k], ranks int32 [S, Q] or None: the merge of the lists that
// the shards of one catalogue return (rank: an empty tensor without ranks)
std::tuple<Tensor, Tensor, Tensor> retrieve_merge_shards_cuda(const Tensor& scores_, const Tensor& ids_,
                                                              const c10::optional<Tensor>& ranks_) {
  TORCH_CHECK(scores_.dim() == 3 && scores_.scalar_type() == at::kFloat, "scores must be f32 [S, Q, k]");
  TORCH_CHECK(ids_.scalar_type() == at::kLong && ids_.sizes() == scores_.sizes(), "ids must be int64 [S, Q, k]");
  TORCH_CHECK(ids_.device() == scores_.device(), "scores and ids must be on one device");
  const int64_t S = scores_.size(0), Q = scores_.size(1), k = scores_.size(2);
  TORCH_CHECK(S >= 1 && S <= 64, "retrieve_merge_shards takes 1..64 lists per query (got S=", S, ")");
  TORCH_CHECK(k >= 1 && k <= 1024, "retrieve_merge_shards takes k in 1..1024 (got ", k, ")");
  TORCH_CHECK(Q >= 1, "retrieve_merge_shards takes at least one query");
  const Tensor scores = scores_.contiguous(), ids = ids_.contiguous();
  const bool has_r = ranks_.has_value() && ranks_->defined();
  Tensor ranks, out_rank = at::empty({has_r ? Q : 0}, ids.options());
  if (has_r) {
    TORCH_CHECK(ranks_->scalar_type() == at::kInt && ranks_->dim() == 2 && ranks_->size(0) == S && ranks_->size(1) == Q &&
                    ranks_->device() == scores.device(),
                "ranks must be int32 [S, Q] on the scores' device");
    ranks = ranks_->contiguous();
  }
  Tensor out_scores = at::empty({Q, k}, scores.options()), out_ids = at::empty({Q, k}, ids.options());
  hip_ok(lthm_retrieve_merge_shards(scores.data_ptr<float>(), ids.data_ptr<int64_t>(),
                                    has_r ? ranks.data_ptr<int32_t>() : nullptr, (int32_t)S, Q, (int32_t)k,
                                    out_scores.data_ptr<float>(), out_ids.data_ptr<int64_t>(),
                                    has_r ? out_rank.data_ptr<int64_t>() : nullptr, cur_stream()),
         "lthm_retrieve_merge_shards");
  return {out_scores, out_ids, out_rank};
}

// S clustered catalogues of one device in one call (lthm_retrieve_ivf_topk_shards): items / row_ids /
// list_off / centroids are lists of S tensors, tags and bias lists of S tensors or empty (none); every shard
// probes its min(nprobe, L_s) nearest lists.  exclude_rows int32 [S, Q, X]; tag_filter int32 [Q, 3]; use_bias
// with bias_weight f32 [Q] or None; after_scores f32 [Q] / after_ids int64 [Q]; target_rows int32 [S, Q] with
// target_scores f32 [Q].  (scores f32 [Q, k], ids int64 [Q, k], rank int64 [Q], empty without targets)
std::tuple<Tensor, Tensor, Tensor> retrieve_ivf_topk_shards_cuda(
    const Tensor& q_, at::TensorList items, at::TensorList row_ids, at::TensorList list_off, at::TensorList centroids,
    at::TensorList tags, at::TensorList bias, int64_t nprobe, int64_t k, bool normalize_q,
    const c10::optional<Tensor>& exclude_rows, const c10::optional<Tensor>& tag_filter, bool use_bias,
    const c10::optional<Tensor>& bias_weight, const c10::optional<Tensor>& after_scores,
    const c10::optional<Tensor>& after_ids, const c10::optional<Tensor>& target_rows,
    const c10::optional<Tensor>& target_scores) {
  const int64_t S = (int64_t)items.size();
  TORCH_CHECK(S >= 1 && S <= 64, "retrieve_ivf_topk_shards takes 1..64 shards (got S=", S, ")");
  TORCH_CHECK((int64_t)row_ids.size() == S && (int64_t)list_off.size() == S && (int64_t)centroids.size() == S,
              "retrieve_ivf_topk_shards takes one row_ids, list_off and centroids tensor per shard");
  TORCH_CHECK(tags.empty() || (int64_t)tags.size() == S, "tags: one tensor per shard, or none");
  TORCH_CHECK(bias.empty() || (int64_t)bias.size() == S, "bias: one tensor per shard, or none");
  TORCH_CHECK(q_.is_cuda() && q_.dim() == 2 && q_.size(1) == 128 && q_.size(0) >= 1, "q must be a CUDA tensor [Q, 128]");
  TORCH_CHECK(q_.scalar_type() == at::kFloat || q_.scalar_type() == at::kBFloat16, "q must be f32 or bf16");
  TORCH_CHECK(nprobe >= 1 && k >= 1 && k <= 1024, "retrieve_ivf_topk_shards takes nprobe >= 1 and k in 1..1024");
  const Tensor q = q_.contiguous();
  const int64_t Q = q.size(0);
  const auto dev = q.device();
  std::vector<Tensor> keep;  // the contiguous tensors the descriptors point at
  std::vector<lthm_retrieve_ivf_shard> sh((size_t)S);
  auto held = [&](const Tensor& t, at::ScalarType ty, const char* what) {
    TORCH_CHECK(t.device() == dev && t.scalar_type() == ty, what, ": wrong device or dtype");
    keep.push_back(t.contiguous());
    return keep.back().data_ptr();
  };
  for (int64_t i = 0; i < S; ++i) {
    const int64_t N = items[i].size(0), L = centroids[i].size(0);
    TORCH_CHECK(items[i].dim() == 2 && items[i].size(1) == 128 && N >= 1, "items must be bf16 [N, 128]");
    TORCH_CHECK(centroids[i].dim() == 2 && centroids[i].size(1) == 128 && L >= 1, "centroids must be bf16 [L, 128]");
    TORCH_CHECK(row_ids[i].dim() == 1 && row_ids[i].size(0) == N, "row_ids must be int64 [N]");
    TORCH_CHECK(list_off[i].dim() == 1 && list_off[i].size(0) == L + 1, "list_off must be int64 [L + 1]");
    sh[i].items = held(items[i], at::kBFloat16, "items");
    sh[i].row_ids = (const int64_t*)held(row_ids[i], at::kLong, "row_ids");
    sh[i].list_off = (const int64_t*)held(list_off[i], at::kLong, "list_off");
    sh[i].centroids = held(centroids[i], at::kBFloat16, "centroids");
    sh[i].tags = nullptr;
    sh[i].bias = nullptr;
    if (!tags.empty()) {
      TORCH_CHECK(tags[i].dim() == 1 && tags[i].size(0) == N, "tags must be int32 [N]");
      sh[i].tags = (const int32_t*)held(tags[i], at::kInt, "tags");
    }
    if (!bias.empty()) {
      TORCH_CHECK(bias[i].dim() == 1 && bias[i].size(0) == N, "bias must be f32 [N]");
      sh[i].bias = (const float*)held(bias[i], at::kFloat, "bias");
    }
    sh[i].N = N;
    sh[i].L = L;
  }
  auto opt = [&](const c10::optional<Tensor>& t, at::ScalarType ty, std::vector<int64_t> shape, const char* what) -> void* {
    if (!t.has_value() || !t->defined()) return nullptr;
    TORCH_CHECK(t->device() == dev && t->scalar_type() == ty && t->sizes() == at::IntArrayRef(shape), what,
                ": wrong device, dtype or shape");
    keep.push_back(t->contiguous());
    return keep.back().data_ptr();
  };
  int64_t X = 0;
  if (exclude_rows.has_value() && exclude_rows->defined()) {
    TORCH_CHECK(exclude_rows->dim() == 3, "exclude_rows must be int32 [S, Q, X]");
    X = exclude_rows->size(2);
    TORCH_CHECK(X >= 1 && X <= 1024, "exclude_rows takes 1..1024 rows per query");
  }
  const int32_t* xr = (const int32_t*)opt(exclude_rows, at::kInt, {S, Q, X}, "exclude_rows");
  const int32_t* tf = (const int32_t*)opt(tag_filter, at::kInt, {Q, 3}, "tag_filter");
  TORCH_CHECK(!tf || !tags.empty(), "tag_filter takes shards with tags");
  TORCH_CHECK(!use_bias || !bias.empty(), "use_bias takes shards with a bias");
  const float* bw = (const float*)opt(bias_weight, at::kFloat, {Q}, "bias_weight");
  TORCH_CHECK(use_bias || !bw, "bias_weight takes use_bias");
  lthm_retrieve_ivf_cursor c = {};
  c.after_score = (const float*)opt(after_scores, at::kFloat, {Q}, "after_scores");
  c.after_id = (const int64_t*)opt(after_ids, at::kLong, {Q}, "after_ids");
  TORCH_CHECK((c.after_score != nullptr) == (c.after_id != nullptr), "after_scores and after_ids come together or neither");
  const int32_t* tr = (const int32_t*)opt(target_rows, at::kInt, {S, Q}, "target_rows");
  const float* ts = (const float*)opt(target_scores, at::kFloat, {Q}, "target_scores");
  TORCH_CHECK((tr != nullptr) == (ts != nullptr), "target_rows and target_scores come together or neither");
  const int64_t need = lthm_retrieve_ivf_shards_ws_bytes(sh.data(), (int32_t)S, Q, (int32_t)std::min<int64_t>(nprobe, 1 << 30),
                                                         (int32_t)k, X, c.after_score ? 1 : 0);
  TORCH_CHECK(need >= 0, "retrieve_ivf_topk_shards: unsupported sizes (the probe slots of all shards together stay within 64)");
  Tensor ws = at::empty({need}, q.options().dtype(at::kByte));
  Tensor out_scores = at::empty({Q, k}, q.options().dtype(at::kFloat)), out_ids = at::empty({Q, k}, q.options().dtype(at::kLong));
  Tensor out_rank = at::empty({tr ? Q : 0}, q.options().dtype(at::kLong));
  hip_ok(lthm_retrieve_ivf_topk_shards(sh.data(), (int32_t)S, q.data_ptr(), q.scalar_type() == at::kBFloat16 ? LTHM_BF16 : LTHM_F32,
                                       normalize_q ? 1 : 0, Q, (int32_t)std::min<int64_t>(nprobe, 1 << 30), (int32_t)k, xr, X, tf,
                                       use_bias ? 1 : 0, bw, c.after_score ? &c : nullptr, tr, ts,
                                       out_scores.data_ptr<float>(), out_ids.data_ptr<int64_t>(),
                                       tr ? out_rank.data_ptr<int64_t>() : nullptr, ws.data_ptr(), need, cur_stream()),
         "lthm_retrieve_ivf_topk_shards");
  return {out_scores, out_ids, out_rank};
}

// the scan of a clustered catalogue: items bf16 [N, 128] list-major, row_ids int64 [N], list_off int64
// [L + 1], probes int32 [Q, P] (P <= 64), exclude_rows int32 [Q, X] in the clustered row numbering or
// None; (scores f32 [Q, k], ids int64 [Q, k])
std::tuple<Tensor, Tensor> retrieve_ivf_topk_filt_cuda(
    const Tensor& q_, const Tensor& items_, const Tensor& row_ids_, const Tensor& list_off_, const Tensor& probes_,
    int64_t k, bool normalize_q, const c10::optional<Tensor>& exclude_rows, const c10::optional<Tensor>& tags_,
    const c10::optional<Tensor>& tag_filter_, const c10::optional<Tensor>& bias_,
    const c10::optional<Tensor>& bias_weight_, const c10::optional<Tensor>& after_scores_,
    const c10::optional<Tensor>& after_ids_);

std::tuple<Tensor, Tensor> retrieve_ivf_topk_cuda(const Tensor& q, const Tensor& items, const Tensor& row_ids,
                                                  const Tensor& list_off, const Tensor& probes, int64_t k,
                                                  bool normalize_q, const c10::optional<Tensor>& exclude_rows) {
  return retrieve_ivf_topk_filt_cuda(q, items, row_ids, list_off, probes, k, normalize_q, exclude_rows, c10::nullopt,
                                     c10::nullopt, c10::nullopt, c10::nullopt, c10::nullopt, c10::nullopt);
}

// the same with retrieve_topk's filters, prior and cursor on the probed rows: tags int32 [N] and bias
// f32 [N] in the clustered row numbering, tag_filter int32 [Q, 3], bias_weight f32 [Q] or None (1),
// after_scores f32 [Q] with after_ids int64 [Q]; tags with tag_filter, after_scores with after_ids,
// bias_weight only with bias.  With none of them it is retrieve_ivf_topk's call.  deep: k up to 1,024
// through lthm_retrieve_ivf_topk_deep (retrieve_ivf_topk_deep below), one call for the whole batch.
// grouped: q is [U, G, 128], G in 1..8, everything "per query" above is per user, and the call is
// lthm_retrieve_ivf_topk_group (retrieve_ivf_topk_group below), k in 1..128
static std::tuple<Tensor, Tensor> retrieve_ivf_topk_impl(
    const Tensor& q_, const Tensor& items_, const Tensor& row_ids_, const Tensor& list_off_, const Tensor& probes_,
    int64_t k, bool normalize_q, const c10::optional<Tensor>& exclude_rows, const c10::optional<Tensor>& tags_,
    const c10::optional<Tensor>& tag_filter_, const c10::optional<Tensor>& bias_,
    const c10::optional<Tensor>& bias_weight_, const c10::optional<Tensor>& after_scores_,
    const c10::optional<Tensor>& after_ids_, bool deep, bool grouped = false) {
  on_gpu(q_, "q");
  on_gpu(items_, "items");
  on_gpu(row_ids_, "row_ids");
  on_gpu(list_off_, "list_off");
  on_gpu(probes_, "probes");
  TORCH_CHECK(items_.dim() == 2 && items_.size(1) == 128 && items_.scalar_type() == at::kBFloat16,
              "items must be a bf16 [N, 128] catalogue");
  if (grouped) {
    TORCH_CHECK(q_.dim() == 3 && q_.size(2) == 128, "q must be [U, G, 128]");
    TORCH_CHECK(q_.size(1) >= 1 && q_.size(1) <= 8, "retrieve_ivf_topk_group takes 1..8 queries per user, got G=",
                q_.size(1));
  } else {
    TORCH_CHECK(q_.dim() == 2 && q_.size(1) == 128, "q must be [Q, 128]");
  }
  if (deep) {
    TORCH_CHECK(k >= 1 && k <= 1024, "retrieve_ivf_topk_deep takes k in 1..1024, got ", k);
  } else {
    TORCH_CHECK(k >= 1 && k <= 128, "k must be in 1..128, got ", k);
  }
  TORCH_CHECK(items_.size(0) >= 1 && q_.size(0) >= 1, "retrieve_ivf_topk takes a non-empty catalogue and query set");
  auto q = q_.contiguous(), items = items_.contiguous();
  const int64_t Q = q.size(0), N = items.size(0), G = grouped ? q.size(1) : 1;
  TORCH_CHECK(row_ids_.scalar_type() == at::kLong && row_ids_.dim() == 1 && row_ids_.size(0) == N,
              "row_ids must be int64 [N], one id per catalogue row");
  TORCH_CHECK(list_off_.scalar_type() == at::kLong && list_off_.dim() == 1 && list_off_.size(0) >= 2,
              "list_off must be int64 [L + 1], L >= 1");
  TORCH_CHECK(probes_.scalar_type() == at::kInt && probes_.dim() == 2 && probes_.size(0) == Q, "probes must be int32 [Q, P]");
  TORCH_CHECK(probes_.size(1) >= 1 && probes_.size(1) <= 64, "retrieve_ivf_topk takes 1..64 probes per query, got P=",
              probes_.size(1));
  TORCH_CHECK(row_ids_.device() == items.device() && list_off_.device() == items.device() &&
                  probes_.device() == items.device() && q.device() == items.device(),
              "q, row_ids, list_off and probes must be on the catalogue's device");
  auto row_ids = row_ids_.contiguous(), list_off = list_off_.contiguous(), probes = probes_.contiguous();
  const int64_t L = list_off.size(0) - 1, P = probes.size(1);
  Tensor xr;
  const bool excl = exclude_rows.has_value() && exclude_rows->defined();
  if (excl) {
    on_gpu(*exclude_rows, "exclude_rows");
    TORCH_CHECK(exclude_rows->scalar_type() == at::kInt && exclude_rows->dim() == 2 && exclude_rows->size(0) == Q,
                "exclude_rows must be int32 [Q, X]");
    TORCH_CHECK(exclude_rows->size(1) >= 1 && exclude_rows->size(1) <= 1024,
                "exclude_rows takes 1..1024 rows per query, got ", exclude_rows->size(1));
    TORCH_CHECK(exclude_rows->device() == q.device(), "exclude_rows must be on the queries' device");
    xr = exclude_rows->contiguous();
  }
  const bool has_tags = tags_.has_value() && tags_->defined(), has_filter = tag_filter_.has_value() && tag_filter_->defined();
  TORCH_CHECK(has_tags == has_filter, "retrieve_ivf_topk_filt takes tags and tag_filter together or neither");
  const bool has_b = bias_.has_value() && bias_->defined(), has_w = bias_weight_.has_value() && bias_weight_->defined();
  TORCH_CHECK(has_b || !has_w, "retrieve_ivf_topk_filt takes a bias_weight only with a bias");
  const bool has_cs = after_scores_.has_value() && after_scores_->defined();
  const bool has_ci = after_ids_.has_value() && after_ids_->defined();
  TORCH_CHECK(has_cs == has_ci, "retrieve_ivf_topk_filt takes after_scores and after_ids together or neither");
  Tensor tags, tag_filter, bias, bias_weight, after_scores, after_ids;
  if (has_tags) {
    on_gpu(*tags_, "tags");
    on_gpu(*tag_filter_, "tag_filter");
    TORCH_CHECK(tags_->scalar_type() == at::kInt && tags_->dim() == 1 && tags_->size(0) == N &&
                    tags_->device() == items.device(),
                "tags must be int32 [N] on the catalogue's device");
    TORCH_CHECK(tag_filter_->scalar_type() == at::kInt && tag_filter_->dim() == 2 && tag_filter_->size(0) == Q &&
                    tag_filter_->size(1) == 3 && tag_filter_->device() == q.device(),
                "tag_filter must be int32 [Q, 3] on the queries' device");
    tags = tags_->contiguous();
    tag_filter = tag_filter_->contiguous();
  }
  if (has_b) {
    on_gpu(*bias_, "bias");
    TORCH_CHECK(bias_->scalar_type() == at::kFloat && bias_->dim() == 1 && bias_->size(0) == N &&
                    bias_->device() == items.device(),
                "bias must be f32 [N] on the catalogue's device");
    bias = bias_->contiguous();
    if (has_w) {
      on_gpu(*bias_weight_, "bias_weight");
      TORCH_CHECK(bias_weight_->scalar_type() == at::kFloat && bias_weight_->dim() == 1 && bias_weight_->size(0) == Q &&
                      bias_weight_->device() == q.device(),
                  "bias_weight must be f32 [Q] on the queries' device");
      bias_weight = bias_weight_->contiguous();
    }
  }
  if (has_cs) {
    on_gpu(*after_scores_, "after_scores");
    on_gpu(*after_ids_, "after_ids");
    TORCH_CHECK(after_scores_->scalar_type() == at::kFloat && after_scores_->dim() == 1 && after_scores_->size(0) == Q &&
                    after_scores_->device() == q.device(),
                "after_scores must be f32 [Q] on the queries' device");
    TORCH_CHECK(after_ids_->scalar_type() == at::kLong && after_ids_->dim() == 1 && after_ids_->size(0) == Q &&
                    after_ids_->device() == q.device(),
                "after_ids must be int64 [Q] on the queries' device");
    after_scores = after_scores_->contiguous();
    after_ids = after_ids_->contiguous();
  }
  const int64_t need =
      grouped ? lthm_retrieve_ivf_group_ws_bytes(Q, (int32_t)G, N, L, (int32_t)P, (int32_t)k, excl ? xr.size(1) : 0,
                                                 has_cs ? 1 : 0)
      : deep  ? lthm_retrieve_ivf_deep_ws_bytes(Q, N, L, (int32_t)P, (int32_t)k, excl ? xr.size(1) : 0, has_cs ? 1 : 0)
              : lthm_retrieve_ivf_filt_ws_bytes(Q, N, L, (int32_t)P, (int32_t)k, excl ? xr.size(1) : 0, has_cs ? 1 : 0);
  TORCH_CHECK(need >= 0, "retrieve_ivf_topk: unsupported sizes Q=", Q, " N=", N, " L=", L, " P=", P);
  auto scores = at::empty({Q, k}, q.options().dtype(at::kFloat));
  auto ids = at::empty({Q, k}, q.options().dtype(at::kLong));
  auto ws = at::empty({need}, q.options().dtype(at::kByte));
  lthm_retrieve_excl x = {};
  if (excl) {
    x.rows = xr.data_ptr<int32_t>();
    x.X = xr.size(1);
  }
  lthm_retrieve_tags t = {};
  if (has_tags) {
    t.tags = tags.data_ptr<int32_t>();
    t.filter = tag_filter.data_ptr<int32_t>();
  }
  lthm_retrieve_bias b = {};
  if (has_b) {
    b.bias = bias.data_ptr<float>();
    b.weight = has_w ? bias_weight.data_ptr<float>() : nullptr;
  }
  lthm_retrieve_ivf_cursor c = {};
  if (has_cs) {
    c.after_score = after_scores.data_ptr<float>();
    c.after_id = after_ids.data_ptr<int64_t>();
  }
  if (grouped) {
    lthm_retrieve_group g = {};
    g.G = (int32_t)G;
    hip_ok(lthm_retrieve_ivf_topk_group(items.data_ptr(), N, row_ids.data_ptr<int64_t>(), list_off.data_ptr<int64_t>(), L,
                                        q.data_ptr(), dcode(q), normalize_q ? 1 : 0, Q, &g, probes.data_ptr<int32_t>(),
                                        (int32_t)P, (int32_t)k, excl ? &x : nullptr, has_tags ? &t : nullptr,
                                        has_b ? &b : nullptr, has_cs ? &c : nullptr, scores.data_ptr<float>(),
                                        ids.data_ptr<int64_t>(), ws.data_ptr(), need, cur_stream()),
           "lthm_retrieve_ivf_topk_group");
    return std::make_tuple(scores, ids);
  }
  const auto entry = deep ? &lthm_retrieve_ivf_topk_deep : &lthm_retrieve_ivf_topk_filt;
  hip_ok(entry(items.data_ptr(), N, row_ids.data_ptr<int64_t>(), list_off.data_ptr<int64_t>(), L, q.data_ptr(), dcode(q),
               normalize_q ? 1 : 0, Q, probes.data_ptr<int32_t>(), (int32_t)P, (int32_t)k, excl ? &x : nullptr,
               has_tags ? &t : nullptr, has_b ? &b : nullptr, has_cs ? &c : nullptr, scores.data_ptr<float>(),
               ids.data_ptr<int64_t>(), ws.data_ptr(), need, cur_stream()),
         deep ? "lthm_retrieve_ivf_topk_deep" : "lthm_retrieve_ivf_topk_filt");
  return std::make_tuple(scores, ids);
}

std::tuple<Tensor, Tensor> retrieve_ivf_topk_filt_cuda(
    const Tensor& q, const Tensor& items, const Tensor& row_ids, const Tensor& list_off, const Tensor& probes, int64_t k,
    bool normalize_q, const c10::optional<Tensor>& exclude_rows, const c10::optional<Tensor>& tags,
    const c10::optional<Tensor>& tag_filter, const c10::optional<Tensor>& bias, const c10::optional<Tensor>& bias_weight,
    const c10::optional<Tensor>& after_scores, const c10::optional<Tensor>& after_ids) {
  return retrieve_ivf_topk_impl(q, items, row_ids, list_off, probes, k, normalize_q, exclude_rows, tags, tag_filter, bias,
                                bias_weight, after_scores, after_ids, false);
}

// retrieve_ivf_topk_filt with k up to 1,024; k <= 128 runs retrieve_ivf_topk_filt's kernels
std::tuple<Tensor, Tensor> retrieve_ivf_topk_deep_cuda(
    const Tensor& q, const Tensor& items, const Tensor& row_ids, const Tensor& list_off, const Tensor& probes, int64_t k,
    bool normalize_q, const c10::optional<Tensor>& exclude_rows, const c10::optional<Tensor>& tags,
    const c10::optional<Tensor>& tag_filter, const c10::optional<Tensor>& bias, const c10::optional<Tensor>& bias_weight,
    const c10::optional<Tensor>& after_scores, const c10::optional<Tensor>& after_ids) {
  return retrieve_ivf_topk_impl(q, items, row_ids, list_off, probes, k, normalize_q, exclude_rows, tags, tag_filter, bias,
                                bias_weight, after_scores, after_ids, true);
}

// retrieve_ivf_topk_filt for users of G queries each: q [U, G, 128], probes [U, P], every other argument
// per user; an item is scored by its best match over the user's queries and takes one slot
std::tuple<Tensor, Tensor> retrieve_ivf_topk_group_cuda(
    const Tensor& q, const Tensor& items, const Tensor& row_ids, const Tensor& list_off, const Tensor& probes, int64_t k,
    bool normalize_q, const c10::optional<Tensor>& exclude_rows, const c10::optional<Tensor>& tags,
    const c10::optional<Tensor>& tag_filter, const c10::optional<Tensor>& bias, const c10::optional<Tensor>& bias_weight,
    const c10::optional<Tensor>& after_scores, const c10::optional<Tensor>& after_ids) {
  return retrieve_ivf_topk_impl(q, items, row_ids, list_off, probes, k, normalize_q, exclude_rows, tags, tag_filter, bias,
                                bias_weight, after_scores, after_ids, false, true);
}

// items bf16 [N, 128], rows int32 [Q, M], scores f32 [Q, M] (M <= 1024), lam f32 [Q] or None (1
// everywhere), groups int32 [N] or None with cap >= 1; (rows int32 [Q, k], scores f32 [Q, k],
// objective f32 [Q, k]) in selection order, empty slots (-1, -inf, -inf)
std::tuple<Tensor, Tensor, Tensor> retrieve_diversify_cuda(const Tensor& items_, const Tensor& rows_, const Tensor& scores_,
                                                           int64_t k, const c10::optional<Tensor>& lam_,
                                                           const c10::optional<Tensor>& groups_, int64_t cap) {
  on_gpu(items_, "items");
  on_gpu(rows_, "rows");
  on_gpu(scores_, "scores");
  TORCH_CHECK(items_.dim() == 2 && items_.size(1) == 128 && items_.scalar_type() == at::kBFloat16 && items_.size(0) >= 1,
              "items must be a bf16 [N, 128] catalogue, N >= 1");
  TORCH_CHECK(rows_.dim() == 2 && rows_.scalar_type() == at::kInt, "rows must be int32 [Q, M]");
  TORCH_CHECK(scores_.scalar_type() == at::kFloat && scores_.sizes() == rows_.sizes(), "scores must be f32 [Q, M]");
  const int64_t N = items_.size(0), Q = rows_.size(0), M = rows_.size(1);
  TORCH_CHECK(M >= 1 && M <= 1024, "retrieve_diversify takes a pool of 1..1024 candidates (got M=", M, ")");
  TORCH_CHECK(k >= 1 && k <= 128, "retrieve_diversify takes k in 1..128 (got ", k, ")");
  TORCH_CHECK(Q >= 1, "retrieve_diversify takes at least one query");
  TORCH_CHECK(rows_.device() == items_.device() && scores_.device() == items_.device(),
              "rows and scores must be on the catalogue's device");
  const Tensor items = items_.contiguous(), rows = rows_.contiguous(), scores = scores_.contiguous();
  Tensor lam, groups;
  const bool has_l = lam_.has_value() && lam_->defined(), has_g = groups_.has_value() && groups_->defined();
  if (has_l) {
    TORCH_CHECK(lam_->scalar_type() == at::kFloat && lam_->dim() == 1 && lam_->size(0) == Q &&
                    lam_->device() == items.device(),
                "lam must be f32 [Q] on the catalogue's device");
    lam = lam_->contiguous();
  }
  if (has_g) {
    TORCH_CHECK(groups_->scalar_type() == at::kInt && groups_->dim() == 1 && groups_->size(0) == N &&
                    groups_->device() == items.device(),
                "groups must be int32 [N] on the catalogue's device");
    TORCH_CHECK(cap >= 1 && cap <= INT32_MAX, "retrieve_diversify takes cap >= 1 (got ", cap, ")");
    groups = groups_->contiguous();
  }
  const int64_t need = lthm_retrieve_diversify_ws_bytes(Q, M, (int32_t)k);
  TORCH_CHECK(need >= 0, "retrieve_diversify: unsupported sizes Q=", Q, " M=", M, " k=", k);
  Tensor out_rows = at::empty({Q, k}, rows.options()), out_scores = at::empty({Q, k}, scores.options()),
         out_obj = at::empty({Q, k}, scores.options());
  auto ws = at::empty({need}, rows.options().dtype(at::kByte));
  hip_ok(lthm_retrieve_diversify(items.data_ptr(), N, rows.data_ptr<int32_t>(), scores.data_ptr<float>(), Q, (int32_t)M,
                                 (int32_t)k, has_l ? lam.data_ptr<float>() : nullptr,
                                 has_g ? groups.data_ptr<int32_t>() : nullptr, has_g ? (int32_t)cap : 1,
                                 out_rows.data_ptr<int32_t>(), out_scores.data_ptr<float>(), out_obj.data_ptr<float>(),
                                 need ? ws.data_ptr() : nullptr, need, cur_stream()),
         "lthm_retrieve_diversify");
  return {out_rows, out_scores, out_obj};
}

// e4m3 catalogues (lthm_catalogue_quantize_q8, lthm_retrieve_q8_topk, lthm_retrieve_rescore)
// items bf16 [N, 128] -> (codes uint8 [N, 128], scale f32 [N])
std::tuple<Tensor, Tensor> quantize_catalogue_q8_cuda(const Tensor& items_) {
  on_gpu(items_, "items");
  TORCH_CHECK(items_.dim() == 2 && items_.size(1) == 128 && items_.scalar_type() == at::kBFloat16 && items_.size(0) >= 1,
              "items must be a bf16 [N, 128] catalogue, N >= 1");
  const Tensor items = items_.contiguous();
  const int64_t N = items.size(0);
  Tensor codes = at::empty({N, 128}, items.options().dtype(at::kByte)), scale = at::empty({N}, items.options().dtype(at::kFloat));
  hip_ok(lthm_catalogue_quantize_q8(items.data_ptr(), N, codes.data_ptr<uint8_t>(), scale.data_ptr<float>(), cur_stream()),
         "lthm_catalogue_quantize_q8");
  return {codes, scale};
}

// q f32 / bf16 [Q, 128], codes uint8 [N, 128], scale f32 [N], pool in 1..1024, exclude_rows int32
// [Q, X] or None -> (scores f32 [Q, pool], rows int32 [Q, pool]), padded with -inf / -1
std::tuple<Tensor, Tensor> retrieve_q8_topk_cuda(const Tensor& q_, const Tensor& codes_, const Tensor& scale_, int64_t pool,
                                                 bool normalize_q, const c10::optional<Tensor>& excl_) {
  on_gpu(q_, "q");
  on_gpu(codes_, "codes");
  on_gpu(scale_, "scale");
  TORCH_CHECK(codes_.dim() == 2 && codes_.size(1) == 128 && codes_.scalar_type() == at::kByte && codes_.size(0) >= 1,
              "codes must be uint8 [N, 128], N >= 1");
  const int64_t N = codes_.size(0);
  TORCH_CHECK(scale_.scalar_type() == at::kFloat && scale_.dim() == 1 && scale_.size(0) == N, "scale must be f32 [N]");
  TORCH_CHECK(q_.dim() == 2 && q_.size(1) == 128 && q_.size(0) >= 1, "q must be [Q, 128], Q >= 1");
  TORCH_CHECK(pool >= 1 && pool <= 1024, "retrieve_q8_topk takes a pool of 1..1024 rows (got ", pool, ")");
  TORCH_CHECK(codes_.device() == q_.device() && scale_.device() == q_.device(),
              "codes and scales must be on the queries' device");
  const Tensor q = q_.contiguous(), codes = codes_.contiguous(), scale = scale_.contiguous();
  const int64_t Q = q.size(0);
  const bool has_x = excl_.has_value() && excl_->defined();
  Tensor xr;
  if (has_x) {
    on_gpu(*excl_, "exclude_rows");
    TORCH_CHECK(excl_->scalar_type() == at::kInt && excl_->dim() == 2 && excl_->size(0) == Q,
                "exclude_rows must be int32 [Q, X]");
    TORCH_CHECK(excl_->size(1) >= 1 && excl_->size(1) <= 1024, "exclude_rows takes 1..1024 rows per query, got ",
                excl_->size(1));
    TORCH_CHECK(excl_->device() == q.device(), "exclude_rows must be on the queries' device");
    xr = excl_->contiguous();
  }
  const int64_t need = lthm_retrieve_q8_ws_bytes(Q, N, (int32_t)pool, 0, has_x ? xr.size(1) : 0);
  TORCH_CHECK(need >= 0, "retrieve_q8_topk: unsupported sizes Q=", Q, " N=", N);
  auto scores = at::empty({Q, pool}, q.options().dtype(at::kFloat));
  auto rows = at::empty({Q, pool}, q.options().dtype(at::kInt));
  auto ws = at::empty({need}, q.options().dtype(at::kByte));
  lthm_retrieve_excl x = {};
  if (has_x) {
    x.rows = xr.data_ptr<int32_t>();
    x.X = xr.size(1);
  }
  hip_ok(lthm_retrieve_q8_topk(codes.data_ptr<uint8_t>(), scale.data_ptr<float>(), N, q.data_ptr(), dcode(q),
                               normalize_q ? 1 : 0, Q, (int32_t)pool, 0, has_x ? &x : nullptr, scores.data_ptr<float>(),
                               rows.data_ptr<int32_t>(), ws.data_ptr(), need, cur_stream()),
         "lthm_retrieve_q8_topk");
  return {scores, rows};
}

// q f32 / bf16 [Q, 128], items bf16 [N, 128], rows int32 [Q, M] (M <= 1024), k in 1..M ->
// (scores f32 [Q, k], rows int32 [Q, k]): the flat call's bits for the listed rows, sorted
std::tuple<Tensor, Tensor> retrieve_rescore_cuda(const Tensor& q_, const Tensor& items_, const Tensor& rows_, int64_t k,
                                                 bool normalize_q) {
  on_gpu(q_, "q");
  on_gpu(items_, "items");
  on_gpu(rows_, "rows");
  TORCH_CHECK(items_.dim() == 2 && items_.size(1) == 128 && items_.scalar_type() == at::kBFloat16 && items_.size(0) >= 1,
              "items must be a bf16 [N, 128] catalogue, N >= 1");
  TORCH_CHECK(q_.dim() == 2 && q_.size(1) == 128 && q_.size(0) >= 1, "q must be [Q, 128], Q >= 1");
  const int64_t Q = q_.size(0), N = items_.size(0);
  TORCH_CHECK(rows_.dim() == 2 && rows_.scalar_type() == at::kInt && rows_.size(0) == Q, "rows must be int32 [Q, M]");
  const int64_t M = rows_.size(1);
  TORCH_CHECK(M >= 1 && M <= 1024, "retrieve_rescore takes lists of 1..1024 rows (got M=", M, ")");
  TORCH_CHECK(k >= 1 && k <= M, "retrieve_rescore takes k in 1..M (got k=", k, ", M=", M, ")");
  TORCH_CHECK(rows_.device() == q_.device() && items_.device() == q_.device(),
              "rows and the catalogue must be on the queries' device");
  const Tensor q = q_.contiguous(), items = items_.contiguous(), rows = rows_.contiguous();
  const int64_t need = lthm_retrieve_rescore_ws_bytes(Q, (int32_t)M, (int32_t)k);
  TORCH_CHECK(need >= 0, "retrieve_rescore: unsupported sizes Q=", Q, " M=", M, " k=", k);
  auto scores = at::empty({Q, k}, q.options().dtype(at::kFloat));
  auto out_rows = at::empty({Q, k}, rows.options());
  auto ws = at::empty({need}, rows.options().dtype(at::kByte));
  hip_ok(lthm_retrieve_rescore(items.data_ptr(), N, q.data_ptr(), dcode(q), normalize_q ? 1 : 0, Q, rows.data_ptr<int32_t>(),
                               (int32_t)M, (int32_t)k, scores.data_ptr<float>(), out_rows.data_ptr<int32_t>(), ws.data_ptr(),
                               need, cur_stream()),
         "lthm_retrieve_rescore");
  return {scores, out_rows};
}

// retrieve_rescore with a prior (bias f32 [N], bias_weight f32 [Q] or None: 1) and an id order
// (order_ids int64 [N] or None): fma(w, bias[row], dot) under (score descending, order_ids[row] ascending)
std::tuple<Tensor, Tensor> retrieve_rescore_bias_cuda(const Tensor& q_, const Tensor& items_, const Tensor& rows_, int64_t k,
                                                      bool normalize_q, const c10::optional<Tensor>& bias_,
                                                      const c10::optional<Tensor>& bias_weight_,
                                                      const c10::optional<Tensor>& order_ids_) {
  on_gpu(q_, "q");
  on_gpu(items_, "items");
  on_gpu(rows_, "rows");
  TORCH_CHECK(items_.dim() == 2 && items_.size(1) == 128 && items_.scalar_type() == at::kBFloat16 && items_.size(0) >= 1,
              "items must be a bf16 [N, 128] catalogue, N >= 1");
  TORCH_CHECK(q_.dim() == 2 && q_.size(1) == 128 && q_.size(0) >= 1, "q must be [Q, 128], Q >= 1");
  const int64_t Q = q_.size(0), N = items_.size(0);
  TORCH_CHECK(rows_.dim() == 2 && rows_.scalar_type() == at::kInt && rows_.size(0) == Q, "rows must be int32 [Q, M]");
  const int64_t M = rows_.size(1);
  TORCH_CHECK(M >= 1 && M <= 1024, "retrieve_rescore_bias takes lists of 1..1024 rows (got M=", M, ")");
  TORCH_CHECK(k >= 1 && k <= M, "retrieve_rescore_bias takes k in 1..M (got k=", k, ", M=", M, ")");
  TORCH_CHECK(rows_.device() == q_.device() && items_.device() == q_.device(),
              "rows and the catalogue must be on the queries' device");
  const bool has_b = bias_.has_value() && bias_->defined(), has_w = bias_weight_.has_value() && bias_weight_->defined();
  const bool has_o = order_ids_.has_value() && order_ids_->defined();
  TORCH_CHECK(has_b || !has_w, "retrieve_rescore_bias takes a bias_weight only with a bias");
  Tensor bias, bias_weight, order_ids;
  if (has_b) {
    on_gpu(*bias_, "bias");
    TORCH_CHECK(bias_->scalar_type() == at::kFloat && bias_->dim() == 1 && bias_->size(0) == N &&
                    bias_->device() == items_.device(),
                "bias must be f32 [N] on the catalogue's device");
    bias = bias_->contiguous();
  }
  if (has_w) {
    on_gpu(*bias_weight_, "bias_weight");
    TORCH_CHECK(bias_weight_->scalar_type() == at::kFloat && bias_weight_->dim() == 1 && bias_weight_->size(0) == Q &&
                    bias_weight_->device() == q_.device(),
                "bias_weight must be f32 [Q] on the queries' device");
    bias_weight = bias_weight_->contiguous();
  }
  if (has_o) {
    on_gpu(*order_ids_, "order_ids");
    TORCH_CHECK(order_ids_->scalar_type() == at::kLong && order_ids_->dim() == 1 && order_ids_->size(0) == N &&
                    order_ids_->device() == items_.device(),
                "order_ids must be int64 [N] on the catalogue's device");
    order_ids = order_ids_->contiguous();
  }
  const Tensor q = q_.contiguous(), items = items_.contiguous(), rows = rows_.contiguous();
  const int64_t need = lthm_retrieve_rescore_ws_bytes(Q, (int32_t)M, (int32_t)k);
  TORCH_CHECK(need >= 0, "retrieve_rescore_bias: unsupported sizes Q=", Q, " M=", M, " k=", k);
  auto scores = at::empty({Q, k}, q.options().dtype(at::kFloat));
  auto out_rows = at::empty({Q, k}, rows.options());
  auto ws = at::empty({need}, rows.options().dtype(at::kByte));
  hip_ok(lthm_retrieve_rescore_bias(items.data_ptr(), N, q.data_ptr(), dcode(q), normalize_q ? 1 : 0, Q,
                                    rows.data_ptr<int32_t>(), (int32_t)M, (int32_t)k,
                                    has_b ? bias.data_ptr<float>() : nullptr, has_w ? bias_weight.data_ptr<float>() : nullptr,
                                    has_o ? order_ids.data_ptr<int64_t>() : nullptr, scores.data_ptr<float>(),
                                    out_rows.data_ptr<int32_t>(), ws.data_ptr(), need, cur_stream()),
         "lthm_retrieve_rescore_bias");
  return {scores, out_rows};
}

// The shortlist of a clustered e4m3 catalogue (lthm_retrieve_ivf_q8_topk): q f32 / bf16 [Q, 128], codes
// uint8 [N, 128] and scale f32 [N] list-major, row_ids int64 [N], list_off int64 [L + 1], probes int32
// [Q, P], pool in 1..1024, exclude_rows / tags / tag_filter / bias / bias_weight as retrieve_ivf_topk_deep
// takes them -> (scores f32 [Q, pool], rows int32 [Q, pool]) under (score descending, id ascending),
// padded with -inf / -1
std::tuple<Tensor, Tensor> retrieve_ivf_q8_topk_cuda(
    const Tensor& q_, const Tensor& codes_, const Tensor& scale_, const Tensor& row_ids_, const Tensor& list_off_,
    const Tensor& probes_, int64_t pool, bool normalize_q, const c10::optional<Tensor>& exclude_rows,
    const c10::optional<Tensor>& tags_, const c10::optional<Tensor>& tag_filter_, const c10::optional<Tensor>& bias_,
    const c10::optional<Tensor>& bias_weight_) {
  on_gpu(q_, "q");
  on_gpu(codes_, "codes");
  on_gpu(scale_, "scale");
  on_gpu(row_ids_, "row_ids");
  on_gpu(list_off_, "list_off");
  on_gpu(probes_, "probes");
  TORCH_CHECK(codes_.dim() == 2 && codes_.size(1) == 128 && codes_.scalar_type() == at::kByte && codes_.size(0) >= 1,
              "codes must be uint8 [N, 128], N >= 1");
  const int64_t N = codes_.size(0);
  TORCH_CHECK(scale_.scalar_type() == at::kFloat && scale_.dim() == 1 && scale_.size(0) == N, "scale must be f32 [N]");
  TORCH_CHECK(q_.dim() == 2 && q_.size(1) == 128 && q_.size(0) >= 1, "q must be [Q, 128], Q >= 1");
  TORCH_CHECK(pool >= 1 && pool <= 1024, "retrieve_ivf_q8_topk takes a pool of 1..1024 rows (got ", pool, ")");
  const int64_t Q = q_.size(0);
  TORCH_CHECK(row_ids_.scalar_type() == at::kLong && row_ids_.dim() == 1 && row_ids_.size(0) == N,
              "row_ids must be int64 [N], one id per catalogue row");
  TORCH_CHECK(list_off_.scalar_type() == at::kLong && list_off_.dim() == 1 && list_off_.size(0) >= 2,
              "list_off must be int64 [L + 1], L >= 1");
  TORCH_CHECK(probes_.scalar_type() == at::kInt && probes_.dim() == 2 && probes_.size(0) == Q, "probes must be int32 [Q, P]");
  TORCH_CHECK(probes_.size(1) >= 1 && probes_.size(1) <= 64, "retrieve_ivf_q8_topk takes 1..64 probes per query, got P=",
              probes_.size(1));
  TORCH_CHECK(scale_.device() == codes_.device() && row_ids_.device() == codes_.device() &&
                  list_off_.device() == codes_.device() && probes_.device() == codes_.device() &&
                  q_.device() == codes_.device(),
              "q, scale, row_ids, list_off and probes must be on the catalogue's device");
  const Tensor q = q_.contiguous(), codes = codes_.contiguous(), scale = scale_.contiguous();
  const Tensor row_ids = row_ids_.contiguous(), list_off = list_off_.contiguous(), probes = probes_.contiguous();
  const int64_t L = list_off.size(0) - 1, P = probes.size(1);
  Tensor xr;
  const bool excl = exclude_rows.has_value() && exclude_rows->defined();
  if (excl) {
    on_gpu(*exclude_rows, "exclude_rows");
    TORCH_CHECK(exclude_rows->scalar_type() == at::kInt && exclude_rows->dim() == 2 && exclude_rows->size(0) == Q,
                "exclude_rows must be int32 [Q, X]");
    TORCH_CHECK(exclude_rows->size(1) >= 1 && exclude_rows->size(1) <= 1024,
                "exclude_rows takes 1..1024 rows per query, got ", exclude_rows->size(1));
    TORCH_CHECK(exclude_rows->device() == q.device(), "exclude_rows must be on the queries' device");
    xr = exclude_rows->contiguous();
  }
  const bool has_tags = tags_.has_value() && tags_->defined(), has_filter = tag_filter_.has_value() && tag_filter_->defined();
  TORCH_CHECK(has_tags == has_filter, "retrieve_ivf_q8_topk takes tags and tag_filter together or neither");
  const bool has_b = bias_.has_value() && bias_->defined(), has_w = bias_weight_.has_value() && bias_weight_->defined();
  TORCH_CHECK(has_b || !has_w, "retrieve_ivf_q8_topk takes a bias_weight only with a bias");
  Tensor tags, tag_filter, bias, bias_weight;
  if (has_tags) {
    on_gpu(*tags_, "tags");
    on_gpu(*tag_filter_, "tag_filter");
    TORCH_CHECK(tags_->scalar_type() == at::kInt && tags_->dim() == 1 && tags_->size(0) == N &&
                    tags_->device() == codes.device(),
                "tags must be int32 [N] on the catalogue's device");
    TORCH_CHECK(tag_filter_->scalar_type() == at::kInt && tag_filter_->dim() == 2 && tag_filter_->size(0) == Q &&
                    tag_filter_->size(1) == 3 && tag_filter_->device() == q.device(),
                "tag_filter must be int32 [Q, 3] on the queries' device");
    tags = tags_->contiguous();
    tag_filter = tag_filter_->contiguous();
  }
  if (has_b) {
    on_gpu(*bias_, "bias");
    TORCH_CHECK(bias_->scalar_type() == at::kFloat && bias_->dim() == 1 && bias_->size(0) == N &&
                    bias_->device() == codes.device(),
                "bias must be f32 [N] on the catalogue's device");
    bias = bias_->contiguous();
    if (has_w) {
      on_gpu(*bias_weight_, "bias_weight");
      TORCH_CHECK(bias_weight_->scalar_type() == at::kFloat && bias_weight_->dim() == 1 && bias_weight_->size(0) == Q &&
                      bias_weight_->device() == q.device(),
                  "bias_weight must be f32 [Q] on the queries' device");
      bias_weight = bias_weight_->contiguous();
    }
  }
  const int64_t need = lthm_retrieve_ivf_q8_ws_bytes(Q, N, L, (int32_t)P, (int32_t)pool, excl ? xr.size(1) : 0);
  TORCH_CHECK(need >= 0, "retrieve_ivf_q8_topk: unsupported sizes Q=", Q, " N=", N, " L=", L, " P=", P);
  auto scores = at::empty({Q, pool}, q.options().dtype(at::kFloat));
  auto rows = at::empty({Q, pool}, q.options().dtype(at::kInt));
  auto ws = at::empty({need}, q.options().dtype(at::kByte));
  lthm_retrieve_excl x = {};
  if (excl) {
    x.rows = xr.data_ptr<int32_t>();
    x.X = xr.size(1);
  }
  lthm_retrieve_tags t = {};
  if (has_tags) {
    t.tags = tags.data_ptr<int32_t>();
    t.filter = tag_filter.data_ptr<int32_t>();
  }
  lthm_retrieve_bias b = {};
  if (has_b) {
    b.bias = bias.data_ptr<float>();
    b.weight = has_w ? bias_weight.data_ptr<float>() : nullptr;
  }
  hip_ok(lthm_retrieve_ivf_q8_topk(codes.data_ptr<uint8_t>(), scale.data_ptr<float>(), N, row_ids.data_ptr<int64_t>(),
                                   list_off.data_ptr<int64_t>(), L, q.data_ptr(), dcode(q), normalize_q ? 1 : 0, Q,
                                   probes.data_ptr<int32_t>(), (int32_t)P, (int32_t)pool, excl ? &x : nullptr,
                                   has_tags ? &t : nullptr, has_b ? &b : nullptr, scores.data_ptr<float>(),
                                   rows.data_ptr<int32_t>(), ws.data_ptr(), need, cur_stream()),
         "lthm_retrieve_ivf_q8_topk");
  return {scores, rows};
}

int64_t abi_version() { return lthm_abi_version(); }
// the include/lthm.h this op library was compiled against (descriptor layouts)
int64_t built_abi_version() { return LTHM_ABI_VERSION; }

}  // namespace

TORCH_LIBRARY(lthm, m) {
  m.def("abi_version() -> int", &abi_version);
  m.def("built_abi_version() -> int", &built_abi_version);
  m.def("kshift(Tensor ids, Tensor weight, int P, int K, int mode, int F=1, ScalarType? out_dtype=None) -> Tensor");
  m.def("kshift_rows(Tensor ids, int P, int K) -> Tensor");
  m.def("gather_pool(Tensor rows, Tensor weight, int mode, ScalarType out_dtype=float) -> Tensor");
  m.def("activation(Tensor x, int act) -> Tensor");
  m.def("mlp_chain(Tensor x, Tensor[] weights, Tensor[] biases, int[] acts, bool out_f32=True) -> Tensor");
  m.def(
      "item_artifact(Tensor ids, Tensor weight, int K, int mode, Tensor mask_weight, int mask_K, Tensor w1, "
      "Tensor b1, Tensor w2, Tensor b2, ScalarType out_dtype=float) -> Tensor");
  m.def("retrieve_topk(Tensor q, Tensor items, int k, bool normalize_q) -> (Tensor scores, Tensor rows)");
  m.def(
      "retrieve_topk_excl(Tensor q, Tensor items, int k, bool normalize_q, Tensor exclude_rows) -> "
      "(Tensor scores, Tensor rows)");
  m.def(
      "retrieve_topk_group(Tensor q, Tensor items, int k, bool normalize_q, Tensor? exclude_rows=None) -> "
      "(Tensor scores, Tensor rows)");
  m.def(
      "retrieve_topk_tags(Tensor q, Tensor items, int k, bool normalize_q, Tensor? exclude_rows, Tensor tags, "
      "Tensor tag_filter) -> (Tensor scores, Tensor rows)");
  m.def(
      "retrieve_topk_after(Tensor q, Tensor items, int k, bool normalize_q, Tensor? exclude_rows, Tensor? tags, "
      "Tensor? tag_filter, Tensor after_scores, Tensor after_rows) -> (Tensor scores, Tensor rows)");
  m.def(
      "retrieve_topk_bias(Tensor q, Tensor items, int k, bool normalize_q, Tensor? exclude_rows, Tensor? tags, "
      "Tensor? tag_filter, Tensor? after_scores, Tensor? after_rows, Tensor bias, Tensor? bias_weight=None) -> "
      "(Tensor scores, Tensor rows)");
  m.def(
      "retrieve_topk_deep(Tensor q, Tensor items, int k, bool normalize_q, Tensor? exclude_rows, Tensor? tags, "
      "Tensor? tag_filter, Tensor? after_scores, Tensor? after_rows, Tensor? bias, Tensor? bias_weight=None) -> "
      "(Tensor scores, Tensor rows)");
  m.def("retrieve_merge_shards(Tensor scores, Tensor ids, Tensor? ranks=None) -> (Tensor scores, Tensor ids, Tensor rank)");
  m.def(
      "retrieve_ivf_topk_shards(Tensor q, Tensor[] items, Tensor[] row_ids, Tensor[] list_off, Tensor[] centroids, "
      "Tensor[] tags, Tensor[] bias, int nprobe, int k, bool normalize_q=True, Tensor? exclude_rows=None, "
      "Tensor? tag_filter=None, bool use_bias=False, Tensor? bias_weight=None, Tensor? after_scores=None, "
      "Tensor? after_ids=None, Tensor? target_rows=None, Tensor? target_scores=None) -> (Tensor scores, Tensor ids, Tensor rank)");
  m.def(
      "retrieve_ivf_topk(Tensor q, Tensor items, Tensor row_ids, Tensor list_off, Tensor probes, int k, "
      "bool normalize_q, Tensor? exclude_rows=None) -> (Tensor scores, Tensor ids)");
  m.def(
      "retrieve_ivf_topk_filt(Tensor q, Tensor items, Tensor row_ids, Tensor list_off, Tensor probes, int k, "
      "bool normalize_q, Tensor? exclude_rows=None, Tensor? tags=None, Tensor? tag_filter=None, Tensor? bias=None, "
      "Tensor? bias_weight=None, Tensor? after_scores=None, Tensor? after_ids=None) -> (Tensor scores, Tensor ids)");
  m.def(
      "retrieve_ivf_topk_deep(Tensor q, Tensor items, Tensor row_ids, Tensor list_off, Tensor probes, int k, "
      "bool normalize_q, Tensor? exclude_rows=None, Tensor? tags=None, Tensor? tag_filter=None, Tensor? bias=None, "
      "Tensor? bias_weight=None, Tensor? after_scores=None, Tensor? after_ids=None) -> (Tensor scores, Tensor ids)");
  m.def(
      "retrieve_ivf_topk_group(Tensor q, Tensor items, Tensor row_ids, Tensor list_off, Tensor probes, int k, "
      "bool normalize_q, Tensor? exclude_rows=None, Tensor? tags=None, Tensor? tag_filter=None, Tensor? bias=None, "
      "Tensor? bias_weight=None, Tensor? after_scores=None, Tensor? after_ids=None) -> (Tensor scores, Tensor ids)");
  m.def(
      "retrieve_diversify(Tensor items, Tensor rows, Tensor scores, int k, Tensor? lam=None, Tensor? groups=None, "
      "int cap=1) -> (Tensor rows, Tensor scores, Tensor objective)");
  m.def("quantize_catalogue_q8(Tensor items) -> (Tensor codes, Tensor scale)");
  m.def(
      "retrieve_q8_topk(Tensor q, Tensor codes, Tensor scale, int pool, bool normalize_q, Tensor? exclude_rows=None) -> "
      "(Tensor scores, Tensor rows)");
  m.def("retrieve_rescore(Tensor q, Tensor items, Tensor rows, int k, bool normalize_q) -> (Tensor scores, Tensor rows)");
  m.def(
      "retrieve_rescore_bias(Tensor q, Tensor items, Tensor rows, int k, bool normalize_q, Tensor? bias=None, "
      "Tensor? bias_weight=None, Tensor? order_ids=None) -> (Tensor scores, Tensor rows)");
  m.def(
      "retrieve_ivf_q8_topk(Tensor q, Tensor codes, Tensor scale, Tensor row_ids, Tensor list_off, Tensor probes, "
      "int pool, bool normalize_q, Tensor? exclude_rows=None, Tensor? tags=None, Tensor? tag_filter=None, "
      "Tensor? bias=None, Tensor? bias_weight=None) -> (Tensor scores, Tensor rows)");
}

TORCH_LIBRARY_IMPL(lthm, CUDA, m) {
  m.impl("kshift", &kshift_cuda);
  m.impl("kshift_rows", &kshift_rows_cuda);
  m.impl("gather_pool", &gather_pool_cuda);
  m.impl("mlp_chain", &mlp_chain_cuda);
  m.impl("activation", &activation_cuda);
  m.impl("item_artifact", &item_artifact_cuda);
  m.impl("retrieve_topk", &retrieve_topk_cuda);
  m.impl("retrieve_topk_excl", &retrieve_topk_excl_cuda);
  m.impl("retrieve_topk_group", &retrieve_topk_group_cuda);
  m.impl("retrieve_topk_tags", &retrieve_topk_tags_cuda);
  m.impl("retrieve_topk_after", &retrieve_topk_after_cuda);
  m.impl("retrieve_topk_bias", &retrieve_topk_bias_cuda);
  m.impl("retrieve_topk_deep", &retrieve_topk_deep_cuda);
  m.impl("retrieve_merge_shards", &retrieve_merge_shards_cuda);
  m.impl("retrieve_ivf_topk_shards", &retrieve_ivf_topk_shards_cuda);
  m.impl("retrieve_ivf_topk", &retrieve_ivf_topk_cuda);
  m.impl("retrieve_ivf_topk_filt", &retrieve_ivf_topk_filt_cuda);
  m.impl("retrieve_ivf_topk_deep", &retrieve_ivf_topk_deep_cuda);
  m.impl("retrieve_ivf_topk_group", &retrieve_ivf_topk_group_cuda);
  m.impl("retrieve_diversify", &retrieve_diversify_cuda);
  m.impl("quantize_catalogue_q8", &quantize_catalogue_q8_cuda);
  m.impl("retrieve_q8_topk", &retrieve_q8_topk_cuda);
  m.impl("retrieve_rescore", &retrieve_rescore_cuda);
  m.impl("retrieve_rescore_bias", &retrieve_rescore_bias_cuda);
  m.impl("retrieve_ivf_q8_topk", &retrieve_ivf_q8_topk_cuda);
}

TORCH_LIBRARY_IMPL(lthm, Autograd, m) {
  m.impl("kshift", &kshift_autograd);
  m.impl("mlp_chain", &mlp_chain_autograd);
  m.impl("activation", &activation_autograd);
}
