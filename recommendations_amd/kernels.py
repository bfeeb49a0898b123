"""torch.autograd.Function wrappers over the C ABI (include/lthm.h).

These are the only places the product path computes anything: each op checks
that its tensors are on the GPU (no CPU fallback), allocates outputs through
torch, and launches the gfx950 kernel on torch's current stream.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional

import collections
import os

import torch

from ._lib import BF16, F32, call, dcode, load, ptr, require_gpu, stream

KSHIFT_SCALE, KSHIFT_NORMALIZE, KSHIFT_NONE = 0, 1, 2


# ----------------------------------------------------------------- KShift
def kshift_rows(ids: torch.Tensor, P: int, K: int) -> torch.Tensor:
    """All K row indices of every id: [.., K] int64 (commons/layers.py:174-185)."""
    require_gpu(ids)
    _check_kshift(ids, P, K, 1, 1)
    rows = torch.empty(ids.shape + (K,), dtype=torch.int64, device=ids.device)
    call("lthm_kshift_rows", ptr(ids), ids.numel(), P, K, ptr(rows), stream())
    return rows


class OperandError(RuntimeError, ValueError):
    """Bad op argument, caught on the host before any launch.  A RuntimeError like
    the reference's own argument errors (transformers/layers.py:26-29)."""


def _check(cond, msg):
    """Host-side operand check before a launch: the kernels trust their sizes."""
    if not cond:
        raise OperandError(msg)


def _need(t, n: int, name: str):
    """t must back at least n elements from its data pointer (views included)."""
    if t is None:
        return
    avail = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
    _check(avail >= n, f"{name}: needs {n} elements from its data pointer, has {avail}")


def _check_kshift(ids, P, K, F, D, table_rows=None, gy=None, out=None, norms=None):
    _check(ids.dtype == torch.int64, f"ids must be int64, got {ids.dtype}")
    _check(P > 0 and 0 < K <= 64 and F >= 1, f"bad KShift config P={P} K={K} F={F}")
    _check(ids.numel() % F == 0, f"ids.numel()={ids.numel()} is not a multiple of F={F}")
    if table_rows is not None:
        _check(table_rows == F * P, f"table has {table_rows} rows, expected F*P = {F * P}")
    if gy is not None:
        _check(gy.numel() == ids.numel() * D, f"grad has {gy.numel()} elements, expected {ids.numel() * D}")
    if out is not None:
        _check(out.numel() == ids.numel() * D, f"out has {out.numel()} elements, expected {ids.numel() * D}")
    if norms is not None:
        _check(norms.numel() == ids.numel(), "norms must hold one value per id")


class KShiftFn(torch.autograd.Function):
    """Gather + in-order pool of K table rows (commons/layers.py:152-172).

    ``F`` > 1 selects the table-batched layout: ids [..., F], weight [F*P, D],
    feature f reading rows [f*P, (f+1)*P).
    """

    @staticmethod
    def forward(ctx, ids, weight, P: int, K: int, mode: int, F: int, out_dtype):
        require_gpu(ids, weight)
        D = weight.shape[1]
        _check_kshift(ids, P, K, F, D, table_rows=weight.shape[0])
        n = ids.numel() // F
        out = torch.empty(ids.shape + (D,), dtype=out_dtype, device=ids.device)
        need_norms = mode == KSHIFT_NORMALIZE and weight.requires_grad
        norms = torch.empty(ids.shape, dtype=torch.float32, device=ids.device) if need_norms else None
        call("lthm_kshift_fwd_multi", ptr(ids), n, F, ptr(weight), dcode(weight), P, D, K, mode,
             ptr(out), dcode(out), ptr(norms), stream(), _key="kshift_fwd_k",
             _work=ids.numel() * (8 + K * D * weight.element_size() + D * out.element_size()), _unit="byte")
        ctx.save_for_backward(ids, out if mode == KSHIFT_NORMALIZE else None, norms)
        ctx.cfg = (P, K, mode, F, D, weight.shape, weight.dtype)
        return out

    @staticmethod
    def backward(ctx, gy):
        ids, out, norms = ctx.saved_tensors
        P, K, mode, F, D, wshape, wdtype = ctx.cfg
        gy = gy.contiguous()
        _check_kshift(ids, P, K, F, D, table_rows=wshape[0], gy=gy, out=out, norms=norms)
        dW = torch.zeros(wshape, dtype=torch.float32, device=gy.device)
        n = ids.numel() // F
        call("lthm_kshift_bwd_dense", ptr(ids), n, F, ptr(gy), dcode(gy),
             ptr(out) if out is not None else None, dcode(out) if out is not None else F32,
             ptr(norms), P, D, K, mode, ptr(dW), stream())
        if wdtype != torch.float32:
            dW = dW.to(wdtype)
        return None, dW, None, None, None, None, None


def kshift(ids, weight, P: int, K: int, mode: int, F: int = 1, out_dtype=None):
    if out_dtype is None:
        out_dtype = weight.dtype
    return KShiftFn.apply(ids.contiguous(), weight, P, K, mode, F, out_dtype)


def gather_pool(rows: torch.Tensor, W: torch.Tensor, mode: int, out_dtype=torch.float32):
    """out[i] = finalize(sum_c W[rows[i, c]]) (include/lthm.h lthm_gather_pool): rows [n, K] int64 < W.shape[0]."""
    require_gpu(rows, W)
    _check(rows.dtype == torch.int64 and rows.dim() == 2, "rows must be int64 [n, K]")
    n, Kk = rows.shape
    _check(0 < Kk <= 64, "K must be in 1..64")
    D = W.shape[1]
    out = torch.empty((n, D), dtype=out_dtype, device=W.device)
    call("lthm_gather_pool", ptr(rows), n, Kk, ptr(W), dcode(W), W.shape[0], D, mode, ptr(out), dcode(out), None,
         stream(), _key="kshift_fwd_k", _work=n * (8 * Kk + Kk * D * W.element_size() + D * out.element_size()),
         _unit="byte")
    return out


def shard_route(ids: torch.Tensor, P: int, K: int, world: int):
    """Row-sharded KShift lookup routing (lthm_shard_route; C3 item table): the K rows of every
    id deduplicated per 2,048 (row, shift) pairs, owner-major (row r on rank r % world).
    Returns send_rows [n K] (the first owner_base[world] used), send_counts [world] and
    owner_base [world + 1] (device int64) and inv [n, K]: each pair's position in the
    owner-major value buffer the exchange returns."""
    require_gpu(ids)
    flat = ids.reshape(-1).contiguous()
    n = flat.numel()
    # world <= 256: the dedup kernel counts requests per owner in a 256-entry LDS array (csrc/shard.hip)
    _check(flat.dtype == torch.int64 and 0 < K <= 64 and P > 0 and 0 < world <= 256,
           "shard_route: int64 ids, 0 < K <= 64, 0 < world <= 256")
    dev = ids.device
    npairs = n * K
    send = torch.empty(max(npairs, 1), dtype=torch.int64, device=dev)
    cnt = torch.empty(world, dtype=torch.int64, device=dev)
    base = torch.empty(world + 1, dtype=torch.int64, device=dev)
    inv = torch.empty(max(npairs, 1), dtype=torch.int64, device=dev)
    wsb = int(load().lthm_shard_route_ws_bytes(npairs, world))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)  # stream-ordered by the allocator (side streams)
    call("lthm_shard_route", ptr(flat), n, K, P, world, ptr(send), ptr(cnt), ptr(base), ptr(inv), ptr(ws), wsb,
         stream(), _key="shard_route", _work=float(npairs) * (8 + 16 + 8 + 8), _unit="byte")
    return send, cnt, base, inv[:npairs].view(n, K)


def shard_gather(shard: torch.Tensor, rows: torch.Tensor, world: int, count: torch.Tensor = None):
    """out[i] = shard[rows[i] // world] (lthm_shard_gather), for i < count[0] when ``count`` (a device
    int64 scalar view) is given, else for every row."""
    require_gpu(shard, rows, count)
    _check(shard.dim() == 2 and (shard.shape[1] * shard.element_size()) % 16 == 0,
           "shard_gather: [n, D] shard with 16-byte-multiple rows")
    cap = rows.numel()
    out = torch.empty((cap, shard.shape[1]), dtype=shard.dtype, device=shard.device)
    rb = shard.shape[1] * shard.element_size()
    call("lthm_shard_gather", ptr(shard), shard.shape[0], rb, ptr(rows), ptr(count), cap, world, ptr(out), stream(),
         _key="shard_gather", _work=float(cap) * (8 + 2 * rb), _unit="byte")
    return out


# ----------------------------------------------------------------- helpers
def cast(x: torch.Tensor, dtype) -> torch.Tensor:
    """dtype cast in a HIP kernel (f32 <-> bf16)."""
    require_gpu(x)
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    call("lthm_cast", ptr(x), dcode(x), ptr(out), dcode(out), x.numel(), stream())
    return out


# bf16 GEMM operands of fp32 weights.  They are cast from the live fp32 parameter
# at every forward, never kept across steps: a copy that outlives its forward can go
# stale behind writes torch does not version (p.data.copy_, a collective writing
# into p, module.to()).  A model casts all its encoder weights in ONE launch at
# the start of its forward (``bf16_operands`` scope, lthm_cast_multi_bf16); inside
# the scope ``bf16_operand`` returns those copies, outside it casts on the spot.
_CAST_SCOPES: list = []


def cast_multi_bf16(ts):
    """[bf16(t) for t in ts] for contiguous fp32 CUDA tensors, one launch per 48 tensors."""
    import ctypes
    ts = [t.detach() for t in ts]
    for t in ts:
        require_gpu(t)
        _check(t.dtype == torch.float32, "cast_multi_bf16 takes fp32 tensors")
    outs = [torch.empty(t.shape, dtype=torch.bfloat16, device=t.device) for t in ts]
    n = len(ts)
    if n == 0:
        return outs
    arr = lambda xs: ctypes.cast((ctypes.c_void_p * n)(*[x.data_ptr() for x in xs]), ctypes.c_void_p)  # noqa: E731
    cnt = (ctypes.c_int64 * n)(*[t.numel() for t in ts])
    call("lthm_cast_multi_bf16", n, arr(ts), arr(outs), ctypes.cast(cnt, ctypes.c_void_p), stream(),
         _key="cast_multi_k", _work=6.0 * sum(t.numel() for t in ts), _unit="byte")
    return outs


def cast_multi_bf16_into(ts, outs):
    """outs[i][:] = bf16(ts[i]) for contiguous fp32 sources and bf16 destinations of the same
    element counts (e.g. row slices of one image), one launch per 48 tensors."""
    import ctypes
    ts = [t.detach() for t in ts]
    n = len(ts)
    _check(n == len(outs), "cast_multi_bf16_into: one destination per source")
    for t, o in zip(ts, outs):
        require_gpu(t, o)
        _check(t.dtype == torch.float32 and o.dtype == torch.bfloat16 and t.numel() == o.numel()
               and t.is_contiguous() and o.is_contiguous(), "cast_multi_bf16_into: fp32 -> bf16, equal sizes")
    if n == 0:
        return outs
    arr = lambda xs: ctypes.cast((ctypes.c_void_p * n)(*[x.data_ptr() for x in xs]), ctypes.c_void_p)  # noqa: E731
    cnt = (ctypes.c_int64 * n)(*[t.numel() for t in ts])
    call("lthm_cast_multi_bf16", n, arr(ts), arr(outs), ctypes.cast(cnt, ctypes.c_void_p), stream(),
         _key="cast_multi_k", _work=6.0 * sum(t.numel() for t in ts), _unit="byte")
    return outs


class bf16_operands:
    """Context: the bf16 copies of ``params`` (fp32), cast in one launch on entry and
    served by ``bf16_operand`` until exit.  Scopes nest; the innermost match wins."""

    def __init__(self, params):
        # weights an enclosing scope already cast are served from there
        self.params = [p for p in params if p is not None and p.dtype == torch.float32 and not _in_scope(p)]

    def __enter__(self):
        outs = cast_multi_bf16(self.params)
        _CAST_SCOPES.append({id(p): (p, o) for p, o in zip(self.params, outs)})
        return self

    def __exit__(self, *exc):
        _CAST_SCOPES.pop()
        return False


def _in_scope(w) -> bool:
    return any(id(w) in sc and sc[id(w)][0] is w for sc in _CAST_SCOPES)


def bf16_operand(w: torch.Tensor) -> torch.Tensor:
    """bf16 GEMM operand of the weight w: the scope's copy if w was cast on scope entry
    (same tensor object, same storage), else a fresh cast."""
    for scope in reversed(_CAST_SCOPES):
        ent = scope.get(id(w))
        if ent is not None and ent[0] is w:
            return ent[1]
    if w.dtype == torch.bfloat16:
        return w.detach().contiguous()
    return cast(w.detach().contiguous(), torch.bfloat16)


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """Sum over all leading dims of x [..., C] -> f32 [C]."""
    require_gpu(x)
    C = x.shape[-1]
    rows = x.numel() // C if C else 0
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=x.device)
        accumulate = False
    call("lthm_colsum", ptr(x), dcode(x), rows, C, C, ptr(out), int(accumulate), stream())
    return out


# ----------------------------------------------------------------- dropout
def new_dropout_seed() -> int:
    """A fresh 62-bit dropout seed from torch's default (CPU) generator, so
    torch.manual_seed makes the masks reproducible; no device sync."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def dropout(x, p: float, seed: int, res1=None, res2=None, out_dtype=None):
    """[res1] + [res2] + dropout_p(x) with the hash mask of ``seed`` (lthm_dropout)."""
    require_gpu(x, res1, res2)
    _check(0.0 <= p < 1.0, f"dropout p must be in [0, 1), got {p}")
    for r in (res1, res2):
        _check(r is None or (r.dtype == torch.float32 and r.numel() == x.numel()), "dropout residual: f32, x's size")
    y = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    call("lthm_dropout", ptr(x), dcode(x), ptr(y), dcode(y), x.numel(), float(p), seed, ptr(res1), ptr(res2),
         stream())
    return y


def dropout_rows_(x, groups: int, p: float, seed: int):
    """In place: x [rows, groups * cols], row r of group g scaled by keep(g * rows + r) / (1 - p)."""
    require_gpu(x)
    _check(0.0 <= p < 1.0 and x.dim() == 2 and x.shape[1] % groups == 0, "dropout_rows_: bad arguments")
    call("lthm_dropout_rows", ptr(x), dcode(x), x.shape[0], x.shape[1] // groups, groups, float(p), seed, stream())
    return x


def dropout_mask(n: int, p: float, seed: int, device) -> torch.Tensor:
    """The keep decisions lthm_dropout applies to elements 0..n-1 (uint8)."""
    out = torch.empty(n, dtype=torch.uint8, device=device)
    require_gpu(out)
    call("lthm_dropout_mask", ptr(out), n, float(p), seed, stream())
    return out


class DropoutFn(torch.autograd.Function):
    """nn.Dropout(p) in training mode on the hash-mask kernel; the backward re-derives
    the mask from the saved seed."""

    @staticmethod
    def forward(ctx, x, p: float, seed: int):
        ctx.p, ctx.seed = p, seed
        return dropout(x.contiguous(), p, seed)

    @staticmethod
    def backward(ctx, dy):
        return dropout(dy.contiguous(), ctx.p, ctx.seed), None, None


# ----------------------------------------------------------------- GEMM
ACT_NONE, ACT_GELU, ACT_QGELU, ACT_GELU_GRAD, ACT_QGELU_GRAD = 0, 1, 2, 3, 4
# GELU whose aux_out receives GELU'(x), and the backward's plain multiply by that saved derivative
ACT_GELU_D, ACT_MUL_AUX = 5, 6
_ws_cache = {}


def _workspace(dev, nbytes: int) -> torch.Tensor:
    t = _ws_cache.get(dev)
    if t is None or t.numel() * 4 < nbytes:
        t = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        _ws_cache[dev] = t
    return t


GemmPlan = collections.namedtuple(
    "GemmPlan", "kernel ka kb bres epi spread splits combine amax fast_ok grid block tiles_m tiles_n walkers "
                "k_per_split ps_mode pp_mode pp_f8_mode wg_ragged")
GEMM_KERNELS = {-1: "NONE", 0: "K128", 1: "PS", 2: "WG", 3: "PP", 4: "PS_F8", 5: "PP_F8"}
GEMM_COMBINES = {0: "none", 1: "reduce", 2: "reduce4"}
GEMM_AMAX = {0: "none", 1: "kernel", 2: "after"}


def _gemm_desc(A, B, M, N, K, *, a_kcontig=True, b_kcontig=True, lda=None, ldb=None, out=None,
               out_dtype=torch.bfloat16, ldc=None, alpha=1.0, bias=None, act=ACT_NONE, aux=None, aux_out=None,
               res1=None, res2=None, batch=1, sA=0, sB=0, sC=0, splits=1, a_scale=None, b_scale=None, amax_out=None,
               ldaux=None, ldr1=None, ldr2=None, workspace=None):
    """The checked lthm_gemm_desc of a gemm() call: (descriptor, out, the tensors it points to)."""
    from ._lib import STRUCTS
    require_gpu(A, B)
    dev = A.device
    if out is None:
        shape = (batch, M, N) if batch > 1 else (M, N)
        out = torch.empty(shape, dtype=out_dtype, device=dev)
    lda_ = lda if lda is not None else (K if a_kcontig else M)
    ldb_ = ldb if ldb is not None else (K if b_kcontig else N)
    ldc_ = ldc if ldc is not None else N
    ldaux_ = ldaux if ldaux is not None else N
    ldr1_ = ldr1 if ldr1 is not None else N
    ldr2_ = ldr2 if ldr2 is not None else N
    sC_ = sC if sC else M * ldc_
    _check(min(M, N, K, batch) >= 1, f"bad GEMM dims M={M} N={N} K={K} batch={batch}")
    _check(lda_ >= (K if a_kcontig else M) and ldb_ >= (K if b_kcontig else N) and ldc_ >= N, "bad leading dims")
    _check(min(ldaux_, ldr1_, ldr2_) >= N, "bad epilogue leading dims")
    _need(A, (batch - 1) * sA + ((M - 1) * lda_ + K if a_kcontig else (K - 1) * lda_ + M), "A")
    _need(B, (batch - 1) * sB + ((N - 1) * ldb_ + K if b_kcontig else (K - 1) * ldb_ + N), "B")
    _need(out, (batch - 1) * sC_ + (M - 1) * ldc_ + N, "C")
    # the epilogue tensors of batch b start at b * M * ld (csrc/gemm.hip epilogue8)
    for t, ld, nm in ((aux, ldaux_, "aux"), (aux_out, ldaux_, "aux_out"), (res1, ldr1_, "res1"), (res2, ldr2_, "res2")):
        _need(t, (batch * M - 1) * ld + N, nm)
    _need(bias, N, "bias")
    d = STRUCTS["lthm_gemm_desc"]()
    d.A, d.B, d.C = ptr(A), ptr(B), ptr(out)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = lda_, ldb_, ldc_
    d.sA, d.sB, d.sC = sA, sB, sC_
    d.batch, d.a_kcontig, d.b_kcontig = batch, int(a_kcontig), int(b_kcontig)
    d.out_dtype = dcode(out)
    d.alpha, d.act = alpha, act
    d.bias = ptr(bias)
    d.aux, d.aux_out = ptr(aux), ptr(aux_out)
    d.ldaux = ldaux_
    d.res1, d.res2 = ptr(res1), ptr(res2)
    d.ldr1, d.ldr2 = ldr1_, ldr2_
    d.res1_dtype = dcode(res1) if res1 is not None else F32
    d.res2_dtype = dcode(res2) if res2 is not None else F32
    ws = workspace
    if ws is None and splits > 1:
        ws = _workspace(dev, splits * batch * M * N * 4)
    if ws is not None:
        _check(ws.dtype == torch.float32 and ws.is_cuda, "the split-K workspace is f32 device memory")
        d.workspace, d.workspace_bytes = ptr(ws), ws.numel() * 4
    d.splits = splits
    if amax_out is not None:
        _check(amax_out.dtype == torch.int32 and amax_out.is_cuda, "amax_out is an int32 device word")
        d.amax_out = ptr(amax_out)
    fp8 = A.dtype == torch.uint8
    if fp8:
        _check(B.dtype == torch.uint8 and a_scale is not None and b_scale is not None,
               "fp8 GEMM takes uint8 (e4m3) A and B with device scales")
        d.ab_dtype, d.a_scale, d.b_scale = FP8_E4M3, ptr(a_scale), ptr(b_scale)
    return d, out, ws


def gemm(A, B, M, N, K, *, a_kcontig=True, b_kcontig=True, lda=None, ldb=None, out=None,
         out_dtype=torch.bfloat16, ldc=None, alpha=1.0, bias=None, act=ACT_NONE, aux=None, aux_out=None,
         res1=None, res2=None, batch=1, sA=0, sB=0, sC=0, splits=1, a_scale=None, b_scale=None, amax_out=None,
         ldaux=None, ldr1=None, ldr2=None, workspace=None):
    """C = epi(alpha * A.B) on the MFMA GEMM kernel (include/lthm.h lthm_gemm).  uint8
    A / B are fp8 e4m3 bytes with per-tensor device scales a_scale / b_scale; amax_out
    (int32 [1] device word) receives the running max of |C| as f32 bits.  ldaux (aux and
    aux_out), ldr1 and ldr2 are the row strides of the epilogue tensors (default N);
    workspace: the caller's f32 split-K slabs (default: a cached one when splits > 1)."""
    import ctypes
    d, out, _ws = _gemm_desc(A, B, M, N, K, a_kcontig=a_kcontig, b_kcontig=b_kcontig, lda=lda, ldb=ldb, out=out,
                             out_dtype=out_dtype, ldc=ldc, alpha=alpha, bias=bias, act=act, aux=aux, aux_out=aux_out,
                             res1=res1, res2=res2, batch=batch, sA=sA, sB=sB, sC=sC, splits=splits, a_scale=a_scale,
                             b_scale=b_scale, amax_out=amax_out, ldaux=ldaux, ldr1=ldr1, ldr2=ldr2,
                             workspace=workspace)
    fp8 = A.dtype == torch.uint8
    key = "gemm_fp8" if fp8 else f"gemm_k<{int(a_kcontig)},{int(b_kcontig)}>"
    # compulsory HBM bytes (each operand read once, C written once, epilogue tensors):
    # with the flops this places the call on the roofline (bench.py encoder_gemm)
    nbytes = batch * (M * K * A.element_size() + N * K * B.element_size() + M * N * out.element_size())
    for t in (aux, aux_out, res1, res2):
        if t is not None:
            nbytes += M * N * batch * t.element_size()
    call("lthm_gemm", ctypes.addressof(d), stream(), _key=(_GEMM_TAG[-1] + ":" + key) if _GEMM_TAG else key,
         _work=2.0 * M * N * K * batch, _unit="flop", _bytes=float(nbytes))
    return out


def gemm_plan(A, B, M, N, K, *, cus=None, **kw):
    """The launch plan lthm_gemm takes for gemm(A, B, M, N, K, **kw) on a device of ``cus``
    compute units (default: A's device), as a GemmPlan (include/lthm.h lthm_gemm_plan_out;
    kernel, combine and amax by name).  Nothing is launched."""
    import ctypes
    from ._lib import STRUCTS
    d, _out, _ws = _gemm_desc(A, B, M, N, K, **kw)
    if cus is None:
        cus = torch.cuda.get_device_properties(A.device).multi_processor_count
    p = STRUCTS["lthm_gemm_plan_out"]()
    rc = load().lthm_gemm_plan(ctypes.addressof(d), int(cus), ctypes.addressof(p))
    if rc != 0:
        raise OperandError(f"lthm_gemm refuses this descriptor (error {rc})")
    return GemmPlan(GEMM_KERNELS[p.kernel], p.ka, p.kb, p.bres, p.epi, p.spread, p.splits, GEMM_COMBINES[p.combine],
                    GEMM_AMAX[p.amax], p.fast_ok, (p.grid_x, p.grid_y, p.grid_z), p.block, p.tiles_m, p.tiles_n,
                    p.walkers, p.k_per_split, p.ps_mode, p.pp_mode, p.pp_f8_mode, p.wg_ragged)


# Kernel-timer key prefix for the GEMMs launched inside a ``gemm_tag`` scope (bench.py
# reports the encoder GEMMs -- the north star's MFMA target -- apart from the rest).
_GEMM_TAG: list = []


class gemm_tag:
    def __init__(self, tag: str):
        self.tag = tag

    def __enter__(self):
        _GEMM_TAG.append(self.tag)

    def __exit__(self, *exc):
        _GEMM_TAG.pop()
        return False


FP8_E4M3 = 2


def quantize_fp8(x, amax=None):
    """Per-tensor e4m3 quantisation (include/lthm.h lthm_quantize_fp8): -> (q uint8 of
    x's shape, scale f32 [1] on the device) with x = q * scale up to e4m3 rounding.
    amax: the int32 [1] word a producer already reduced max |x| into (layernorm_fwd /
    gemm amax_out / amax_): x is then read once (lthm_quantize_fp8_amax)."""
    require_gpu(x)
    n = x.numel()
    _check(n % 8 == 0, "quantize_fp8 takes n % 8 == 0")
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    if amax is not None:
        _check(amax.dtype == torch.int32 and amax.is_cuda, "amax is an int32 device word")
        call("lthm_quantize_fp8_amax", ptr(x), dcode(x), n, ptr(amax), ptr(q), ptr(scale), stream(),
             _key="quantize_fp8", _work=n * (x.element_size() + 1), _unit="byte")
        return q, scale
    work = torch.empty(1, dtype=torch.int32, device=x.device)
    call("lthm_quantize_fp8", ptr(x), dcode(x), n, ptr(q), ptr(scale), ptr(work), stream(), _key="quantize_fp8",
         _work=n * (x.element_size() * 2 + 1), _unit="byte")
    return q, scale


def amax_(x, amax):
    """amax (int32 [1] device word) = max(amax, max |x|) as f32 bits (lthm_amax)."""
    require_gpu(x, amax)
    _check(x.numel() % 8 == 0 and amax.dtype == torch.int32, "amax_ takes n % 8 == 0 and an int32 word")
    call("lthm_amax", ptr(x), dcode(x), x.numel(), ptr(amax), stream(), _key="amax",
         _work=x.numel() * x.element_size(), _unit="byte")
    return amax


def linear_fwd_fp8(xq, xs, wq, ws, bias=None, act=ACT_NONE, aux_out=None, res1=None, res2=None,
                   out_dtype=torch.bfloat16, amax_out=None):
    """y = act(xs ws (xq wq^T) + b) (+ res1 + res2) on the fp8 MFMA: xq [M, K], wq [N, K] e4m3 bytes."""
    M, K_ = xq.shape
    N = wq.shape[0]
    return gemm(xq, wq, M, N, K_, bias=bias, act=act, aux_out=aux_out, res1=res1, res2=res2, out_dtype=out_dtype,
                a_scale=xs, b_scale=ws, amax_out=amax_out)


def _splits_for(M: int, N: int, K: int) -> int:
    """Split-K factor (and so the f32 partial-slab workspace) for tall reductions
    (weight gradients): ~2 waves of 128 x 128 tiles on 256 CUs for the one-tile
    kernel, or one 256 x 256 tile per CU for gemm_wg_k (csrc/gemm.hip), whichever
    is larger; the library picks its kernel and uses at most this many splits."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 256 or K < 4096:
        return 1
    s = max(1, min(512 // tiles, K // 2048))
    tiles256 = ((M + 255) // 256) * ((N + 255) // 256)
    return max(s, min(256 // tiles256, K // 256))


def linear_fwd(x2d, w_bf16, bias=None, act=ACT_NONE, aux_out=None, res1=None, res2=None, out_dtype=torch.bfloat16):
    """y = act(x W^T + b) (+ res1 + res2). x2d [M, K] bf16, w [N, K] bf16."""
    M, K_ = x2d.shape
    N = w_bf16.shape[0]
    return gemm(x2d, w_bf16, M, N, K_, bias=bias, act=act, aux_out=aux_out, res1=res1, res2=res2,
                out_dtype=out_dtype)


_DGRAD_WT = os.environ.get("LTHM_DGRAD_WT", "1") == "1"
# W^T copies of the bf16 weight operands, reused by every dgrad of one backward (the c_attn and
# c_fc dgrads of a block run twice when the LayerNorm backward is fused into them, and the same
# copy serves recomputed blocks): keyed by the operand object, valid while its version holds
_WT_CACHE = collections.OrderedDict()
_WT_CACHE_MAX = 64


def weight_t(w_bf16: torch.Tensor) -> torch.Tensor:
    """w_bf16.t().contiguous(), cached per operand tensor (bounded LRU; entries hold the operand,
    so its id cannot be reused while cached, and a torch in-place write bumps its version)."""
    ent = _WT_CACHE.get(id(w_bf16))
    if ent is not None and ent[0] is w_bf16 and ent[1] == w_bf16._version:
        _WT_CACHE.move_to_end(id(w_bf16))
        return ent[2]
    wt = w_bf16.t().contiguous()
    _WT_CACHE[id(w_bf16)] = (w_bf16, w_bf16._version, wt)
    while len(_WT_CACHE) > _WT_CACHE_MAX:
        _WT_CACHE.popitem(last=False)
    return wt


def linear_dgrad(dy2d, w_bf16, act_grad=ACT_NONE, aux=None, out_dtype=torch.bfloat16, res1=None):
    """dx = (dy W) [* act'(aux)].  dy [M, N] bf16, w [N, K] bf16.  B is a K-contiguous W^T
    copy (the forward kernel form; tools/ab_dgrad_wt.sh: C5 encoder dgrad 1.39 -> 1.29 ms per
    call, C2 encoder forward + dgrad GEMMs 14.27 -> 14.06 ms per step); LTHM_DGRAD_WT=0
    reads W K-strided."""
    M, N = dy2d.shape
    K_ = w_bf16.shape[1]
    if _DGRAD_WT:
        wt = weight_t(w_bf16)
        return gemm(dy2d, wt, M, K_, N, act=act_grad, aux=aux, out_dtype=out_dtype, res1=res1)
    return gemm(dy2d, w_bf16, M, K_, N, a_kcontig=True, b_kcontig=False, ldb=K_, act=act_grad, aux=aux,
                out_dtype=out_dtype, res1=res1)


def linear_wgrad(dy2d, x2d, out=None, accumulate=False):
    """dW = dy^T x  -> f32 [N, K].  dy [M, N] bf16, x [M, K] bf16 (both K-strided over M)."""
    M, N = dy2d.shape
    K_ = x2d.shape[1]
    res = out if (accumulate and out is not None) else None
    s = _splits_for(N, K_, M)
    return gemm(dy2d, x2d, N, K_, M, a_kcontig=False, b_kcontig=False, lda=N, ldb=K_, out=out,
                out_dtype=torch.float32, res1=res, splits=s)


# ----------------------------------------------------------------- fused MLP
def mlp_supported(D: int, HID: int) -> bool:
    """Shapes the fused MLP kernels take (include/lthm.h lthm_mlp_supported)."""
    from ._lib import load
    return bool(load().lthm_mlp_supported(D, HID))


MLP_ENTRIES = {"fwd": 0, "fwd_ln": 1, "bwd": 2, "bwd_hidden": 3, "bwd_dx": 4, "wgrad": 5}
MlpPlan = collections.namedtuple(
    "MlpPlan", "entry waves tile_rows grid max_tiles nslice ngroup full ntiles ws_bytes lds_static lds_dynamic")


def mlp_plan(entry: str, M: int, D: int, HID: int, cus=None):
    """The launch geometry of a fused-MLP entry point ("fwd", "fwd_ln", "bwd", "bwd_hidden", "bwd_dx",
    "wgrad") on a device of ``cus`` compute units (default: the current device), as an MlpPlan
    (include/lthm.h lthm_mlp_plan_out).  Nothing is launched; OperandError for a refused shape."""
    import ctypes
    from ._lib import STRUCTS, load
    if cus is None:
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    p = STRUCTS["lthm_mlp_plan_out"]()
    rc = load().lthm_mlp_plan(MLP_ENTRIES[entry], int(M), int(D), int(HID), int(cus), ctypes.addressof(p))
    if rc != 0:
        raise OperandError(f"the fused MLP's {entry} entry refuses M={M} D={D} HID={HID} (error {rc})")
    return MlpPlan(entry, p.waves, p.tile_rows, p.grid, p.max_tiles, p.nslice, p.ngroup, p.full, p.ntiles,
                   p.ws_bytes, p.lds_static, p.lds_dynamic)


PTowerPlan = collections.namedtuple(
    "PTowerPlan", "path total R R32 nslab nslice rows_dm rows_full nf dma opl rows_grid emb_grid_x emb_grid_y "
                  "tok_grid rows_lds_static emb_lds_dynamic tok_lds_dynamic")


def product_tower_plan(desc):
    """Which kernels lthm_product_tower_fwd runs for ``desc`` (a filled STRUCTS["lthm_ptower_desc"]) and
    their geometry, as a PTowerPlan (include/lthm.h lthm_ptower_plan_out; path "mfma" or "token").
    Nothing is launched and no pointer is followed; OperandError for a refused descriptor."""
    import ctypes
    from ._lib import STRUCTS, load
    p = STRUCTS["lthm_ptower_plan_out"]()
    rc = load().lthm_product_tower_plan(ctypes.addressof(desc), ctypes.addressof(p))
    if rc != 0:
        raise OperandError(f"lthm_product_tower_fwd refuses this descriptor (error {rc})")
    return PTowerPlan("mfma" if p.path == 1 else "token", *[getattr(p, f) for f in PTowerPlan._fields[1:]])


def mlp_fwd(x2d, w1_b, b1, w2t_b, b2, res1=None, res2=None):
    """res1 [+ res2] + c_proj(GELU(c_fc(x))) in one kernel, hidden on chip (lthm_mlp_fwd).
    x2d [M, D] bf16, w1_b [HID, D] bf16 (c_fc.weight), w2t_b [HID, D] bf16 (c_proj.weight^T)."""
    require_gpu(x2d, w1_b, w2t_b)
    M, D = x2d.shape
    HID = w1_b.shape[0]
    _check(x2d.dtype == torch.bfloat16 and w1_b.dtype == torch.bfloat16 and w2t_b.dtype == torch.bfloat16,
           "mlp_fwd takes bf16 x / weights")
    _check(mlp_supported(D, HID), f"fused MLP does not take D={D} HID={HID}")
    _check(tuple(w1_b.shape) == (HID, D) and tuple(w2t_b.shape) == (HID, D), "mlp_fwd: weight shapes")
    for t in (x2d, w1_b, w2t_b, b1, b2, res1, res2):
        _check(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0), "mlp_fwd: contiguous 16-B aligned operands")
    for t, n in ((b1, HID), (b2, D)):
        _check(t is None or (t.dtype == torch.float32 and t.numel() == n), "mlp_fwd: f32 biases")
    for t in (res1, res2):
        _check(t is None or (t.dtype == torch.float32 and t.numel() == M * D), "mlp_fwd: f32 [M, D] residuals")
    out = torch.empty((M, D), dtype=torch.float32, device=x2d.device)
    # compulsory HBM bytes: x bf16, the residuals and out f32 (the hidden never leaves the chip)
    nbytes = M * D * (2 + 4 + 4 * sum(t is not None for t in (res1, res2)))
    call("lthm_mlp_fwd", ptr(x2d), M, D, HID, ptr(w1_b), ptr(b1), ptr(w2t_b), ptr(b2), ptr(res1), ptr(res2),
         ptr(out), stream(), _key=(_GEMM_TAG[-1] + ":mlp_fwd") if _GEMM_TAG else "mlp_fwd",
         _work=4.0 * M * D * HID, _unit="flop", _bytes=float(nbytes))
    return out


def mlp_fwd_ln(x32, ln_w, ln_b, w1_b, b1, w2t_b, b2, res1=None, res2=None, save=True):
    """res1 [+ res2] + c_proj(GELU(c_fc(LayerNorm(x32)))) in one kernel (lthm_mlp_fwd_ln) ->
    (out f32 [M, D], h bf16 [M, D], mean, rstd) -- h / mean / rstd None unless ``save``."""
    require_gpu(x32, w1_b, w2t_b)
    M, D = x32.shape
    HID = w1_b.shape[0]
    _check(x32.dtype == torch.float32 and w1_b.dtype == torch.bfloat16 and w2t_b.dtype == torch.bfloat16,
           "mlp_fwd_ln takes f32 x and bf16 weights")
    _check(mlp_supported(D, HID), f"fused MLP does not take D={D} HID={HID}")
    _check(tuple(w1_b.shape) == (HID, D) and tuple(w2t_b.shape) == (HID, D), "mlp_fwd_ln: weight shapes")
    for t in (x32, w1_b, w2t_b, b1, b2, res1, res2, ln_w, ln_b):
        _check(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0), "mlp_fwd_ln: contiguous aligned operands")
    for t, n in ((b1, HID), (b2, D), (ln_w, D), (ln_b, D)):
        _check(t is None or (t.dtype == torch.float32 and t.numel() == n), "mlp_fwd_ln: f32 vectors")
    for t in (res1, res2):
        _check(t is None or (t.dtype == torch.float32 and t.numel() == M * D), "mlp_fwd_ln: f32 [M, D] residuals")
    dev = x32.device
    out = torch.empty((M, D), dtype=torch.float32, device=dev)
    h = torch.empty((M, D), dtype=torch.bfloat16, device=dev) if save else None
    mean = torch.empty(M, dtype=torch.float32, device=dev) if save else None
    rstd = torch.empty(M, dtype=torch.float32, device=dev) if save else None
    call("lthm_mlp_fwd_ln", ptr(x32), ptr(ln_w), ptr(ln_b), M, D, HID, ptr(w1_b), ptr(b1), ptr(w2t_b), ptr(b2),
         ptr(res1), ptr(res2), ptr(out), ptr(h), ptr(mean), ptr(rstd), stream(),
         _key=(_GEMM_TAG[-1] + ":mlp_fwd") if _GEMM_TAG else "mlp_fwd", _work=4.0 * M * D * HID, _unit="flop")
    return out, h, mean, rstd


# LTHM_MLP_BWD=fused: one kernel also accumulates dX (one wave per SIMD); default: the split form
_MLP_BWD_SPLIT = os.environ.get("LTHM_MLP_BWD", "split") != "fused"


def mlp_bwd(x2d, dy2d, w1_b, b1, w2t_b, dx_dtype=torch.bfloat16, want_dx=True):
    """Backward of the fused MLP with the hidden recomputed (lthm_mlp_bwd): -> (dx [M, D],
    g [M, HID] = GELU(pre) bf16, dpre [M, HID] bf16).  x2d / dy2d [M, D] bf16.  want_dx=False:
    dx is None where the split path would run dX = dpre W1 on the GEMM (the caller runs it, e.g.
    fused with the LayerNorm backward: dgrad_layernorm_bwd)."""
    require_gpu(x2d, dy2d, w1_b, w2t_b)
    M, D = x2d.shape
    HID = w1_b.shape[0]
    _check(x2d.dtype == torch.bfloat16 and dy2d.dtype == torch.bfloat16 and w1_b.dtype == torch.bfloat16
           and w2t_b.dtype == torch.bfloat16, "mlp_bwd takes bf16 x / dy / weights")
    _check(mlp_supported(D, HID), f"fused MLP does not take D={D} HID={HID}")
    _check(tuple(dy2d.shape) == (M, D) and tuple(w1_b.shape) == (HID, D) and tuple(w2t_b.shape) == (HID, D),
           "mlp_bwd: shapes")
    for t in (x2d, dy2d, w1_b, w2t_b, b1):
        _check(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0), "mlp_bwd: contiguous 16-B aligned operands")
    _check(b1 is None or (b1.dtype == torch.float32 and b1.numel() == HID), "mlp_bwd: f32 b1")
    dev = x2d.device
    g = torch.empty((M, HID), dtype=torch.bfloat16, device=dev)
    dpre = torch.empty((M, HID), dtype=torch.bfloat16, device=dev)
    if _MLP_BWD_SPLIT and HID <= 4096:
        # recompute kernel for G / dP at two waves per SIMD, then dX = dP W1 on the GEMM
        # compulsory HBM bytes: x, dy read (bf16), g and dpre written (bf16 [M, HID] each)
        call("lthm_mlp_bwd_hidden", ptr(x2d), ptr(dy2d), M, D, HID, ptr(w1_b), ptr(b1), ptr(w2t_b), ptr(g), ptr(dpre),
             stream(), _key=(_GEMM_TAG[-1] + ":mlp_bwd") if _GEMM_TAG else "mlp_bwd", _work=4.0 * M * D * HID,
             _unit="flop", _bytes=float(M * (4 * D + 4 * HID)))
        return (linear_dgrad(dpre, w1_b, out_dtype=dx_dtype) if want_dx else None), g, dpre
    dx = torch.empty((M, D), dtype=dx_dtype, device=dev)
    call("lthm_mlp_bwd", ptr(x2d), ptr(dy2d), M, D, HID, ptr(w1_b), ptr(b1), ptr(w2t_b), ptr(dx), dcode(dx),
         ptr(g), ptr(dpre), stream(), _key=(_GEMM_TAG[-1] + ":mlp_bwd") if _GEMM_TAG else "mlp_bwd",
         _work=6.0 * M * D * HID, _unit="flop")
    return dx, g, dpre


def mlp_wgrad_supported(D: int, HID: int) -> bool:
    return mlp_supported(D, HID) and HID % 128 == 0 and HID <= 4096


def mlp_bwd_dx(x2d, dy2d, w1_b, b1, w2t_b, dx_dtype=torch.bfloat16):
    """dX of the fused MLP with the hidden recomputed and nothing else written
    (lthm_mlp_bwd_dx): x2d / dy2d [M, D] bf16 -> dx [M, D] in dx_dtype."""
    require_gpu(x2d, dy2d, w1_b, w2t_b)
    M, D = x2d.shape
    HID = w1_b.shape[0]
    _check(x2d.dtype == torch.bfloat16 and dy2d.dtype == torch.bfloat16 and w1_b.dtype == torch.bfloat16
           and w2t_b.dtype == torch.bfloat16, "mlp_bwd_dx takes bf16 x / dy / weights")
    _check(mlp_supported(D, HID), f"fused MLP does not take D={D} HID={HID}")
    _check(tuple(dy2d.shape) == (M, D) and tuple(w1_b.shape) == (HID, D) and tuple(w2t_b.shape) == (HID, D),
           "mlp_bwd_dx: shapes")
    for t in (x2d, dy2d, w1_b, w2t_b, b1):
        _check(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0), "mlp_bwd_dx: contiguous aligned operands")
    _check(b1 is None or (b1.dtype == torch.float32 and b1.numel() == HID), "mlp_bwd_dx: f32 b1")
    dx = torch.empty((M, D), dtype=dx_dtype, device=x2d.device)
    # compulsory HBM bytes: x, dy read, dx written
    call("lthm_mlp_bwd_dx", ptr(x2d), ptr(dy2d), M, D, HID, ptr(w1_b), ptr(b1), ptr(w2t_b), ptr(dx), dcode(dx),
         stream(), _key=(_GEMM_TAG[-1] + ":mlp_bwd") if _GEMM_TAG else "mlp_bwd", _work=6.0 * M * D * HID,
         _unit="flop", _bytes=float(M * D * (4 + dx.element_size())))
    return dx


def mlp_wgrad(x2d, dy2d, w1_b, b1, w2t_b, want_db1=True):
    """Weight gradients of the fused MLP with the hidden recomputed in the kernel (lthm_mlp_wgrad):
    -> (dW1 f32 [HID, D] = dP^T x, dW2 f32 [D, HID] = dY^T G, db1 f32 [HID] = colsum dP or None)."""
    from ._lib import load
    require_gpu(x2d, dy2d, w1_b, w2t_b)
    M, D = x2d.shape
    HID = w1_b.shape[0]
    _check(x2d.dtype == torch.bfloat16 and dy2d.dtype == torch.bfloat16 and w1_b.dtype == torch.bfloat16
           and w2t_b.dtype == torch.bfloat16, "mlp_wgrad takes bf16 x / dy / weights")
    _check(mlp_wgrad_supported(D, HID), f"mlp_wgrad does not take D={D} HID={HID}")
    _check(tuple(dy2d.shape) == (M, D) and tuple(w1_b.shape) == (HID, D) and tuple(w2t_b.shape) == (HID, D),
           "mlp_wgrad: shapes")
    for t in (x2d, dy2d, w1_b, w2t_b, b1):
        _check(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0), "mlp_wgrad: contiguous aligned operands")
    _check(b1 is None or (b1.dtype == torch.float32 and b1.numel() == HID), "mlp_wgrad: f32 b1")
    dev = x2d.device
    dw1 = torch.empty((HID, D), dtype=torch.float32, device=dev)
    dw2 = torch.empty((D, HID), dtype=torch.float32, device=dev)
    db1 = torch.empty(HID, dtype=torch.float32, device=dev) if want_db1 else None
    wsb = int(load().lthm_mlp_wgrad_ws_bytes(M, D, HID))
    _check(wsb >= 0, "mlp_wgrad: workspace size")
    ws = _workspace(dev, wsb)
    # compulsory HBM bytes: x and dy read, the two weight gradients written (f32)
    call("lthm_mlp_wgrad", ptr(x2d), ptr(dy2d), M, D, HID, ptr(w1_b), ptr(b1), ptr(w2t_b), ptr(dw1), ptr(dw2),
         ptr(db1), ptr(ws), ws.numel() * 4, stream(),
         _key=(_GEMM_TAG[-1] + ":mlp_wgrad") if _GEMM_TAG else "mlp_wgrad", _work=8.0 * M * D * HID, _unit="flop",
         _bytes=float(M * D * 4 + 8 * HID * D))
    return dw1, dw2, db1


# ----------------------------------------------------------------- row gather
def rows_gather(src2d, idx, out=None):
    """dst[i] = src2d[idx[i]] (a zero row where idx[i] < 0), idx int32 on the device, rows of a
    multiple of 16 bytes (lthm_rows_move).  ``out`` may be ``src2d`` itself only when every
    idx[i] is i or negative (zeroing rows in place)."""
    require_gpu(src2d, idx)
    _check(src2d.dim() == 2 and src2d.is_contiguous() and idx.dtype == torch.int32 and idx.is_contiguous(),
           "rows_gather takes a contiguous [n, W] source and int32 indices")
    rb = src2d.shape[1] * src2d.element_size()
    _check(rb % 16 == 0 and src2d.data_ptr() % 16 == 0, "rows_gather: 16-B rows")
    c = idx.numel()
    dst = out if out is not None else torch.empty((c, src2d.shape[1]), dtype=src2d.dtype, device=src2d.device)
    _check(dst.is_contiguous() and tuple(dst.shape) == (c, src2d.shape[1]) and dst.dtype == src2d.dtype,
           "rows_gather: destination shape")
    call("lthm_rows_move", ptr(src2d), rb, ptr(idx), c, ptr(dst), rb, rb, 0, stream(), _work=2.0 * c * rb,
         _unit="byte")
    return dst


# ----------------------------------------------------------------- LayerNorm
def layernorm_fwd(x2d, w, b, y_dtype=torch.bfloat16, amax=None):
    """amax: optional int32 [1] device word (zeroed by the caller) that receives the
    running max of |y| as f32 bits -- the fp8 quantisation's reduction, fused."""
    require_gpu(x2d, w)
    M, D = x2d.shape
    _need(w, D, "ln weight")
    _need(b, D, "ln bias")
    y = torch.empty((M, D), dtype=y_dtype, device=x2d.device)
    mean = torch.empty(M, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x2d.device)
    # algorithmic bytes: x read, y written, the row statistics written
    nb = float(M * D * (x2d.element_size() + y.element_size()) + 8 * M)
    if amax is not None:
        _check(amax.dtype == torch.int32 and amax.is_cuda, "amax is an int32 device word")
        call("lthm_layernorm_fwd_amax", ptr(x2d), M, D, ptr(w), ptr(b), ptr(y), dcode(y), ptr(mean), ptr(rstd),
             ptr(amax), stream(), _work=nb, _unit="byte")
    else:
        call("lthm_layernorm_fwd", ptr(x2d), M, D, ptr(w), ptr(b), ptr(y), dcode(y), ptr(mean), ptr(rstd), stream(),
             _work=nb, _unit="byte")
    return y, mean, rstd


def dgrad_layernorm_bwd_ok(dy2d, w_bf16, x2d) -> bool:
    """Shapes lthm_dgrad_layernorm_bwd takes: LayerNorm width 256 (one column tile of whole
    rows), the dgrad's reduction dim a multiple of 64, 16-B aligned contiguous operands."""
    M, N = dy2d.shape
    return (_LN_DGRAD and x2d.shape[1] == 256 and tuple(w_bf16.shape) == (N, 256) and N % 64 == 0
            and dy2d.dtype == torch.bfloat16 and w_bf16.dtype == torch.bfloat16 and x2d.dtype == torch.float32
            and dy2d.is_contiguous() and x2d.is_contiguous() and dy2d.data_ptr() % 16 == 0
            and x2d.data_ptr() % 16 == 0 and x2d.shape[0] == M)


def dgrad_layernorm_bwd(dy2d, w_bf16, x2d, w, mean, rstd, res1=None, res2=None, want_bf16=True, need_bias=True,
                        res1_twice=False):
    """layernorm_bwd(linear_dgrad(dy2d, w_bf16), x2d, ...) in one kernel (lthm_dgrad_layernorm_bwd):
    dh = dy W stays on chip (f32) and the 256-row GEMM tiles finish the LayerNorm backward.
    -> (dx f32, dx bf16 or None, dw, db or None)."""
    from ._lib import load
    require_gpu(dy2d, w_bf16, x2d)
    _check(dgrad_layernorm_bwd_ok(dy2d, w_bf16, x2d), "dgrad_layernorm_bwd: unsupported shapes")
    M, N = dy2d.shape
    D = 256
    for t, nm in ((res1, "res1"), (res2, "res2")):
        _need(t, M * D, nm)
        _check(t is None or (t.dtype == torch.float32 and t.data_ptr() % 16 == 0), f"{nm}: 16-B aligned f32")
    _need(w, D, "ln weight")
    _check(w.dtype == torch.float32 and w.data_ptr() % 16 == 0, "ln weight: 16-B aligned f32")
    _need(mean, M, "mean")
    _need(rstd, M, "rstd")
    _check(not res1_twice or res1 is not None, "dgrad_layernorm_bwd(res1_twice) needs res1")
    wt = weight_t(w_bf16)
    tiles = int(load().lthm_dgrad_layernorm_bwd_tiles(M))
    part = torch.empty((2, tiles, D), dtype=torch.float32, device=x2d.device)
    dx = torch.empty((M, D), dtype=torch.float32, device=x2d.device)
    dxb = torch.empty((M, D), dtype=torch.bfloat16, device=x2d.device) if want_bf16 else None
    # compulsory HBM bytes: dy read, x and the residuals read, dx (and its bf16 copy) written
    nb = float(M * N * 2 + M * D * (4 + 4 + (4 if res1 is not None else 0) + (4 if res2 is not None else 0)
                                    + (2 if want_bf16 else 0)) + 8 * M)
    call("lthm_dgrad_layernorm_bwd", ptr(dy2d), ptr(wt), M, D, N, ptr(x2d), ptr(w), ptr(mean), ptr(rstd), ptr(res1),
         ptr(res2), ptr(dx), ptr(dxb), ptr(part), 1 if res1_twice else 0, stream(),
         _key=(_GEMM_TAG[-1] + ":dgrad_ln") if _GEMM_TAG else "dgrad_ln", _work=2.0 * M * N * D, _unit="flop",
         _bytes=nb)
    dw = colsum(part[0])
    db = colsum(part[1]) if need_bias else None
    return dx, dxb, dw, db


# LTHM_LN_DGRAD=0: the dgrad GEMM writes dh (bf16) and the LayerNorm backward runs as its own pass
_LN_DGRAD = os.environ.get("LTHM_LN_DGRAD", "1") != "0"
# LTHM_LN_LINEAR=0: the c_proj GEMM writes x1 and ln_2's forward runs as its own pass
_LN_LINEAR = os.environ.get("LTHM_LN_LINEAR", "1") != "0"


def _ln_epi_operands_ok(M, bias, res1, ln_w, ln_b):
    """The epilogue operands of lthm_linear_layernorm_fwd: contiguous 16-B aligned f32 of the
    right size (bias / ln_b may be absent, ln_w may not)."""
    if ln_w is None:
        return False
    for t, n in ((bias, 256), (ln_w, 256), (ln_b, 256), (res1, M * 256)):
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
                                  and t.numel() == n):
            return False
    return True


def linear_layernorm_fwd_ok(x2d, w_bf16, bias=None, res1=None, ln_w=None, ln_b=None, check_epi=True) -> bool:
    """Shapes lthm_linear_layernorm_fwd takes: output width 256, K a multiple of 64, aligned, and
    (check_epi) f32 epilogue operands it can read directly -- a caller whose residual or LayerNorm
    parameters fail this drops to the unfused GEMM + LayerNorm path instead of raising."""
    M, Kd = x2d.shape
    return (_LN_LINEAR and tuple(w_bf16.shape) == (256, Kd) and Kd % 64 == 0 and x2d.dtype == torch.bfloat16
            and w_bf16.dtype == torch.bfloat16 and x2d.is_contiguous() and w_bf16.is_contiguous()
            and x2d.data_ptr() % 16 == 0 and w_bf16.data_ptr() % 16 == 0
            and (not check_epi or _ln_epi_operands_ok(M, bias, res1, ln_w, ln_b)))


def linear_layernorm_fwd(x2d, w_bf16, bias, res1, ln_w, ln_b):
    """x1 = res1 + x W^T + bias (f32) and LayerNorm(x1) in one kernel (lthm_linear_layernorm_fwd)
    -> (x1 f32 [M, 256], h bf16 [M, 256], mean, rstd)."""
    require_gpu(x2d, w_bf16)
    _check(linear_layernorm_fwd_ok(x2d, w_bf16, check_epi=False), "linear_layernorm_fwd: unsupported shapes")
    M, Kd = x2d.shape
    for t, n, nm in ((bias, 256, "bias"), (ln_w, 256, "ln weight"), (ln_b, 256, "ln bias"), (res1, M * 256, "res1")):
        _check(t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
                             and t.numel() == n), f"linear_layernorm_fwd: {nm} must be contiguous aligned f32 [{n}]")
    _check(ln_w is not None, "linear_layernorm_fwd: ln weight")
    dev = x2d.device
    x1 = torch.empty((M, 256), dtype=torch.float32, device=dev)
    h = torch.empty((M, 256), dtype=torch.bfloat16, device=dev)
    mean = torch.empty(M, dtype=torch.float32, device=dev)
    rstd = torch.empty(M, dtype=torch.float32, device=dev)
    # compulsory HBM bytes: x read, the residual read, x1 (f32) and h (bf16) written, the statistics
    nb = float(M * Kd * 2 + M * 256 * ((4 if res1 is not None else 0) + 4 + 2) + 8 * M)
    call("lthm_linear_layernorm_fwd", ptr(x2d), ptr(w_bf16), ptr(bias), ptr(res1), M, 256, Kd, ptr(ln_w), ptr(ln_b),
         ptr(x1), ptr(h), ptr(mean), ptr(rstd), stream(),
         _key=(_GEMM_TAG[-1] + ":linear_ln") if _GEMM_TAG else "linear_ln", _work=2.0 * M * Kd * 256, _unit="flop",
         _bytes=nb)
    return x1, h, mean, rstd


def layernorm_bwd(dy2d, x2d, w, mean, rstd, res1=None, res2=None, want_bf16=True, need_bias=True, res1_twice=False):
    """dx = LN'(dy) + res1 + res2 (f32) and its bf16 copy.  res1_twice: the f32 dx carries res1
    once more than the bf16 copy (lthm_layernorm_bwd_ex flag 1)."""
    from ._lib import load
    M, D = x2d.shape
    for t, nm in ((dy2d, "dy"), (res1, "res1"), (res2, "res2")):
        _need(t, M * D, nm)
    _need(w, D, "ln weight")
    _need(mean, M, "mean")
    _need(rstd, M, "rstd")
    nblk = load().lthm_layernorm_bwd_blocks(M)
    part = torch.empty((2, nblk, D), dtype=torch.float32, device=x2d.device)
    dx = torch.empty((M, D), dtype=torch.float32, device=x2d.device)
    dxb = torch.empty((M, D), dtype=torch.bfloat16, device=x2d.device) if want_bf16 else None
    # algorithmic bytes: dy, x and the residuals read, dx (and its bf16 copy) written, the row
    # statistics read, the per-block weight-gradient partials written
    nb = float(M * D * (dy2d.element_size() + x2d.element_size() + 4 + (4 if res1 is not None else 0)
                        + (4 if res2 is not None else 0) + (2 if want_bf16 else 0)) + 8 * M + part.numel() * 4)
    if res1_twice:
        _check(res1 is not None and D % 4 == 0, "layernorm_bwd(res1_twice): res1 and D % 4 == 0")
        call("lthm_layernorm_bwd_ex", ptr(dy2d), dcode(dy2d), ptr(x2d), M, D, ptr(w), ptr(mean), ptr(rstd), ptr(res1),
             ptr(res2), ptr(dx), ptr(dxb), ptr(part), 1, stream(), _key="lthm_layernorm_bwd", _work=nb, _unit="byte")
    else:
        call("lthm_layernorm_bwd", ptr(dy2d), dcode(dy2d), ptr(x2d), M, D, ptr(w), ptr(mean), ptr(rstd), ptr(res1),
             ptr(res2), ptr(dx), ptr(dxb), ptr(part), stream(), _work=nb, _unit="byte")
    dw = colsum(part[0])
    db = colsum(part[1]) if need_bias else None
    return dx, dxb, dw, db


# ----------------------------------------------------------------- attention
_MASK_OK: dict = {}


def attn_mask_ok(T, E):
    """A general additive mask is served at this (T, E), forward and backward: the C
    dispatcher's own test (lthm_attn_mask_ok)."""
    key = (int(T), int(E))
    ok = _MASK_OK.get(key)
    if ok is None:
        from ._lib import load
        ok = _MASK_OK[key] = bool(load().lthm_attn_mask_ok(key[0], key[1]))
    return ok


def _check_mask_limit(T, E):
    _check(attn_mask_ok(T, E),
           f"a general additive attn_mask is supported for T <= 256 with E = 16 / 32 / 64 and T <= 149 with E = 128 "
           f"(the masked backward keeps Q, K, V and dO of one head in LDS: T (8 E + 72) + 16 bytes <= 160 KiB); "
           f"got T={T} E={E}")


def attn_mask_operand(mask, B, H, T, E=None):
    """The reference's additive attn_mask (broadcast onto the [B, H, T, T] scores,
    commons/transformers/layers.py:57-58) as an f32 operand with its broadcast
    strides: [T, T], [B or 1, T, T] or [B or 1, H or 1, T, T].

    Limit: the masked kernels hold one head whole in LDS, and the backward (Q, K, V, dO and the
    row buffers: T (8 E + 72) + 16 bytes of 160 KiB) is the larger of the two, so a mask is taken
    for T <= 256 at E = 16 / 32 / 64 and for T <= 149 at E = 128 (lthm_attn_mask_ok).  With E
    given, a shape past the limit is refused here; without it only T <= 256 is checked here and
    the (T, E) limit when the forward's descriptor is built (_attn_desc), still before any launch."""
    if mask is None:
        return None
    require_gpu(mask)
    m = mask.to(torch.float32)
    while m.dim() < 4:
        m = m.unsqueeze(0 if m.dim() != 3 else 1)
    _check(m.dim() == 4 and tuple(m.shape[-2:]) == (T, T) and m.shape[0] in (1, B) and m.shape[1] in (1, H),
           f"attn_mask of shape {tuple(mask.shape)} does not broadcast onto [B={B}, H={H}, T={T}, T]")
    _check(T <= 256, "a general additive attn_mask is supported for T <= 256 (T <= 149 with E = 128)")
    if E is not None:
        _check_mask_limit(T, E)
    m = m.contiguous()
    return m, (0 if m.shape[0] == 1 else m.stride(0)), (0 if m.shape[1] == 1 else m.stride(1)), m.stride(2)


def _attn_desc(q, k, v, B, T, H, E, out, lse, table, causal, q_ts, kv_ts, kv_hs, mask=None, pack=None):
    from ._lib import STRUCTS
    _check(min(B, T, H, E) >= 1 and T <= 4096 and (T <= 256 or E in (32, 64, 128)),
           f"attention takes 1 <= T <= 4096 (E in 32/64/128 beyond T = 256; got B={B} T={T} H={H} E={E})")
    if mask is not None:  # forward and backward alike: never a forward whose backward cannot run
        _check_mask_limit(T, E)
    rows = pack.M if pack is not None else B * T  # packed rows: the maps index M rows
    _need(q, (rows - 1) * q_ts + (H - 1) * E + E, "q")
    _need(k, (rows - 1) * kv_ts + (H - 1) * kv_hs + E, "k")
    _need(v, (rows - 1) * kv_ts + (H - 1) * kv_hs + E, "v")
    _need(out, rows * H * E, "out")
    _need(lse, B * H * T, "lse")
    d = STRUCTS["lthm_attn_desc"]()
    if pack is not None:
        _check(attn_packed_ok(T, E, mask) and pack.B == B and pack.Tp == T, "packed attention: T > 256, E = 64, no mask")
        d.row_map, d.live_map = ptr(pack.pof), ptr(pack.pof_x)
    d.q, d.k, d.v = ptr(q), ptr(k), ptr(v)
    d.q_tok_stride, d.k_tok_stride, d.v_tok_stride = q_ts, kv_ts, kv_ts
    d.q_head_stride, d.k_head_stride, d.v_head_stride = E, kv_hs, kv_hs
    d.q_batch_stride, d.k_batch_stride, d.v_batch_stride = T * q_ts, T * kv_ts, T * kv_ts
    d.out, d.o_tok_stride, d.o_head_stride, d.o_batch_stride = ptr(out), H * E, E, T * H * E
    d.table = ptr(table)
    d.table_rows = table.shape[0] if table is not None else 0
    d.lse = ptr(lse)
    d.B, d.T, d.H, d.E, d.causal = B, T, H, E, int(causal)
    if mask is not None:  # (tensor, batch stride, head stride, row stride) from attn_mask_operand
        d.mask, d.mask_batch_stride, d.mask_head_stride, d.mask_row_stride = ptr(mask[0]), mask[1], mask[2], mask[3]
    return d


_PACKED_OK: dict = {}


def attn_packed_ok(T, E, mask=None):
    """The attention kernels read packed rows (a shared pad prefix's row maps) directly: the
    long-T' 32x32x16 kernels (T > 256, E = 64, no general mask, both LDS images fit, A/B
    switches off) -- the C dispatcher's own test (lthm_attn_packed_ok), so a shape it would
    refuse drops to the unpack path instead of raising."""
    if mask is not None:
        return False
    key = (int(T), int(E))
    ok = _PACKED_OK.get(key)
    if ok is None:
        from ._lib import load
        ok = _PACKED_OK[key] = bool(load().lthm_attn_packed_ok(key[0], key[1]))
    return ok


def attn_fwd_qkv(qkv, B, T, H, E, table=None, causal=True, mask=None, pack=None):
    """qkv bf16 [B*T, 3*H*E] (c_attn output) -> out bf16 [B*T, H*E], lse f32 [B, H, T].
    pack (recommendations_amd/pad_prefix.py, attn_packed_ok): qkv and out are the packed rows."""
    import ctypes
    C = H * E
    out = torch.empty((qkv.shape[0] if pack is not None else B * T, C), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=qkv.device)
    q = qkv
    k = qkv[:, C:]
    v = qkv[:, 2 * C:]
    d = _attn_desc(q, k, v, B, T, H, E, out, lse, table, causal, 3 * C, 3 * C, E, mask, pack=pack)
    # compulsory HBM bytes: q / k / v read, out written (bf16 rows), lse written
    call("lthm_attn_fwd", ctypes.addressof(d), stream(), _key="attn_fwd_k", _work=4.0 * B * H * T * T * E,
         _unit="flop", _bytes=float(4 * qkv.shape[0] * C * 2 + B * H * T * 4))
    return out, lse


def attn_fwd_mqa(q, kv, B, T, H, E, table=None, causal=True, mask=None):
    """Multi-query attention forward: q bf16 [B*T, H*E], kv bf16 [B*T, 2E] (one K/V head
    shared by all query heads: head stride 0) -> out bf16 [B*T, H*E], lse f32 [B, H, T]."""
    import ctypes
    require_gpu(q, kv)
    C = H * E
    _check(q.shape[-1] == C and kv.shape[-1] == 2 * E, "attn_fwd_mqa takes q [M, H*E] and kv [M, 2E]")
    out = torch.empty((B * T, C), dtype=torch.bfloat16, device=q.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    d = _attn_desc(q, kv, kv[:, E:], B, T, H, E, out, lse, table, causal, C, 2 * E, 0, mask)
    call("lthm_attn_fwd", ctypes.addressof(d), stream(), _key="attn_fwd_k", _work=4.0 * B * H * T * T * E,
         _unit="flop")
    return out, lse


def attn_bwd_qkv(qkv, out, dout, lse, B, T, H, E, table=None, causal=True, mask=None, pack=None):
    """-> dqkv bf16 [B*T, 3C], dtable f32 [2T+1, H] (or None).  pack: qkv / out / dout / dqkv
    are packed rows; the chain keys' dK / dV shares land in a [B, P+1, 2C] buffer whose
    per-sequence rows are then summed into the chain rows."""
    import ctypes
    C = H * E
    dqkv = torch.empty_like(qkv)
    from ._lib import load
    parts = int(load().lthm_attn_bwd_parts(B, T))
    part = torch.empty((parts, 2 * T + 1, H), dtype=torch.float32, device=qkv.device) if table is not None else None
    delta = torch.empty((B, H, T), dtype=torch.float32, device=qkv.device) if T > 256 else None
    d = _attn_desc(qkv, qkv[:, C:], qkv[:, 2 * C:], B, T, H, E, out, lse, table, causal, 3 * C, 3 * C, E, mask,
                   pack=pack)
    d.dout, d.dq, d.dk, d.dv = ptr(dout), ptr(dqkv), ptr(dqkv[:, C:]), ptr(dqkv[:, 2 * C:])
    chain = None
    if pack is not None:
        _check(dout.shape == out.shape and dout.is_contiguous(), "attn_bwd_qkv: packed dout")
        chain = torch.empty((B * (pack.P + 1), 2 * C), dtype=torch.bfloat16, device=qkv.device)
        d.dk_chain, d.dv_chain, d.chain_ts, d.chain_rows = ptr(chain), ptr(chain[:, C:]), 2 * C, pack.P + 1
    d.dtable_part, d.delta = ptr(part), ptr(delta)
    # compulsory HBM bytes: q / k / v, out and dout read, dq / dk / dv written (bf16 rows), lse read
    call("lthm_attn_bwd", ctypes.addressof(d), stream(), _key="attn_bwd_k", _work=10.0 * B * H * T * T * E,
         _unit="flop", _bytes=float(8 * qkv.shape[0] * C * 2 + B * H * T * 4))
    if chain is not None:
        pack.chain_sum(chain, 2 * C, pack.P + 1, dqkv[:, C:])
    dtab = None
    if part is not None:
        dtab = colsum(part.view(parts, (2 * T + 1) * H)).view(2 * T + 1, H)
    return dqkv, dtab


# ----------------------------------------------------------------- sparse KShift backward
# LTHM_KSHIFT_FIRST=0 keeps the all-atomic K = 1 table backward (A/B switch)
_KSHIFT_FIRST = os.environ.get("LTHM_KSHIFT_FIRST", "1") != "0"
# duplicate-list workspaces of the first-touch backward, one per (device, stream): word 0 is the
# kernel's duplicate counter, so two tables' backwards on different streams must not share one
_dup_ws = {}


def kshift_first_touch_ok(K, mode, D) -> bool:
    """The K = 1 table backward with first-touch stores and a touched-row bitmap
    (lthm_kshift_bwd_sparse_first) serves this table shape (LTHM_KSHIFT_FIRST=0: never)."""
    return _KSHIFT_FIRST and K == 1 and mode != KSHIFT_NORMALIZE and D <= 64 and 64 % D == 0


def kshift_bwd_sparse(ids, gy, out, norms, P, K, mode, F, dW, flags, rows_list, count, pending=0, flag_bits=False,
                      dy_ld=None):
    """Accumulate into dense dW and append the touched rows (see include/lthm.h).
    Table-batched layout: dW and flags cover all F*P rows; rows_list must hold
    every row that can still be appended (<= F*P, <= pending + ids*K).  flag_bits: flags is
    the touched-row bitmap of the first-touch K = 1 backward (int32 words, >= ceil(F*P / 32))."""
    # a row-strided gy (dy_ld) is not contiguous by design: its device is checked below
    require_gpu(ids, gy if dy_ld is None else None, out, norms, dW, flags, rows_list, count)
    D = dW.shape[1]
    if dy_ld is None:
        _check_kshift(ids, P, K, F, D, table_rows=dW.shape[0], gy=gy, out=out, norms=norms)
    else:
        # gy: a [B, F * D] view with row stride dy_ld inside a wider gradient row (the first-touch
        # K = 1 path reads it in place: lthm_kshift_bwd_sparse_first_ld)
        _check_kshift(ids, P, K, F, D, table_rows=dW.shape[0])
        _check(flag_bits and gy.is_cuda and gy.dim() == 2 and gy.shape == (ids.numel() // F, F * D) and gy.stride(1) == 1
               and gy.stride(0) == dy_ld and gy.data_ptr() % 16 == 0 and dy_ld % 4 == 0,
               "kshift_bwd_sparse(dy_ld): a [B, F*D] row-strided view, first-touch tables only")
    _check(dW.dtype == torch.float32, "dW must be float32")
    nflag = (F * P + 31) // 32 if flag_bits else F * P
    _check(flags.dtype == torch.int32 and flags.numel() >= nflag, f"flags must be int32 with >= {nflag} entries")
    _check(not flag_bits or kshift_first_touch_ok(K, mode, D), "a touched-row bitmap needs the K = 1 first-touch path")
    cap = min(F * P, pending + ids.numel() * K)
    _check(rows_list.dtype == torch.int64 and rows_list.numel() >= cap, f"rows_list must be int64 with >= {cap} entries")
    _check(count.dtype == torch.int64 and count.numel() >= 1, "count must be an int64 scalar buffer")
    n = ids.numel() // F
    if flag_bits:
        if not ids.numel():
            return
        # first-touch rows stored, repeats added afterwards (lthm_kshift_bwd_sparse_first)
        key = (ids.device, torch.cuda.current_stream(ids.device).cuda_stream)
        ws = _dup_ws.get(key)
        if ws is None or ws.numel() < ids.numel() + 1:
            ws = torch.empty(ids.numel() + 1, dtype=torch.int64, device=ids.device)
            _dup_ws[key] = ws
        if dy_ld is not None:
            call("lthm_kshift_bwd_sparse_first_ld", ptr(ids), n, F, ptr(gy), dcode(gy), dy_ld, P, D, ptr(dW),
                 ptr(flags), ptr(rows_list), ptr(count), ptr(ws), ws.numel(), stream())
            return
        call("lthm_kshift_bwd_sparse_first", ptr(ids), n, F, ptr(gy), dcode(gy), P, D, ptr(dW), ptr(flags),
             ptr(rows_list), ptr(count), ptr(ws), ws.numel(), stream())
        return
    call("lthm_kshift_bwd_sparse", ptr(ids), n, F, ptr(gy), dcode(gy),
         ptr(out) if out is not None else None, dcode(out) if out is not None else F32, ptr(norms),
         P, D, K, mode, ptr(dW), ptr(flags), ptr(rows_list), ptr(count), stream())


# fused dedup + Adagrad workspaces, one per (device, stream) (the kernel counters live in it)
_kag_ws = {}
_kag_need = {}


def kshift_adagrad_fused(ids, gy, out, norms, P, K, mode, F, W, state, clr, eps):
    """lthm_kshift_adagrad_fused: the KShift backward of ids [n, F] / gy [n, F, D] and the
    Adagrad step of the rows it touches in one call (W, state [F * P, D] f32, updated in place;
    clr = lr / (1 + (step - 1) lr_decay))."""
    require_gpu(ids, gy, out, norms, W, state)
    D = W.shape[1]
    _check_kshift(ids, P, K, F, D, table_rows=W.shape[0], gy=gy, out=out, norms=norms)
    _check(W.dtype == torch.float32 and state.dtype == torch.float32 and state.shape == W.shape,
           "kshift_adagrad_fused: W and state are [F * P, D] float32")
    _check(W.is_contiguous() and state.is_contiguous(), "kshift_adagrad_fused: W and state contiguous")
    _check(mode != KSHIFT_NORMALIZE or (out is not None and norms is not None), "normalize mode needs out / norms")
    n = ids.numel() // F
    if n == 0:
        return
    need = _kag_need.get((n * F, K, D))
    if need is None:  # (the size query asks the sort for its temporary storage: once per shape)
        need = _kag_need[(n * F, K, D)] = load().lthm_kshift_adagrad_ws_bytes(n * F, K, D)
    _check(need > 0, f"kshift_adagrad_fused: unsupported sizes (n * F * K = {n * F * K}, D = {D}, K = {K})")
    key = (ids.device, torch.cuda.current_stream(ids.device).cuda_stream)
    ws = _kag_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=ids.device)
        _kag_ws[key] = ws
    call("lthm_kshift_adagrad_fused", ptr(ids), n, F, ptr(gy), dcode(gy),
         ptr(out) if out is not None else None, dcode(out) if out is not None else F32, ptr(norms), P, D, K, mode,
         ptr(W), ptr(state), clr, eps, ptr(ws), ws.numel(), stream(), _key="lthm_kshift_adagrad_fused")


# ----------------------------------------------------------------- optimizers / norms
def adamw_(p, g, m, v, lr, betas, eps, wd, step, grad_scale=1.0, shadow=None, zero_grad=False):
    for t, nm in ((g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq"), (shadow, "shadow")):
        _need(t, p.numel(), nm)
    call("lthm_adamw", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps, wd, step,
         grad_scale, ptr(shadow), int(zero_grad), stream())


def adamw_multi_(ps, gs, ms, vs, lr, betas, eps, wd, step, grad_scale=1.0):
    """lthm_adamw_multi: one launch per 48 fp32 tensors with identical hyper-parameters and step."""
    import ctypes
    n = len(ps)
    for p, g, m, v in zip(ps, gs, ms, vs):
        require_gpu(p)
        for t, nm in ((g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
            _need(t, p.numel(), nm)
        _check(all(t.dtype == torch.float32 and t.is_contiguous() for t in (p, g, m, v)),
               "adamw_multi_ takes contiguous fp32 tensors")
    plan = adamw_multi_plan(ps, gs, ms, vs)
    adamw_multi_run(plan, lr, betas, eps, wd, step, grad_scale)


def adamw_multi_plan(ps, gs, ms, vs):
    """The pointer / count arrays of one lthm_adamw_multi call (checked by the caller),
    kept by FusedAdamW across steps while the tensors stay where they are."""
    import ctypes
    n = len(ps)
    arr = lambda ts: (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in ts])  # noqa: E731
    arrs = (arr(ps), arr(gs), arr(ms), arr(vs), (ctypes.c_int64 * max(n, 1))(*[p.numel() for p in ps]))
    # the moment buffers are held (their addresses are baked in); parameters and gradients
    # are not (holding last step's gradients would move the next step's), so a user of a
    # kept plan must check their addresses first, as FusedAdamW.step does
    return n, (arrs, list(ms), list(vs)), tuple(ctypes.cast(a, ctypes.c_void_p) for a in arrs), \
        28.0 * sum(p.numel() for p in ps)


def adamw_multi_run(plan, lr, betas, eps, wd, step, grad_scale=1.0):
    n, _, (pp, pg, pm, pv, pc), work = plan
    call("lthm_adamw_multi", n, pp, pg, pm, pv, pc, lr, betas[0], betas[1], eps, wd, step, grad_scale, stream(),
         _key="lthm_adamw", _work=work, _unit="byte")


def adagrad_(p, g, s, lr, lr_decay, eps, wd, step, zero_grad=False):
    _need(g, p.numel(), "grad")
    _need(s, p.numel(), "state_sum")
    call("lthm_adagrad", ptr(p), ptr(g), ptr(s), p.numel(), lr, lr_decay, eps, wd, step, int(zero_grad), stream())


def _check_sparse_rows(rows, max_rows, p, flags, *states):
    _check(p.dim() == 2 and max_rows <= p.shape[0], "sparse update: p must be [R, D] and max_rows <= R")
    _need(rows, max_rows, "rows")
    _need(flags, p.shape[0], "flags")  # (flags None: the caller clears its touched-row bitmap itself)
    for t in states:
        _need(t, p.numel(), "state")


def _touched_work(count, max_rows, per_row):
    """Algorithmic bytes of a row-wise update for the live kernel timer: the touched-row
    count is on the device, so it is snapshotted (one 8-byte copy, timed runs only) and
    read after the timed region."""
    from . import _lib
    if _lib.TIMER is None:
        return None
    snap = count.clone()
    return lambda: float(min(int(snap.item()), max_rows)) * per_row


def sparse_adamw_(rows, count, max_rows, p, g, m, v, flags, lr, betas, eps, wd, step, shadow=None, keep_grad=False):
    """Row-wise AdamW over the touched rows (lthm_sparse_adamw_ex).  keep_grad: the gradient rows
    are not re-zeroed (first-touch tables: the next backward overwrites them)."""
    _check_sparse_rows(rows, max_rows, p, flags, g, m, v, shadow)
    D = p.shape[1]
    # per touched row: its index, p / g / m / v read, p / m / v written, g zeroed (unless kept), the
    # touched flag, the bf16 shadow row
    per_row = 8 + 4 + (7 if keep_grad else 8) * 4 * D + (2 * D if shadow is not None else 0)
    call("lthm_sparse_adamw_ex", ptr(rows), ptr(count), max_rows, D, ptr(p), ptr(g), ptr(m), ptr(v),
         ptr(flags), lr, betas[0], betas[1], eps, wd, step, ptr(shadow), int(keep_grad), stream(),
         _key="lthm_sparse_adamw", _work=_touched_work(count, max_rows, per_row), _unit="byte")


def sparse_adagrad_(rows, count, max_rows, p, g, s, flags, lr, lr_decay, eps, step, shadow=None, keep_grad=False):
    _check_sparse_rows(rows, max_rows, p, flags, g, s, shadow)
    D = p.shape[1]
    # p / g / s read, p / s written, g zeroed (unless kept)
    per_row = 8 + 4 + (5 if keep_grad else 6) * 4 * D + (2 * D if shadow is not None else 0)
    call("lthm_sparse_adagrad_ex", ptr(rows), ptr(count), max_rows, D, ptr(p), ptr(g), ptr(s), ptr(flags),
         lr, lr_decay, eps, step, ptr(shadow), int(keep_grad), stream(), _key="lthm_sparse_adagrad",
         _work=_touched_work(count, max_rows, per_row), _unit="byte")


def sumsq(x, acc):
    call("lthm_sumsq", ptr(x), dcode(x), x.numel(), ptr(acc), stream())


def scale_by_norm(x, y, ss, add_eps=1e-6, max_norm=0.0):
    call("lthm_scale_by_norm", ptr(x), ptr(y), dcode(x), x.numel(), ptr(ss), add_eps, max_norm, stream())


class CapGradientsFn(torch.autograd.Function):
    """commons/functional.py:4-25: identity forward, g / (||g||_2 + 1e-6) backward."""

    @staticmethod
    def forward(ctx, x):
        require_gpu(x)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        ss = torch.zeros(1, dtype=torch.float32, device=g.device)
        sumsq(g, ss)
        out = torch.empty_like(g)
        scale_by_norm(g, out, ss, add_eps=1e-6)
        return out


# ----------------------------------------------------------------- towers
def flip_tokens(x):
    require_gpu(x)
    out = torch.empty_like(x)
    B, T = x.shape
    call("lthm_flip_tokens", ptr(x), ptr(out), B, T, stream())
    return out


def _table_ws(dev, n, R, D):
    """Partial-sum workspace for lthm_*_table_bwd: up to 32 token chunks of [R, D] f32."""
    nz = max(1, min(32, (n + 511) // 512))
    if nz < 2:
        return None, 0
    ws = _workspace(dev, nz * R * D * 4)
    return ws, ws.numel() * 4


def small_table_bwd(rows, dY, R, out=None):
    """rows uint16 stored as int16 [n, nidx]; dY [n, D] -> f32 [R, D] (accumulated into out)."""
    require_gpu(rows, dY, out)
    n, nidx = rows.shape
    D = dY.shape[-1]
    _check(rows.dtype == torch.int16 and dY.numel() == n * D, "rows must be int16 [n, nidx] and dY [n, D]")
    _check(0 < nidx <= 64 and 0 < R < 0xFFFF, f"small_table_bwd takes nidx <= 64 slots and R < 65535 rows")
    mfma = D in (16, 32, 64, 128, 256) and nidx <= 8 and R <= 8192
    wide = D > 256 and D % 256 == 0 and nidx <= 8 and R <= 8192
    _check(mfma or wide or R * 64 * 4 <= 160 * 1024, f"R={R} rows exceed the LDS slice; use segmented_table_bwd")
    if out is None:
        out = torch.zeros((R, D), dtype=torch.float32, device=dY.device)
    _check(out.dtype == torch.float32 and tuple(out.shape) == (R, D), "out must be float32 [R, D]")
    if wide:
        # d_model > 256 (C5: 512): the one-hot MFMA reduction over 256-column slices of dY
        dYc = dY.contiguous()
        for c0 in range(0, D, 256):
            part = zeros((R, 256), torch.float32, dY.device)
            ws, wsb = _table_ws(dY.device, n, R, 256)
            call("lthm_table_bwd_mfma", ptr(rows), nidx, R, dYc.data_ptr() + c0 * dYc.element_size(), dcode(dYc), D,
                 n, 256, ptr(part), ptr(ws) if ws is not None else None, wsb, stream(), _key="table_bwd_mfma_k",
                 _work=2.0 * n * 256 * R * (2 if dY.dtype == torch.float32 else 1), _unit="flop")
            out[:, c0:c0 + 256] += part
        return out
    ws, wsb = _table_ws(dY.device, n, R, D)
    if mfma:
        # one-hot MFMA reduction (f32 dY split into bf16 hi + lo): no LDS atomics
        call("lthm_table_bwd_mfma", ptr(rows), nidx, R, ptr(dY), dcode(dY), D, n, D, ptr(out),
             ptr(ws) if ws is not None else None, wsb, stream(), _key="table_bwd_mfma_k",
             _work=2.0 * n * D * R * (2 if dY.dtype == torch.float32 else 1), _unit="flop")
        return out
    call("lthm_small_table_bwd", ptr(rows), nidx, ptr(dY), dcode(dY), D, n, R, D, ptr(out),
         ptr(ws) if ws is not None else None, wsb, stream(), _key="small_tab_bwd_k",
         _work=float(n) * D * dY.element_size(), _unit="byte")
    return out


def rownorm(x2d, row_mask=None):
    """F.normalize rows -> (bf16 rows, f32 norms).  ``row_mask`` (uint8 [G, >= rows / G],
    any row stride): rows r with row_mask[r // G, r % G] set get a zero output row."""
    rows, D = x2d.shape
    out = torch.empty((rows, D), dtype=torch.bfloat16, device=x2d.device)
    norms = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    mg = ms = 0
    if row_mask is not None:
        _check(row_mask.dtype == torch.uint8 and row_mask.dim() == 2 and row_mask.stride(1) == 1,
               "row_mask must be uint8 [G, n] with unit column stride")
        mg, ms = row_mask.shape[1], row_mask.stride(0)
        _check(mg > 0 and rows % mg == 0 and rows // mg <= row_mask.shape[0], "row_mask shape does not cover the rows")
    call("lthm_rownorm", ptr(x2d), dcode(x2d), rows, D, ptr(out), ptr(norms), ptr(row_mask), mg, ms, stream())
    return out, norms


def rownorm_bwd(x2d, norms, g, want_f32=False):
    rows, D = x2d.shape
    dxb = torch.empty((rows, D), dtype=torch.bfloat16, device=x2d.device)
    dxf = torch.empty((rows, D), dtype=torch.float32, device=x2d.device) if want_f32 else None
    call("lthm_rownorm_bwd", ptr(x2d), dcode(x2d), ptr(norms), ptr(g), rows, D, ptr(dxb), ptr(dxf), stream())
    return dxb, dxf


# ----------------------------------------------------------------- MLP chains
class MLPChainFn(torch.autograd.Function):
    """x -> Linear -> act -> Linear -> act ... -> Linear (acts[i] after layer i; last is ACT_NONE).

    Every Linear is one MFMA GEMM with the bias and activation fused in its
    epilogue; the backward fuses act' into the preceding dgrad GEMM.  Serves
    commons/layers.py:65-81 (QuickGELU gates) and commons/transformers/layers.py:67-81.
    """

    @staticmethod
    def forward(ctx, x, x2, acts, out_f32, *wb):
        """x2 (optional, [.., K2]): concatenated after x's features as the first GEMM's operand
        (the ranker's [dense | categorical] input, built once in bf16, the GEMM operand dtype,
        instead of as an f32 concatenation the GEMM would cast again).  x2 may also be a
        ``RowsInput`` (round 6): row-wise trained K = 1 tables whose lookups are gathered straight
        into the operand's columns after x's, and whose gradient the backward hands to their
        sparse backward in place (no concatenation, no strided-slice copy)."""
        require_gpu(x)
        shp = x.shape
        h = x.contiguous().view(-1, shp[-1])
        ctx.k1, ctx.rows = None, None
        if isinstance(x2, RowsInput):
            B, E = h.shape
            F_, D = x2.mod._F, x2.gather_w.shape[1]
            buf = torch.empty((B, E + F_ * D), dtype=torch.bfloat16, device=x.device)
            buf[:, :E].copy_(h)  # round to nearest even, as the operand cast below
            x2.gather_into(buf, E)
            ctx.k1, ctx.rows = E, x2
            h = buf
            shp = tuple(shp[:-1]) + (h.shape[1],)
        h = h if h.dtype == torch.bfloat16 else cast(h, torch.bfloat16)
        if x2 is not None and ctx.rows is None:
            ctx.k1 = h.shape[1]
            h = torch.cat([h, x2.reshape(h.shape[0], -1).to(torch.bfloat16)], dim=1)
            shp = tuple(shp[:-1]) + (h.shape[1],)
        n = len(wb) // 2
        ws = [cast(wb[2 * i].detach().contiguous(), torch.bfloat16) for i in range(n)]
        hs, pres = [h], []
        for i in range(n):
            last = i == n - 1
            b = wb[2 * i + 1]
            pre = None
            if acts[i] != ACT_NONE:
                pre = torch.empty((h.shape[0], ws[i].shape[0]), dtype=torch.bfloat16, device=x.device)
            h = linear_fwd(h, ws[i], bias=None if b is None else b.detach().contiguous(), act=acts[i], aux_out=pre,
                           out_dtype=torch.float32 if (last and out_f32) else torch.bfloat16)
            pres.append(pre)
            if not last:
                hs.append(h)
        ctx.save_for_backward(*hs, *[p for p in pres if p is not None], *ws)
        ctx.meta = (n, acts, [p is not None for p in pres], [wb[2 * i + 1] is not None for i in range(n)], shp,
                    x.dtype)
        return h.view(*shp[:-1], h.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        n, acts, has_pre, has_b, shp, xdt = ctx.meta
        saved = ctx.saved_tensors
        hs = saved[:n]
        npre = sum(has_pre)
        pre_list = list(saved[n:n + npre])
        ws = saved[n + npre:]
        pres = []
        it = iter(pre_list)
        for hp in has_pre:
            pres.append(next(it) if hp else None)
        g = dy.contiguous().view(-1, dy.shape[-1])
        gb = g if g.dtype == torch.bfloat16 else cast(g, torch.bfloat16)
        grads = [None] * (2 * n)
        dx = None
        for i in range(n - 1, -1, -1):
            grads[2 * i] = linear_wgrad(gb, hs[i])
            if has_b[i]:
                grads[2 * i + 1] = colsum(gb)
            if i > 0:
                ag = {ACT_GELU: ACT_GELU_GRAD, ACT_QGELU: ACT_QGELU_GRAD}.get(acts[i - 1], ACT_NONE)
                gb = linear_dgrad(gb, ws[i], act_grad=ag, aux=pres[i - 1])
            else:
                dx = linear_dgrad(gb, ws[0], out_dtype=torch.float32 if xdt == torch.float32 else torch.bfloat16)
        if ctx.rows is not None:  # the tables' columns of dx go to their sparse backward in place
            k1 = ctx.k1
            ctx.rows.backward_from(dx, k1)
            ctx.rows = None
            return (dx[:, :k1].reshape(*shp[:-1], k1), None, None, None, *grads)
        if ctx.k1 is not None:  # the two inputs' parts of dx (x2's cast to its dtype by autograd)
            k1 = ctx.k1
            return (dx[:, :k1].reshape(*shp[:-1], k1), dx[:, k1:], None, None, *grads)
        return (dx.view(*shp[:-1], dx.shape[-1]), None, None, None, *grads)


class RowsInput:
    """Row-wise trained K = 1 tables (``mod``: TableBatchedKShiftEmbedding with ``into_row_ok``)
    looked up by ``ids`` [B, F] as the second part of MLPChainFn's operand (see there)."""

    def __init__(self, ids, mod, gather_w):
        self.ids, self.mod, self.gather_w = ids, mod, gather_w

    def gather_into(self, buf, col0):
        from .commons.layers import _kshift_fwd_into
        _kshift_fwd_into(self.mod, self.ids, self.gather_w, buf, col0)

    def backward_from(self, dx, col0):
        from .commons.layers import _kshift_bwd_rows
        _kshift_bwd_rows(self.mod, self.ids, dx, col0)


def mlp_chain(x, linears, acts, out_f32=True, x2=None):
    wb = []
    for lin in linears:
        wb += [lin.weight, lin.bias]
    return MLPChainFn.apply(x, x2, tuple(acts), out_f32, *wb)


class ActivationFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        require_gpu(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        call("lthm_activation", ptr(x), None, ptr(y), dcode(x), x.numel(), act, stream())
        ctx.save_for_backward(x)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous().to(x.dtype)
        dx = torch.empty_like(x)
        call("lthm_activation", ptr(x), ptr(dy), ptr(dx), dcode(x), x.numel(), ctx.act, stream())
        return dx, None


def zeros(shape, dtype, device):
    """Zero-filled tensor (f32 through the HIP fill kernel; other dtypes via memset)."""
    t = torch.empty(shape, dtype=dtype, device=device)
    if dtype == torch.float32:
        call("lthm_fill_f32", ptr(t), 0.0, t.numel(), stream())
    else:
        t.zero_()
    return t


def quantile_map(x, quantiles, shared):
    """QuantileMapper (commons/transformers/layers.py:484-487) on x [B, F]:
    bucketize(x[:, f], q_f) / (nq + 1) - 0.5; quantiles [1 or F, nq]."""
    require_gpu(x, quantiles)
    B, Fd = x.shape if x.dim() == 2 else (x.numel(), 1)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("lthm_quantile_map", ptr(x), B, Fd, ptr(quantiles), quantiles.shape[-1], int(shared), ptr(out), stream())
    return out


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def simhash(x2d, proj):
    """SimhashVectorIndexer (commons/transformers/layers.py:431-437): int64 [rows] of the
    sign bits of x2d [rows, dim] @ proj [dim, P] (f32 dot products, P <= 64)."""
    require_gpu(x2d, proj)
    rows, dim = x2d.shape
    P = proj.shape[1]
    _check(proj.shape[0] == dim and 0 < P <= 64, f"simhash takes proj [{dim}, P <= 64], got {tuple(proj.shape)}")
    x2d, proj = _aligned16(x2d.contiguous().float()), proj.contiguous().float()
    out = torch.empty(rows, dtype=torch.int64, device=x2d.device)
    call("lthm_rowproj_fwd", ptr(x2d), rows, dim, ptr(proj), 1, P, P, 0, ptr(out), stream(),
         _key="rowproj_fwd_k", _work=4.0 * rows * dim + 8.0 * rows, _unit="B")
    return out


def l2norm_rows(x2d):
    """F.normalize(x, dim=-1) over f32 rows (lthm_l2norm_rows)."""
    rows, dim = x2d.shape
    y = torch.empty_like(x2d)
    call("lthm_l2norm_rows", ptr(x2d), rows, dim, ptr(y), stream())
    return y


def l2norm_rows_bwd(x2d, g=None, dz=None, w_hat=None, rinv=None):
    rows, dim = x2d.shape
    dx = torch.empty_like(x2d)
    call("lthm_l2norm_rows_bwd", ptr(x2d), rows, dim, ptr(g), ptr(dz), ptr(w_hat),
         0 if w_hat is None else w_hat.shape[0], ptr(dx), ptr(rinv), stream())
    return dx


class CosineLinearFn(torch.autograd.Function):
    """CosineLinear (commons/transformers/layers.py:517-525): normalize(x) @ normalize(W)^T
    in f32.  fwd: lthm_l2norm_rows(W) + lthm_rowproj_fwd(mode 1).  bwd: lthm_l2norm_rows_bwd
    (x side, dz @ W_hat fused), lthm_cosine_wgrad + lthm_l2norm_rows_bwd (W side)."""

    @staticmethod
    def forward(ctx, x, w):
        require_gpu(x, w)
        shp = x.shape
        x2 = _aligned16(x.detach().contiguous().view(-1, shp[-1]).float())
        wf = w.detach().contiguous().float()
        P, dim = wf.shape
        _check(dim == x2.shape[1], f"CosineLinear: x dim {x2.shape[1]} != weight dim {dim}")
        w_hat = l2norm_rows(wf)
        out = torch.empty((x2.shape[0], P), dtype=torch.float32, device=x.device)
        call("lthm_rowproj_fwd", ptr(x2), x2.shape[0], dim, ptr(w_hat), dim, 1, P, 1, ptr(out), stream(),
             _key="rowproj_fwd_k", _work=4.0 * x2.shape[0] * (dim + P), _unit="B")
        ctx.save_for_backward(x2, wf, w_hat)
        ctx.shp, ctx.dts = shp, (x.dtype, w.dtype)
        return out.view(*shp[:-1], P)

    @staticmethod
    def backward(ctx, dy):
        x2, wf, w_hat = ctx.saved_tensors
        P, dim = wf.shape
        dz = dy.contiguous().view(-1, P).float()
        rows = x2.shape[0]
        rinv = torch.empty(rows, dtype=torch.float32, device=x2.device)
        dx = l2norm_rows_bwd(x2, dz=dz, w_hat=w_hat, rinv=rinv)
        dwh = zeros((P, dim), torch.float32, x2.device)
        call("lthm_cosine_wgrad", ptr(dz), ptr(x2), ptr(rinv), rows, P, dim, ptr(dwh), stream())
        dw = l2norm_rows_bwd(wf, g=dwh)
        return dx.view(ctx.shp).to(ctx.dts[0]), dw.to(ctx.dts[1])


class GaussBinsFn(torch.autograd.Function):
    """The gaussian_kernel of LearnableCosineVectorEmbedding / ProbabilityVectorEmbedding
    (commons/transformers/layers.py:558-569, 588-595): z [..., P] f32, mean [P, nb]
    -> [..., P * nb] (bf16 when it feeds the bf16 GEMM, else f32)."""

    @staticmethod
    def forward(ctx, z, mean, sigma2, top_k, out_dtype):
        require_gpu(z, mean)
        zf = z.detach().contiguous().float()
        P = zf.shape[-1]
        mf = mean.detach().contiguous().float().view(P, -1)
        nb = mf.shape[1]
        _check(0 < nb <= 64, f"gaussian bins take 1..64 bins, got {nb}")
        out = torch.empty((*zf.shape[:-1], P * nb), dtype=out_dtype, device=z.device)
        n = zf.numel()
        call("lthm_gauss_bins_fwd", ptr(zf), n, P, ptr(mf), nb, float(sigma2), int(top_k), ptr(out), dcode(out),
             stream(), _key="gauss_bins_fwd_k", _work=4.0 * n + out.element_size() * n * nb, _unit="B")
        ctx.save_for_backward(zf, mf)
        ctx.meta = (float(sigma2), int(top_k), mean.shape, z.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        zf, mf = ctx.saved_tensors
        sigma2, top_k, mshape, zdt = ctx.meta
        P, nb = mf.shape
        g = g.contiguous()
        if g.dtype not in (torch.float32, torch.bfloat16):
            g = g.float()
        dz = torch.empty_like(zf) if ctx.needs_input_grad[0] else None
        dmean = zeros((P, nb), torch.float32, zf.device)
        call("lthm_gauss_bins_bwd", ptr(zf), zf.numel(), P, ptr(mf), nb, sigma2, top_k, ptr(g), dcode(g), ptr(dz),
             ptr(dmean), stream(), _key="gauss_bins_bwd_k")
        return (None if dz is None else dz.to(zdt)), dmean.view(mshape), None, None, None


def cve_table_bwd(rows, dY, R, modules, out=None):
    """MFMA one-hot gradient of CVE-structured tables (include/lthm.h lthm_cve_table_bwd).
    modules: [(slot0, nslot, row0, rows_per_slot)]; dY bf16 or f32 [n, D], D in {16..256} pow2."""
    import numpy as _np
    require_gpu(rows, dY, out)
    n, nidx = rows.shape
    D = dY.shape[-1]
    _check(rows.dtype == torch.int16 and dY.dtype in (torch.bfloat16, torch.float32) and dY.numel() == n * D,
           "rows must be int16 [n, nidx] and dY bf16 / f32 [n, D]")
    _check(D in (16, 32, 64, 128, 256) or D % 256 == 0,
           f"cve_table_bwd takes D in 16..256 (power of two) or a multiple of 256, got {D}")
    _check(0 < len(modules) <= 16, "1..16 modules")
    for s0, ns, r0, rps in modules:
        _check(0 <= s0 and ns > 0 and s0 + ns <= nidx, f"module slots ({s0}, {ns}) outside [0, {nidx})")
        _check(0 <= r0 and rps > 0 and r0 + ns * rps <= R, f"module rows ({r0}, {ns}x{rps}) outside [0, {R})")
    if out is None:
        out = zeros((R, D), torch.float32, dY.device)
    _check(out.dtype == torch.float32 and tuple(out.shape) == (R, D), "out must be float32 [R, D]")
    m = _np.ascontiguousarray(_np.array(modules, dtype=_np.int32).T)
    if D > 256:
        # d_model > 256 (C5: 512): the one-hot MFMA reduction over 256-column slices of dY
        dYc = dY.contiguous()
        ws, wsb = _table_ws(dY.device, n, R, 256)
        for c0 in range(0, D, 256):
            part = zeros((R, 256), torch.float32, dY.device)
            call("lthm_cve_table_bwd", ptr(rows), nidx, m.shape[1], m[0].ctypes.data, m[1].ctypes.data,
                 m[2].ctypes.data, m[3].ctypes.data, dYc.data_ptr() + c0 * dYc.element_size(), dcode(dYc), D, n, 256,
                 ptr(part), ptr(ws) if ws is not None else None, wsb, stream(), _key="cve_tab_bwd_k",
                 _work=2.0 * n * 256 * sum(ns * rps for _, ns, _, rps in modules), _unit="flop")
            out[:, c0:c0 + 256] += part
        return out
    ws, wsb = _table_ws(dY.device, n, R, D)
    call("lthm_cve_table_bwd", ptr(rows), nidx, m.shape[1], m[0].ctypes.data, m[1].ctypes.data, m[2].ctypes.data,
         m[3].ctypes.data, ptr(dY), dcode(dY), D, n, D, ptr(out), ptr(ws) if ws is not None else None, wsb, stream(),
         _key="cve_tab_bwd_k", _work=2.0 * n * D * sum(ns * rps for _, ns, _, rps in modules), _unit="flop")
    return out


def cve_segments(n_proj: int, rows_per_slot: int, slot0: int = 0, row0: int = 0, max_rows: int = 256):
    """Backward segments of one CosineVectorEmbedding module: projection p owns rows
    [row0 + p*rows_per_slot, +rows_per_slot); runs of projections of <= max_rows
    rows keep each block's LDS slice <= 64 KiB (two blocks per CU)."""
    per = max(1, min(64, max_rows // rows_per_slot))
    return [(slot0 + p0, min(per, n_proj - p0), row0 + p0 * rows_per_slot, min(per, n_proj - p0) * rows_per_slot)
            for p0 in range(0, n_proj, per)]


def segmented_table_bwd(rows, dY, R, segments, out=None):
    """Like small_table_bwd, with slots grouped into (slot0, nslot, row0, nrow) segments."""
    import numpy as _np
    require_gpu(rows, dY, out)
    n, nidx = rows.shape
    D = dY.shape[-1]
    _check(rows.dtype == torch.int16 and dY.numel() == n * D, "rows must be int16 [n, nidx] and dY [n, D]")
    for s0, ns, r0, nr in segments:
        _check(0 <= s0 and 0 < ns <= 64 and s0 + ns <= nidx, f"segment slots ({s0}, {ns}) outside [0, {nidx})")
        _check(0 <= r0 and 0 < nr <= 640 and r0 + nr <= R, f"segment rows ({r0}, {nr}) outside [0, {R}) or > 640")
    if out is None:
        out = zeros((R, D), torch.float32, dY.device)
    _check(out.dtype == torch.float32 and tuple(out.shape) == (R, D), "out must be float32 [R, D]")
    ws, wsb = _table_ws(dY.device, n, R, D)
    for g in range(0, len(segments), 64):  # the kernel takes <= 64 segments per launch
        seg = _np.ascontiguousarray(_np.array(segments[g:g + 64], dtype=_np.int32).T)
        call("lthm_segmented_table_bwd", ptr(rows), nidx, seg.shape[1], seg[0].ctypes.data, seg[1].ctypes.data,
             seg[2].ctypes.data, seg[3].ctypes.data, ptr(dY), dcode(dY), D, n, D, ptr(out),
             ptr(ws) if ws is not None else None, wsb, stream(),
             _key="seg_tab_bwd_k", _unit="byte",
             # dY and the uint16 bucket rows read once, the [R, D] f32 gradient read and written
             _work=float(n) * (D * dY.element_size() + 2 * nidx) + 8.0 * R * D)
    return out


# ----------------------------------------------------------------- BCE with logits
class BCEWithLogitsFn(torch.autograd.Function):
    """F.binary_cross_entropy_with_logits(z, y), mean over all elements, on the
    lthm_bce_logits_* kernels (the ranker's click loss)."""

    @staticmethod
    def forward(ctx, z, y):
        require_gpu(z, y)
        _check(z.dtype == torch.float32 and y.dtype == torch.float32 and z.numel() == y.numel(),
               "bce_with_logits takes float32 logits and targets of the same size")
        z, y = z.contiguous(), y.contiguous()
        n = z.numel()
        out = zeros((1,), torch.float32, z.device)
        call("lthm_bce_logits_fwd", ptr(z), ptr(y), n, 1.0 / max(n, 1), ptr(out), stream(), _key="bce_fwd_k",
             _work=8.0 * n, _unit="byte")
        ctx.save_for_backward(z, y)
        return out.view(())

    @staticmethod
    def backward(ctx, g):
        z, y = ctx.saved_tensors
        dz = torch.empty_like(z)
        g = g.contiguous().float()
        call("lthm_bce_logits_bwd", ptr(z), ptr(y), z.numel(), ptr(g), 1.0 / max(z.numel(), 1), ptr(dz), stream(),
             _key="bce_bwd_k", _work=12.0 * z.numel(), _unit="byte")
        return dz, None


def bce_with_logits(z, y):
    return BCEWithLogitsFn.apply(z, y)


class MSELossFn(torch.autograd.Function):
    """nn.MSELoss() (mean) of y (f32 / bf16) against an f32 target, on lthm_mse_*."""

    @staticmethod
    def forward(ctx, y, x):
        require_gpu(y, x)
        _check(y.numel() == x.numel() and y.dtype in (torch.float32, torch.bfloat16) and x.dtype == torch.float32,
               "mse takes f32 / bf16 predictions and an f32 target of the same size")
        y, x = y.contiguous(), x.contiguous()
        n = y.numel()
        out = zeros((1,), torch.float32, y.device)
        call("lthm_mse_fwd", ptr(y), dcode(y), ptr(x), n, 1.0 / max(n, 1), ptr(out), stream())
        ctx.save_for_backward(y, x)
        return out.view(())

    @staticmethod
    def backward(ctx, g):
        y, x = ctx.saved_tensors
        dy = torch.empty_like(y)
        g = g.contiguous().float()
        call("lthm_mse_bwd", ptr(y), dcode(y), ptr(x), y.numel(), ptr(g), 1.0 / max(y.numel(), 1), ptr(dy), stream())
        return dy, None


def mse_loss(y, x):
    return MSELossFn.apply(y, x)


# ----------------------------------------------------------------- full-catalogue retrieval
RETRIEVE_WIDTH = 128          # csrc/retrieve.hip RT_D (= the loss kernels' LOSS_DE)
RETRIEVE_MAX_K = 128          # RT_KMAX
RETRIEVE_MIN_SLAB_ROWS = 64   # RT_IT: the smallest (and the granularity of) slab_rows
RETRIEVE_MAX_EXCLUDE = 1024   # RT_XMAX: the longest exclusion list of a query


def _retrieve_tags(who: str, tags, tag_filter, items, n_filters: int, per: str):
    """The lthm_retrieve_tags of a call, or None without tags: tags int32 [N] and tag_filter
    int32 [n_filters, 3], contiguous, on the catalogue's device, both or neither."""
    from ._lib import STRUCTS
    _check((tags is None) == (tag_filter is None), f"{who} takes tags and tag_filter together or neither")
    if tags is None:
        return None
    N = items.shape[0]
    _check(tags.dtype == torch.int32 and tags.dim() == 1 and tags.shape[0] == N,
           f"tags must be int32 [N], one word per catalogue row (got {tags.dtype} {tuple(tags.shape)}, N={N})")
    _check(tag_filter.dtype == torch.int32 and tag_filter.dim() == 2 and tuple(tag_filter.shape) == (n_filters, 3),
           f"tag_filter must be int32 [{per}, 3] = (all, any, none), one row per {'user' if per == 'U' else 'query'} "
           f"(got {tag_filter.dtype} {tuple(tag_filter.shape)}, {per}={n_filters})")
    _check(tags.is_contiguous() and tag_filter.is_contiguous(), "tags and tag_filter must be contiguous")
    _check(tags.device == items.device and tag_filter.device == items.device,
           "tags and tag_filter must be on the catalogue's device")
    t = STRUCTS["lthm_retrieve_tags"]()
    t.tags, t.filter = ptr(tags), ptr(tag_filter)
    return t


RETRIEVE_MAX_DEEP = 1024      # the longest list of a deep call (RD_KMAX): one scan, or 8 pages of RETRIEVE_MAX_K


def _retrieve_cursor(who: str, after_scores, after_rows, n: int, per: str, device):
    """The lthm_retrieve_cursor of a call, or None without a cursor: after_scores f32 [n] and
    after_rows int32 [n], contiguous, on the queries' device, both or neither."""
    from ._lib import STRUCTS
    _check((after_scores is None) == (after_rows is None), f"{who} takes after_scores and after_rows together or neither")
    if after_scores is None:
        return None
    _check(after_scores.dtype == torch.float32 and tuple(after_scores.shape) == (n,),
           f"after_scores must be f32 [{per}] (got {after_scores.dtype} {tuple(after_scores.shape)}, {per}={n})")
    _check(after_rows.dtype == torch.int32 and tuple(after_rows.shape) == (n,),
           f"after_rows must be int32 [{per}] (got {after_rows.dtype} {tuple(after_rows.shape)}, {per}={n})")
    _check(after_scores.is_contiguous() and after_rows.is_contiguous(), "after_scores and after_rows must be contiguous")
    _check(after_scores.device == device and after_rows.device == device,
           "after_scores and after_rows must be on the queries' device")
    c = STRUCTS["lthm_retrieve_cursor"]()
    c.after_score, c.after_row = ptr(after_scores), ptr(after_rows)
    return c


def _retrieve_bias(who: str, bias, bias_weight, items, n: int, per: str, device):
    """(the lthm_retrieve_bias of a call, the weight tensor it points at) or (None, None) without
    a prior: bias f32 [N], contiguous, on the catalogue's device; bias_weight None (1 for everyone),
    a Python number (one weight for everyone) or f32 [n], contiguous, on the queries' device."""
    from ._lib import STRUCTS
    if bias is None:
        _check(bias_weight is None, f"{who} takes a bias_weight only with a bias")
        return None, None
    N = items.shape[0]
    _check(isinstance(bias, torch.Tensor) and bias.dtype == torch.float32 and tuple(bias.shape) == (N,),
           f"bias must be f32 [N], one word per catalogue row (got {getattr(bias, 'dtype', type(bias).__name__)} "
           f"{tuple(getattr(bias, 'shape', ()))}, N={N})")
    _check(bias.is_contiguous(), "bias must be contiguous")
    _check(bias.device == items.device, "bias must be on the catalogue's device")
    w = bias_weight
    if w is not None and not isinstance(w, torch.Tensor):
        _check(isinstance(w, (int, float)) and not isinstance(w, bool),
               f"bias_weight must be None, a number or an f32 tensor [{per}] (got {type(w).__name__})")
        w = torch.full((n,), float(w), dtype=torch.float32, device=device)
    if w is not None:
        _check(w.dtype == torch.float32 and tuple(w.shape) == (n,),
               f"bias_weight must be f32 [{per}] (got {w.dtype} {tuple(w.shape)}, {per}={n})")
        _check(w.is_contiguous(), "bias_weight must be contiguous")
        _check(w.device == device, "bias_weight must be on the queries' device")
    b = STRUCTS["lthm_retrieve_bias"]()
    b.bias, b.weight = ptr(bias), ptr(w)
    return b, w


def retrieve_deep_passes(k: int):
    """The per-pass list lengths of a paged deep call (deep="paged"): ceil(k / 128) passes, all of
    RETRIEVE_MAX_K rows but the last, which takes the rest.  k in 1..RETRIEVE_MAX_DEEP."""
    k = int(k)
    _check(1 <= k <= RETRIEVE_MAX_DEEP, f"a deep list takes k in 1..{RETRIEVE_MAX_DEEP} (got {k})")
    full, rest = divmod(k, RETRIEVE_MAX_K)
    return [RETRIEVE_MAX_K] * full + ([rest] if rest else [])


def _retrieve_scan(who: str, q, items, k: int, kmax: int, normalize_q, target_rows, slab_rows, exclude_rows, tags,
                   tag_filter, after_scores, after_rows, bias, bias_weight, target_scores):
    """The one call path of retrieve_topk (q [Q, 128]) and retrieve_topk_group (q [U, G, 128]), which
    document the arguments: k in 1..kmax from one scan of the catalogue (csrc/retrieve.hip, retr_scan).
    The call is lthm_retrieve_topk_deep with the parts that are present, which picks the kernels by
    k and G; with target_scores it is lthm_retrieve_topk_shard, the scan of one shard of a catalogue,
    which counts rank against the given scores."""
    import ctypes
    from ._lib import STRUCTS
    grouped = who == "retrieve_topk_group"
    per, one = ("U", "user") if grouped else ("Q", "query")
    k = int(k)
    _check(1 <= k <= kmax, f"{who} takes k in 1..{kmax} (got {k}"
                           + (f"; deep=True takes up to {RETRIEVE_MAX_DEEP})" if kmax < RETRIEVE_MAX_DEEP else ")"))
    require_gpu(q, items, target_rows, exclude_rows, target_scores)
    _check(items.dim() == 2 and items.shape[1] == RETRIEVE_WIDTH and items.dtype == torch.bfloat16,
           f"{who} takes a bf16 [N, {RETRIEVE_WIDTH}] catalogue (got {items.dtype} {tuple(items.shape)})")
    if grouped:
        _check(q.dim() == 3 and q.shape[2] == RETRIEVE_WIDTH,
               f"{who} takes [U, G, {RETRIEVE_WIDTH}] queries (got {tuple(q.shape)})")
        G = q.shape[1]
        _check(1 <= G <= RETRIEVE_MAX_GROUP, f"{who} takes 1..{RETRIEVE_MAX_GROUP} queries per user (got {G})")
    else:
        _check(q.dim() == 2 and q.shape[1] == RETRIEVE_WIDTH,
               f"{who} takes [Q, {RETRIEVE_WIDTH}] queries (got {tuple(q.shape)})")
        G = 1
    U, N = q.shape[0], items.shape[0]
    _check(N >= 1 and U >= 1, f"{who} takes a non-empty catalogue and at least one {one} (N={N}, {per}={U})")
    dev = q.device
    x, X = None, 0
    if exclude_rows is not None:
        _check(exclude_rows.dtype == torch.int32 and exclude_rows.dim() == 2 and exclude_rows.shape[0] == U,
               f"exclude_rows must be int32 [{per}, X], one list per {one} (got {exclude_rows.dtype} "
               f"{tuple(exclude_rows.shape)}, {per}={U})")
        X = exclude_rows.shape[1]
        _check(1 <= X <= RETRIEVE_MAX_EXCLUDE, f"exclude_rows takes 1..{RETRIEVE_MAX_EXCLUDE} rows per {one} (got {X})")
        _check(exclude_rows.device == dev, "exclude_rows must be on the queries' device")
        x = STRUCTS["lthm_retrieve_excl"]()
        x.rows, x.X = ptr(exclude_rows), X
    if target_rows is not None:
        _check(target_rows.dtype == torch.int32 and target_rows.shape == (U,), f"target_rows must be int32 [{per}]")
    need = load().lthm_retrieve_deep_ws_bytes(U, G, N, k, int(slab_rows), X)
    _check(need >= 0, f"{who}: slab_rows={slab_rows} is not 0 or a multiple of {RETRIEVE_MIN_SLAB_ROWS} "
                      f"that cuts N={N} into at most 65535 slabs ({per}={U} G={G} k={k} X={X})")
    scores = torch.empty((U, k), dtype=torch.float32, device=dev)
    rows = torch.empty((U, k), dtype=torch.int32, device=dev)
    rank = tscore = sh = None
    if target_scores is not None:
        _check(target_scores.dtype == torch.float32 and tuple(target_scores.shape) == (U,),
               f"target_scores must be f32 [{per}] (got {target_scores.dtype} {tuple(target_scores.shape)}, {per}={U})")
        _check(target_scores.device == dev, "target_scores must be on the queries' device")
        rank = torch.empty(U, dtype=torch.int32, device=dev)  # the call writes no target score: the caller's are
        sh = STRUCTS["lthm_retrieve_shard"]()
        sh.target_score_in = ptr(target_scores)
    elif target_rows is not None:
        rank = torch.empty(U, dtype=torch.int32, device=dev)
        tscore = torch.empty(U, dtype=torch.float32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    d = STRUCTS["lthm_retrieve_desc"]()
    d.items, d.q, d.target_row = ptr(items), ptr(q), ptr(target_rows)
    d.scores, d.rows, d.rank, d.target_score = ptr(scores), ptr(rows), ptr(rank), ptr(tscore)
    d.workspace, d.ws_bytes = ptr(ws), need
    d.Q, d.N, d.k, d.q_dtype, d.normalize_q, d.slab_rows = U, N, k, dcode(q), int(bool(normalize_q)), int(slab_rows)
    g = None
    if grouped:
        g = STRUCTS["lthm_retrieve_group"]()
        g.G = G
    t = _retrieve_tags(who, tags, tag_filter, items, U, per)
    c = _retrieve_cursor(who, after_scores, after_rows, U, per, dev)
    b, bw = _retrieve_bias(who, bias, bias_weight, items, U, per, dev)
    # the timer's record: the key names the narrowest entry point that takes the call
    if sh is not None:
        key = "retr_shard_topk_k"
    elif k > RETRIEVE_MAX_K:
        key = "retr_deep_topk_k"
    else:
        part = "bias_" if b is not None else "after_" if c is not None else "tags_" if t is not None \
            else "excl_" if x is not None and not grouped else ""
        key = f"retr_topk_{'group_' if grouped else ''}{part}k"
    nbytes = float(N * RETRIEVE_WIDTH * 2 + q.numel() * q.element_size() + U * k * 8 + 4.0 * U * X) \
        + (4.0 * N + 12.0 * U if t is not None else 0.0) + (8.0 * U if c is not None else 0.0) \
        + (4.0 * N if b is not None else 0.0) + (4.0 * U if bw is not None else 0.0) + (4.0 * U if sh is not None else 0.0)
    parts = [ctypes.addressof(o) if o is not None else None for o in (d, x, g, t, c, b)]
    if sh is not None:
        parts.append(ctypes.addressof(sh))
    call("lthm_retrieve_topk_shard" if sh is not None else "lthm_retrieve_topk_deep", *parts, stream(),
         _key=key, _work=2.0 * U * G * N * RETRIEVE_WIDTH, _unit="flop", _bytes=nbytes)
    return scores, rows, rank, target_scores if sh is not None else tscore


def retrieve_target_score(q, items, target_rows, *, normalize_q: bool = True, bias=None, bias_weight=None):
    """The target_score that retrieve_topk (q [Q, 128]) or retrieve_topk_group (q [U, G, 128]) returns
    for the same arguments, bit for bit, without a scan of the catalogue (lthm_retrieve_target_score:
    the same prep kernels).  f32 [Q] or [U]; NaN where target_rows (int32) is outside [0, N): this
    shard of a catalogue does not hold the query's target."""
    require_gpu(q, items, target_rows)
    who = "retrieve_target_score"
    _check(items.dim() == 2 and items.shape[1] == RETRIEVE_WIDTH and items.dtype == torch.bfloat16,
           f"{who} takes a bf16 [N, {RETRIEVE_WIDTH}] catalogue (got {items.dtype} {tuple(items.shape)})")
    _check(q.dim() in (2, 3) and q.shape[-1] == RETRIEVE_WIDTH,
           f"{who} takes [Q, {RETRIEVE_WIDTH}] or [U, G, {RETRIEVE_WIDTH}] queries (got {tuple(q.shape)})")
    U, N = q.shape[0], items.shape[0]
    G = q.shape[1] if q.dim() == 3 else 1
    per = "U" if q.dim() == 3 else "Q"
    _check(1 <= G <= RETRIEVE_MAX_GROUP, f"{who} takes 1..{RETRIEVE_MAX_GROUP} queries per user (got {G})")
    _check(N >= 1 and U >= 1, f"{who} takes a non-empty catalogue and at least one query (N={N}, {per}={U})")
    _check(target_rows.dtype == torch.int32 and target_rows.shape == (U,), f"target_rows must be int32 [{per}]")
    dev = q.device
    bw = None
    if bias is not None or bias_weight is not None:
        bw = _retrieve_bias(who, bias, bias_weight, items, U, per, dev)[1]
    need = load().lthm_retrieve_target_score_ws_bytes(U, G)
    _check(need >= 0, f"{who}: no workspace size for {per}={U} G={G}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(U, dtype=torch.float32, device=dev)
    call("lthm_retrieve_target_score", ptr(items), N, ptr(q), dcode(q), int(bool(normalize_q)), G, ptr(target_rows),
         ptr(bias), ptr(bw), ptr(out), U, ptr(ws), need, stream(), _key="retr_target_score",
         _work=float(q.numel() * q.element_size() + U * (RETRIEVE_WIDTH * 2 + 8)), _unit="byte")
    return out


RETRIEVE_MAX_SHARDS = 64      # RS_SMAX: the most lists of one merge


def retrieve_merge_shards(scores, ids, ranks=None):
    """The k first entries of the union of S lists per query (lthm_retrieve_merge_shards,
    retr_shard_merge_k).  scores f32 [S, Q, k] and ids int64 [S, Q, k]: every list sorted by (score
    descending, id ascending) with its empty slots (-inf, 0) at the end, ids distinct across the
    lists of one query; ranks int32 [S, Q] or None.  1 <= S <= 64, 1 <= k <= 1024.  Returns (scores
    f32 [Q, k], ids int64 [Q, k], rank int64 [Q] | None): rank is -1 where any shard's is, else the
    sum.  -0 equals +0 and comes back as +0.  A pure function of the inputs."""
    require_gpu(scores, ids, ranks)
    _check(scores.dim() == 3 and scores.dtype == torch.float32,
           f"retrieve_merge_shards takes f32 scores [S, Q, k] (got {scores.dtype} {tuple(scores.shape)})")
    _check(ids.dtype == torch.int64 and ids.shape == scores.shape,
           f"retrieve_merge_shards takes int64 ids of the scores' shape (got {ids.dtype} {tuple(ids.shape)})")
    S, Q, k = scores.shape
    _check(1 <= S <= RETRIEVE_MAX_SHARDS, f"retrieve_merge_shards takes 1..{RETRIEVE_MAX_SHARDS} lists per query (got S={S})")
    _check(1 <= k <= RETRIEVE_MAX_DEEP, f"retrieve_merge_shards takes k in 1..{RETRIEVE_MAX_DEEP} (got {k})")
    _check(Q >= 1, "retrieve_merge_shards takes at least one query")
    _check(ids.device == scores.device, "scores and ids must be on one device")
    dev = scores.device
    out_rank = None
    if ranks is not None:
        _check(ranks.dtype == torch.int32 and tuple(ranks.shape) == (S, Q),
               f"ranks must be int32 [S, Q] (got {ranks.dtype} {tuple(ranks.shape)})")
        _check(ranks.device == dev, "ranks must be on the scores' device")
        out_rank = torch.empty(Q, dtype=torch.int64, device=dev)
    out_scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_ids = torch.empty((Q, k), dtype=torch.int64, device=dev)
    call("lthm_retrieve_merge_shards", ptr(scores), ptr(ids), ptr(ranks), S, Q, k, ptr(out_scores), ptr(out_ids),
         ptr(out_rank), stream(), _key="retr_shard_merge_k", _work=float(12 * S * Q * k + 12 * Q * k), _unit="byte")
    return out_scores, out_ids, out_rank


def _retrieve_deep(call, q, items, k: int, target_rows, after_scores, after_rows, kw):
    """deep="paged": k > RETRIEVE_MAX_K as passes of at most RETRIEVE_MAX_K rows: pass i + 1 starts behind the
    last column of pass i, which stays on the device (an exhausted pass ends in (-inf, -1), the
    cursor that admits nothing).  rank and target_score are the first pass's, whose cursor is the
    caller's own."""
    parts_s, parts_r = [], []
    rank = tscore = None
    cs, cr = after_scores, after_rows
    for i, kp in enumerate(retrieve_deep_passes(k)):
        s, r, rk, ts = call(q, items, kp, target_rows=target_rows if i == 0 else None, after_scores=cs, after_rows=cr, **kw)
        if i == 0:
            rank, tscore = rk, ts
        parts_s.append(s)
        parts_r.append(r)
        cs, cr = s[:, -1].contiguous(), r[:, -1].contiguous()
    return torch.cat(parts_s, dim=1), torch.cat(parts_r, dim=1), rank, tscore


def _retrieve_call(fn, q, items, k: int, deep, *, target_rows, after_scores, after_rows, target_scores, **kw):
    """retrieve_topk or retrieve_topk_group (fn): the deep / "paged" handling, then the scan."""
    who = fn.__name__
    bias, bias_weight = kw["bias"], kw["bias_weight"]
    _check(bias is not None or bias_weight is None, f"{who} takes a bias_weight only with a bias")
    _check(target_scores is None or deep != "paged", f'{who} takes target_scores with deep=False or True, not "paged"')
    if target_scores is None and deep and int(k) > RETRIEVE_MAX_K:
        _check(not isinstance(deep, str) or deep == "paged", f'{who} takes deep=False, True or "paged" (got {deep!r})')
        if deep == "paged":
            if bias is not None and bias_weight is not None and not isinstance(bias_weight, torch.Tensor):  # one tensor for all passes
                per = "U" if fn is retrieve_topk_group else "Q"
                kw["bias_weight"] = _retrieve_bias(who, bias, bias_weight, items, q.shape[0], per, q.device)[1]
            return _retrieve_deep(fn, q, items, k, target_rows, after_scores, after_rows, kw)
    return _retrieve_scan(who, q, items, k, RETRIEVE_MAX_DEEP if deep else RETRIEVE_MAX_K, target_rows=target_rows,
                          after_scores=after_scores, after_rows=after_rows, target_scores=target_scores, **kw)


def retrieve_topk(q, items, k: int, *, normalize_q: bool = True, target_rows=None, slab_rows: int = 0,
                  exclude_rows=None, tags=None, tag_filter=None, after_scores=None, after_rows=None,
                  deep: bool = False, bias=None, bias_weight=None, target_scores=None):
    """The k catalogue rows with the largest dot product per query (csrc/retrieve.hip).

    q f32 / bf16 [Q, 128]; items bf16 [N, 128] (normalised rows); target_rows int32 [Q] or None.
    Returns (scores f32 [Q, k], rows int32 [Q, k], rank int32 [Q] | None, target_score f32 [Q] |
    None), each query's entries sorted by (score descending, row ascending) and padded with
    -inf / -1 where N < k.  Forward only; no [Q, N] buffer is formed.

    exclude_rows int32 [Q, X] (contiguous, 1 <= X <= 1024) or None: rows query q must not
    return, in any order; entries outside [0, N) are ignored (-1 pads).  An excluded row is
    scored as -inf: it takes none of the k slots (the tail is -inf / -1 where fewer than k rows
    remain) and does not count in rank.  The target is never excluded as a target: target_score
    stays the plain dot, and rank counts the non-excluded rows other than the target scoring
    above it, also for a target inside its own list.

    tags int32 [N] and tag_filter int32 [Q, 3] = (all, any, none), together or neither: row j is
    eligible for query q iff (tags[j] & all) == all and (any == 0 or tags[j] & any != 0) and
    tags[j] & none == 0, the words read as 32 independent bits.  An ineligible row is treated
    exactly as an excluded one, and the target is never filtered as a target: rank counts the
    eligible, non-excluded rows other than the target scoring above its plain dot.  The filter
    (0, 0, 0) gives the bits of the call without tags.

    after_scores f32 [Q] and after_rows int32 [Q], together or neither: a cursor per query.  Row
    j with score s is eligible iff s < after_scores[q] or (s == after_scores[q] and j >
    after_rows[q]), in f32 on the kernel's own score; a row that is not is treated exactly as an
    excluded one (rank counts eligible rows only, target_score stays the plain dot).  A list's
    last (score, row) as the next call's cursor yields the following k rows of the same order,
    whatever slab_rows or Q either call used.  +inf gives the bits of the call without a cursor;
    -inf or NaN gives an empty list, so the (-inf, -1) tail of an exhausted list ends the paging.

    deep=True lifts the cap on k from 128 to RETRIEVE_MAX_DEEP = 1024: one call of
    lthm_retrieve_topk_deep, which selects the whole list in a single scan of the catalogue.
    deep="paged" gives the same bits the way a caller of the k <= 128 entries gets them:
    ceil(k / 128) passes, each behind the last column of the one before (no host sync),
    concatenated, one catalogue scan per 128 rows; rank and target_score are the first pass's,
    whose cursor is the caller's own, and the single scan returns those.  Without deep, k > 128 is
    refused as it always was.

    bias f32 [N] (contiguous, on the catalogue's device, every value finite) and bias_weight None, a
    number or f32 [Q]: a per-item score prior.  The score of row j for query q becomes
    fma(w[q], bias[j], dot) in f32, with w = 1 where bias_weight is None, and everything above
    (order, ties, the scores returned, cursors, rank) sees that score and only it; target_score is
    biased the same way and is the value rank counts against.  A row at -inf stays at -inf.
    bias_weight = 0 or an all-zero bias gives the rows and ranks of the call without a prior.  A
    non-finite weight gives that query an unspecified list.  A deep list carries the prior, in
    every pass where it is paged.

    target_scores f32 [Q]: the catalogue is one shard of a larger one and these are the targets'
    scores, wherever the targets live (lthm_retrieve_topk_shard; retrieve_target_score computes
    them on the shard that holds the target).  rank[q] then counts the eligible rows other than
    target_rows[q] (None, or -1 where this shard does not hold the target) that score strictly above
    target_scores[q], for every query, -1 where target_scores[q] is NaN; scores and rows are those
    of the call without it, and the target_score returned is the tensor given.  deep="paged" does
    not take it."""
    return _retrieve_call(retrieve_topk, q, items, k, deep, normalize_q=normalize_q, target_rows=target_rows,
                          slab_rows=slab_rows, exclude_rows=exclude_rows, tags=tags, tag_filter=tag_filter,
                          after_scores=after_scores, after_rows=after_rows, bias=bias, bias_weight=bias_weight,
                          target_scores=target_scores)


RETRIEVE_MAX_GROUP = 8        # RT_GMAX: the most queries of one user


def retrieve_topk_group(q, items, k: int, *, normalize_q: bool = True, target_rows=None, slab_rows: int = 0,
                        exclude_rows=None, tags=None, tag_filter=None, after_scores=None, after_rows=None,
                        deep: bool = False, bias=None, bias_weight=None, target_scores=None):
    """retrieve_topk for users with several queries each: an item's score is its best over the
    user's queries, s[u, j] = max_g s_g[u, j], with s_g the score retrieve_topk gives query
    (u, g) (csrc/retrieve.hip, retr_topk_k<EXCL, GP>).

    q f32 / bf16 [U, G, 128], 1 <= G <= 8; items bf16 [N, 128]; target_rows int32 [U] or None;
    exclude_rows int32 [U, X] or None, one list per user under retrieve_topk's rules.  Returns
    (scores f32 [U, k], rows int32 [U, k], rank int32 [U] | None, target_score f32 [U] | None) by
    (score descending, row ascending), -inf / -1 where fewer than k rows remain.  target_score
    is the best of the user's plain target dots and rank = #{j != target, j not excluded :
    s[u, j] > target_score[u]} (-1 where the target is no catalogue row).  The outputs do not
    depend on the order of a user's queries; G = 1 is retrieve_topk on q[:, 0].  Which query
    attained a score is not reported.  tags int32 [N] and tag_filter int32 [U, 3], one filter per
    user, are retrieve_topk's: an ineligible row is -inf for the user, like an excluded one.
    after_scores f32 [U] and after_rows int32 [U], one cursor per user on the best-over-queries
    score, and deep=True (k up to RETRIEVE_MAX_DEEP in one catalogue scan; deep="paged": one scan per
    128 rows) are retrieve_topk's as well.  So are bias f32 [N] and bias_weight (None, a number or f32 [U], one
    weight per user): the prior is added to the best-over-queries score, fma(w[u], bias[j],
    max_g s_g[u, j]), which equals the best biased score since the fma is monotone in the dot.
    target_scores f32 [U], the targets' scores for one shard of a catalogue, is retrieve_topk's too."""
    return _retrieve_call(retrieve_topk_group, q, items, k, deep, normalize_q=normalize_q, target_rows=target_rows,
                          slab_rows=slab_rows, exclude_rows=exclude_rows, tags=tags, tag_filter=tag_filter,
                          after_scores=after_scores, after_rows=after_rows, bias=bias, bias_weight=bias_weight,
                          target_scores=target_scores)


RETRIEVE_MAX_PROBE = RETRIEVE_MAX_SHARDS  # the most lists one query probes: the merge's RS_SMAX


def retrieve_ivf_grid(Q: int, P: int, L: int) -> int:
    """The grid of the clustered scan (lthm_retrieve_ivf_grid): Q P // 64 + min(L, Q P), an upper bound
    on sum_c ceil(n_c / 64) over the lists' pair counts n_c, whatever they are (sum_c n_c <= Q P)."""
    n = int(load().lthm_retrieve_ivf_grid(int(Q), int(P), int(L)))
    _check(n >= 0, f"retrieve_ivf_grid takes Q, P, L >= 1 (got Q={Q} P={P} L={L})")
    return n


def _retrieve_ivf_cursor(who: str, after_scores, after_ids, Q: int, device):
    """The lthm_retrieve_ivf_cursor of a call, or None without a cursor: after_scores f32 [Q] and
    after_ids int64 [Q], contiguous, on the queries' device, both or neither."""
    from ._lib import STRUCTS
    _check((after_scores is None) == (after_ids is None), f"{who} takes after_scores and after_ids together or neither")
    if after_scores is None:
        return None
    _check(after_scores.dtype == torch.float32 and tuple(after_scores.shape) == (Q,),
           f"after_scores must be f32 [Q] (got {after_scores.dtype} {tuple(after_scores.shape)}, Q={Q})")
    _check(after_ids.dtype == torch.int64 and tuple(after_ids.shape) == (Q,),
           f"after_ids must be int64 [Q] (got {after_ids.dtype} {tuple(after_ids.shape)}, Q={Q})")
    _check(after_scores.is_contiguous() and after_ids.is_contiguous(), "after_scores and after_ids must be contiguous")
    _check(after_scores.device == device and after_ids.device == device,
           "after_scores and after_ids must be on the queries' device")
    c = STRUCTS["lthm_retrieve_ivf_cursor"]()
    c.after_score, c.after_id = ptr(after_scores), ptr(after_ids)
    return c


RETRIEVE_IVF_DEEP_WS_BYTES = 1 << 30  # the most workspace one deep clustered call takes: above it the queries are split


def retrieve_ivf_topk(q, items, row_ids, list_off, probes, k: int, *, normalize_q: bool = True, exclude_rows=None,
                      tags=None, tag_filter=None, bias=None, bias_weight=None, after_scores=None, after_ids=None,
                      deep: bool = False):
    """The k best items per query among the lists the query probes (lthm_retrieve_ivf_topk,
    csrc/retrieve.hip retr_ivf_topk_k): the scan of a clustered catalogue.

    q f32 / bf16 [Q, 128]; items bf16 [N, 128], list-major (list c is rows list_off[c] ..
    list_off[c + 1], ids ascending inside a list); row_ids int64 [N], the item id of every row;
    list_off int64 [L + 1]; probes int32 [Q, P], 1 <= P <= 64, the lists of every query, entries
    outside [0, L) ignored (-1 pads); exclude_rows int32 [Q, X] or None, rows in this catalogue's own
    numbering, under retrieve_topk's rules.  Returns (scores f32 [Q, k], ids int64 [Q, k]), 1 <= k <=
    128: the first k under (score descending, id ascending) of the probed, non-excluded rows, then
    (-inf, 0); every score has the bits retrieve_topk returns for the same (query, row).  One call:
    the query preparation, the plan, the scan and the merge run on the device without a host sync.

    tags int32 [N] with tag_filter int32 [Q, 3], bias f32 [N] with bias_weight (None, a number or f32
    [Q]), and after_scores f32 [Q] with after_ids int64 [Q] are retrieve_topk's filters, prior and
    cursor on the probed rows (lthm_retrieve_ivf_topk_filt): tags and bias in this catalogue's own
    row order, the cursor an id, since the cursor row differs per list.  The result is the k first
    of the probed, non-excluded rows that pass the filter and lie strictly behind (after_score,
    after_id), every score fma(w[q], bias[row], dot) as retrieve_topk returns it; with every list
    probed it is retrieve_topk's list.  With none of them the call is the one it always was.

    deep=True lifts k to RETRIEVE_MAX_DEEP = 1024 (lthm_retrieve_ivf_topk_deep, retr_ivf_deep_topk_k):
    the same contract, every score with the bits retrieve_topk(deep=True) returns; k <= 128 then runs
    the kernels it always ran.  Above 128 every (query, probe) pair holds 16 KiB of candidates in the
    workspace, so where one call would take more than RETRIEVE_IVF_DEEP_WS_BYTES (1 GiB) the queries
    go through in consecutive chunks, each one call: a query's list does not depend on the other
    queries, so the split changes no bit.  Without deep, k > 128 is refused as it always was."""
    return _retrieve_ivf_scan("retrieve_ivf_topk", q, items, row_ids, list_off, probes, k, normalize_q, exclude_rows,
                              tags, tag_filter, bias, bias_weight, after_scores, after_ids, deep)


def retrieve_ivf_group_grid(U: int, G: int, P: int, L: int) -> int:
    """The grid of the clustered scan with G queries per user (lthm_retrieve_ivf_group_grid): U P // T +
    min(L, U P) with T = 4 (16 // G) pairs per tile, an upper bound on sum_c ceil(n_c / T) over the lists'
    pair counts n_c, whatever they are (sum_c n_c <= U P).  At G = 1 it is retrieve_ivf_grid."""
    n = int(load().lthm_retrieve_ivf_group_grid(int(U), int(G), int(P), int(L)))
    _check(n >= 0, f"retrieve_ivf_group_grid takes U, P, L >= 1 and G in 1..{RETRIEVE_MAX_GROUP} "
                   f"(got U={U} G={G} P={P} L={L})")
    return n


def retrieve_ivf_topk_group(q, items, row_ids, list_off, probes, k: int, *, normalize_q: bool = True, exclude_rows=None,
                            tags=None, tag_filter=None, bias=None, bias_weight=None, after_scores=None, after_ids=None):
    """retrieve_ivf_topk for users with several queries each (lthm_retrieve_ivf_topk_group, csrc/retrieve.hip
    retr_ivf_topk_k<true, true, TAGS, BIAS, true>): an item's score is its best over the user's queries,
    s[u, j] = max_g s_g[u, j] with s_g the score retrieve_topk gives query (u, g), taken inside the scan
    ahead of candidate selection, so an item takes one slot per user.

    q f32 / bf16 [U, G, 128], 1 <= G <= 8; probes int32 [U, P], one probe row per user; exclude_rows int32
    [U, X], tag_filter int32 [U, 3], bias_weight (None, a number or f32 [U]) and after_scores f32 [U] /
    after_ids int64 [U] are per user and mean what they mean in retrieve_ivf_topk, applied to s[u, j] in
    retrieve_topk_group's order (the prior behind the maximum, then exclusion, tags and the cursor).
    Returns (scores f32 [U, k], ids int64 [U, k]), 1 <= k <= 128 (no deep lists with groups): the first k
    under (score descending, id ascending) of the probed, eligible rows, then (-inf, 0).  The outputs do
    not depend on the order of a user's queries; with every list probed they are retrieve_topk_group's for
    the same arguments, bit for bit, and G = 1 is retrieve_ivf_topk on q[:, 0]: the same kernels."""
    return _retrieve_ivf_scan("retrieve_ivf_topk_group", q, items, row_ids, list_off, probes, k, normalize_q,
                              exclude_rows, tags, tag_filter, bias, bias_weight, after_scores, after_ids, False)


def _retrieve_ivf_scan(who: str, q, items, row_ids, list_off, probes, k: int, normalize_q, exclude_rows, tags,
                       tag_filter, bias, bias_weight, after_scores, after_ids, deep):
    """The one call path of retrieve_ivf_topk (q [Q, 128]) and retrieve_ivf_topk_group (q [U, G, 128]),
    which document the arguments (csrc/retrieve.hip, retr_ivf_call).  Below, Q counts the users of a
    grouped call."""
    import ctypes
    from ._lib import STRUCTS
    grouped = who == "retrieve_ivf_topk_group"
    require_gpu(q, items, row_ids, list_off, probes, exclude_rows, tags, tag_filter, bias, after_scores, after_ids)
    _check(items.dim() == 2 and items.shape[1] == RETRIEVE_WIDTH and items.dtype == torch.bfloat16,
           f"{who} takes a bf16 [N, {RETRIEVE_WIDTH}] catalogue (got {items.dtype} {tuple(items.shape)})")
    G = 1
    if grouped:
        _check(q.dim() == 3 and q.shape[2] == RETRIEVE_WIDTH,
               f"{who} takes [U, G, {RETRIEVE_WIDTH}] queries (got {tuple(q.shape)})")
        G = q.shape[1]
        _check(1 <= G <= RETRIEVE_MAX_GROUP, f"{who} takes 1..{RETRIEVE_MAX_GROUP} queries per user (got {G})")
    else:
        _check(q.dim() == 2 and q.shape[1] == RETRIEVE_WIDTH,
               f"{who} takes [Q, {RETRIEVE_WIDTH}] queries (got {tuple(q.shape)})")
    Q, N, k = q.shape[0], items.shape[0], int(k)
    if deep:
        _check(1 <= k <= RETRIEVE_MAX_DEEP, f"{who} with deep=True takes k in 1..{RETRIEVE_MAX_DEEP} (got {k})")
    else:
        _check(1 <= k <= RETRIEVE_MAX_K, f"{who} takes k in 1..{RETRIEVE_MAX_K} (got {k})")
    deep = bool(deep) and k > RETRIEVE_MAX_K
    _check(N >= 1 and Q >= 1, f"{who} takes a non-empty catalogue and at least one query (N={N}, Q={Q})")
    _check(row_ids.dtype == torch.int64 and tuple(row_ids.shape) == (N,),
           f"row_ids must be int64 [N], one id per catalogue row (got {row_ids.dtype} {tuple(row_ids.shape)}, N={N})")
    _check(list_off.dtype == torch.int64 and list_off.dim() == 1 and list_off.shape[0] >= 2,
           f"list_off must be int64 [L + 1], L >= 1 (got {list_off.dtype} {tuple(list_off.shape)})")
    L = list_off.shape[0] - 1
    _check(probes.dtype == torch.int32 and probes.dim() == 2 and probes.shape[0] == Q,
           f"probes must be int32 [Q, P] (got {probes.dtype} {tuple(probes.shape)}, Q={Q})")
    P = probes.shape[1]
    _check(1 <= P <= RETRIEVE_MAX_PROBE, f"{who} takes 1..{RETRIEVE_MAX_PROBE} probes per query (got P={P})")
    _check(row_ids.is_contiguous() and list_off.is_contiguous() and probes.is_contiguous() and items.is_contiguous(),
           "items, row_ids, list_off and probes must be contiguous")
    _check(row_ids.device == items.device and list_off.device == items.device,
           "row_ids and list_off must be on the catalogue's device")
    _check(probes.device == q.device and q.device == items.device, "q and probes must be on the catalogue's device")
    X = 0
    x = None
    if exclude_rows is not None:
        _check(exclude_rows.dtype == torch.int32 and exclude_rows.dim() == 2 and exclude_rows.shape[0] == Q,
               f"exclude_rows must be int32 [Q, X] (got {exclude_rows.dtype} {tuple(exclude_rows.shape)}, Q={Q})")
        X = exclude_rows.shape[1]
        _check(1 <= X <= RETRIEVE_MAX_EXCLUDE, f"exclude_rows takes 1..{RETRIEVE_MAX_EXCLUDE} rows per query (got {X})")
        _check(exclude_rows.is_contiguous(), "exclude_rows must be contiguous")
        _check(exclude_rows.device == q.device, "exclude_rows must be on the queries' device")
        x = STRUCTS["lthm_retrieve_excl"]()
        x.rows, x.X = ptr(exclude_rows), X
    dev = q.device
    t = _retrieve_tags(who, tags, tag_filter, items, Q, "Q")
    b, bw = _retrieve_bias(who, bias, bias_weight, items, Q, "Q", dev)
    c = _retrieve_ivf_cursor(who, after_scores, after_ids, Q, dev)
    filt = t is not None or b is not None or c is not None
    if deep:
        return _retrieve_ivf_deep(q, items, row_ids, list_off, probes, k, normalize_q, exclude_rows, tags, tag_filter,
                                  bias, bw, after_scores, after_ids)
    if grouped:
        need = load().lthm_retrieve_ivf_group_ws_bytes(Q, G, N, L, P, k, X, int(c is not None))
    elif filt:
        need = load().lthm_retrieve_ivf_filt_ws_bytes(Q, N, L, P, k, X, int(c is not None))
    else:
        need = load().lthm_retrieve_ivf_ws_bytes(Q, N, L, P, k, X)
    _check(need >= 0, f"{who}: no workspace size for Q={Q} N={N} L={L} P={P} k={k} X={X} (Q P must stay below 2^31)")
    q = q.contiguous()
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    ids = torch.empty((Q, k), dtype=torch.int64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    work = float(q.numel() * q.element_size() + 24.0 * P * Q * k + 12.0 * Q * k + 4.0 * Q * (P + X))
    if not filt and not grouped:
        call("lthm_retrieve_ivf_topk", ptr(items), N, ptr(row_ids), ptr(list_off), L, ptr(q), dcode(q),
             int(bool(normalize_q)), Q, ptr(probes), P, k, ctypes.addressof(x) if x is not None else None, ptr(scores),
             ptr(ids), ptr(ws), need, stream(), _key="retr_ivf_topk_k", _work=work, _unit="byte")
        return scores, ids
    parts = [ctypes.addressof(o) if o is not None else None for o in (x, t, b, c)]
    work += (12.0 * Q if t is not None else 0.0) + (4.0 * Q if bw is not None else 0.0) \
        + (12.0 * Q + 4.0 * Q * P if c is not None else 0.0)
    if grouped:
        g = STRUCTS["lthm_retrieve_group"]()
        g.G = G
        call("lthm_retrieve_ivf_topk_group", ptr(items), N, ptr(row_ids), ptr(list_off), L, ptr(q), dcode(q),
             int(bool(normalize_q)), Q, ctypes.addressof(g), ptr(probes), P, k, *parts, ptr(scores), ptr(ids), ptr(ws),
             need, stream(), _key="retr_ivf_topk_group_k", _work=work, _unit="byte")
        return scores, ids
    call("lthm_retrieve_ivf_topk_filt", ptr(items), N, ptr(row_ids), ptr(list_off), L, ptr(q), dcode(q),
         int(bool(normalize_q)), Q, ptr(probes), P, k, *parts, ptr(scores), ptr(ids), ptr(ws), need, stream(),
         _key="retr_ivf_topk_filt_k", _work=work, _unit="byte")
    return scores, ids


def _retrieve_ivf_deep(q, items, row_ids, list_off, probes, k, normalize_q, exclude_rows, tags, tag_filter, bias, bw,
                       after_scores, after_ids):
    """retrieve_ivf_topk's deep call on checked arguments (bw: the weights as f32 [Q] or None): one
    lthm_retrieve_ivf_topk_deep per chunk of consecutive queries, the largest chunk whose workspace
    stays within RETRIEVE_IVF_DEEP_WS_BYTES (one query at the least)."""
    import ctypes
    from ._lib import STRUCTS
    Q, N, L, P = q.shape[0], items.shape[0], list_off.shape[0] - 1, probes.shape[1]
    X = 0 if exclude_rows is None else exclude_rows.shape[1]
    has_c = int(after_scores is not None)
    size = lambda n: load().lthm_retrieve_ivf_deep_ws_bytes(n, N, L, P, k, X, has_c)
    _check(size(Q) >= 0, f"retrieve_ivf_topk: no workspace size for Q={Q} N={N} L={L} P={P} k={k} X={X} "
                         "(Q P must stay below 2^31)")
    step = Q
    if size(Q) > RETRIEVE_IVF_DEEP_WS_BYTES:
        lo, hi = 1, Q  # the size ascends with the queries: the most queries that fit, by bisection
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if size(mid) <= RETRIEVE_IVF_DEEP_WS_BYTES else (lo, mid - 1)
        step = lo
    dev = q.device
    q = q.contiguous()
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    ids = torch.empty((Q, k), dtype=torch.int64, device=dev)
    ws = torch.empty(size(step), dtype=torch.uint8, device=dev)
    for q0 in range(0, Q, step):
        n = min(step, Q - q0)
        cut = lambda v: None if v is None else v[q0:q0 + n]  # a contiguous tensor's leading rows are contiguous
        x = t = b = c = None
        if exclude_rows is not None:
            x = STRUCTS["lthm_retrieve_excl"]()
            x.rows, x.X = ptr(cut(exclude_rows)), X
        if tags is not None:
            t = STRUCTS["lthm_retrieve_tags"]()
            t.tags, t.filter = ptr(tags), ptr(cut(tag_filter))
        if bias is not None:
            b = STRUCTS["lthm_retrieve_bias"]()
            b.bias, b.weight = ptr(bias), (ptr(cut(bw)) if bw is not None else None)
        if after_scores is not None:
            c = STRUCTS["lthm_retrieve_ivf_cursor"]()
            c.after_score, c.after_id = ptr(cut(after_scores)), ptr(cut(after_ids))
        parts = [ctypes.addressof(o) if o is not None else None for o in (x, t, b, c)]
        work = float(n * RETRIEVE_WIDTH * q.element_size() + 24.0 * P * n * k + 12.0 * n * k + 4.0 * n * (P + X))
        call("lthm_retrieve_ivf_topk_deep", ptr(items), N, ptr(row_ids), ptr(list_off), L, ptr(cut(q)), dcode(q),
             int(bool(normalize_q)), n, ptr(cut(probes)), P, k, *parts, ptr(cut(scores)), ptr(cut(ids)), ptr(ws),
             ws.numel(), stream(), _key="retr_ivf_deep_topk_k", _work=work, _unit="byte")
    return scores, ids


def retrieve_ivf_shard_descs(shards):
    """The host array of lthm_retrieve_ivf_shard for ``shards``, a sequence of (items bf16 [N, 128], row_ids
    int64 [N], list_off int64 [L + 1], centroids bf16 [L, 128], tags int32 [N] | None, bias f32 [N] | None),
    all contiguous and on one device.  The array holds pointers only: the caller keeps the tensors alive."""
    from ._lib import STRUCTS
    S = len(shards)
    _check(1 <= S <= RETRIEVE_MAX_SHARDS, f"retrieve_ivf_topk_shards takes 1..{RETRIEVE_MAX_SHARDS} shards (got S={S})")
    arr = (STRUCTS["lthm_retrieve_ivf_shard"] * S)()
    dev = shards[0][0].device
    for i, (items, row_ids, list_off, centroids, tags, bias) in enumerate(shards):
        require_gpu(items, row_ids, list_off, centroids, tags, bias)
        N, L = items.shape[0], centroids.shape[0]
        _check(items.dtype == torch.bfloat16 and items.dim() == 2 and items.shape[1] == RETRIEVE_WIDTH and N >= 1,
               f"shard {i}: items must be bf16 [N, {RETRIEVE_WIDTH}] (got {items.dtype} {tuple(items.shape)})")
        _check(centroids.dtype == torch.bfloat16 and centroids.dim() == 2 and centroids.shape[1] == RETRIEVE_WIDTH and L >= 1,
               f"shard {i}: centroids must be bf16 [L, {RETRIEVE_WIDTH}] (got {centroids.dtype} {tuple(centroids.shape)})")
        _check(row_ids.dtype == torch.int64 and tuple(row_ids.shape) == (N,), f"shard {i}: row_ids must be int64 [N]")
        _check(list_off.dtype == torch.int64 and tuple(list_off.shape) == (L + 1,), f"shard {i}: list_off must be int64 [L + 1]")
        _check(tags is None or (tags.dtype == torch.int32 and tuple(tags.shape) == (N,)), f"shard {i}: tags must be int32 [N]")
        _check(bias is None or (bias.dtype == torch.float32 and tuple(bias.shape) == (N,)), f"shard {i}: bias must be f32 [N]")
        _check(all(t is None or t.device == dev for t in (items, row_ids, list_off, centroids, tags, bias)),
               "the shards of one call must be on one device")
        d = arr[i]
        d.items, d.row_ids, d.list_off, d.centroids = ptr(items), ptr(row_ids), ptr(list_off), ptr(centroids)
        d.tags, d.bias, d.N, d.L = ptr(tags), ptr(bias), N, L
    return arr


def retrieve_ivf_topk_shards(q, shards, nprobe: int, k: int, *, normalize_q: bool = True, exclude_rows=None,
                             tag_filter=None, use_bias: bool = False, bias_weight=None, after_scores=None,
                             after_ids=None, target_rows=None, target_scores=None, out=None):
    """The k best items per query over S clustered catalogues of one device, each probing its own
    min(nprobe, L_s) nearest lists (lthm_retrieve_ivf_topk_shards, csrc/retrieve.hip): one plan, one scan
    launch (retr_ivf_topk_k / retr_ivf_deep_topk_k with the shard descriptors) and one merge for all shards.

    ``shards``: the tuples retrieve_ivf_shard_descs takes (the descriptors are rebuilt per call: a few dozen
    small structs); q f32 / bf16 [Q, 128]; exclude_rows int32 [S, Q, X] or None, the excluded rows in
    every shard's own numbering; tag_filter int32 [Q, 3] (every shard then carries tags); use_bias scores
    with every shard's bias and bias_weight (None, a number or f32 [Q]); after_scores f32 [Q] / after_ids
    int64 [Q], the cursor.  k in 1..1024; the probe slots of all shards together number at most 64.
    target_rows int32 [S, Q] (the row of every query's target in every shard, -1 where it is not there) with
    target_scores f32 [Q] (retrieve_target_score on the shard that holds the target; NaN: none does), both
    or neither: rank then counts the eligible rows of the probed lists, other than the target's, that score
    strictly above the target score (inside the scan, on its own scores).  ``out``: (scores, ids) f32 / int64
    [Q, k] contiguous tensors to write into.
    Returns (scores f32 [Q, k], ids int64 [Q, k], rank int64 [Q] | None): scores and ids bit for bit what one
    retrieve_ivf_topk(deep=True) per shard, each with the shard's own probe row, followed by
    retrieve_merge_shards returns."""
    import ctypes
    who = "retrieve_ivf_topk_shards"
    arr = retrieve_ivf_shard_descs(shards)
    S = len(arr)
    require_gpu(q, exclude_rows, tag_filter, after_scores, after_ids, target_rows, target_scores)
    _check(q.dim() == 2 and q.shape[1] == RETRIEVE_WIDTH and q.shape[0] >= 1,
           f"{who} takes [Q, {RETRIEVE_WIDTH}] queries (got {tuple(q.shape)})")
    Q, k = q.shape[0], int(k)
    dev = q.device
    _check(shards[0][0].device == dev, "q must be on the shards' device")
    _check(isinstance(nprobe, int) and not isinstance(nprobe, bool) and nprobe >= 1, f"{who} takes nprobe >= 1 (got {nprobe!r})")
    _check(1 <= k <= RETRIEVE_MAX_DEEP, f"{who} takes k in 1..{RETRIEVE_MAX_DEEP} (got {k})")
    X = 0
    if exclude_rows is not None:
        _check(exclude_rows.dtype == torch.int32 and exclude_rows.dim() == 3 and tuple(exclude_rows.shape[:2]) == (S, Q),
               f"exclude_rows must be int32 [S, Q, X] (got {exclude_rows.dtype} {tuple(exclude_rows.shape)}, S={S}, Q={Q})")
        X = exclude_rows.shape[2]
        _check(1 <= X <= RETRIEVE_MAX_EXCLUDE, f"exclude_rows takes 1..{RETRIEVE_MAX_EXCLUDE} rows per query (got {X})")
        _check(exclude_rows.device == dev, "exclude_rows must be on the queries' device")
    if tag_filter is not None:
        _check(tag_filter.dtype == torch.int32 and tuple(tag_filter.shape) == (Q, 3) and tag_filter.device == dev,
               f"tag_filter must be int32 [Q, 3] on the queries' device (got {tag_filter.dtype} {tuple(tag_filter.shape)})")
        _check(all(s[4] is not None for s in shards), f"{who} takes a tag_filter only where every shard carries tags")
    bw = None
    if use_bias:
        _check(all(s[5] is not None for s in shards), f"{who} takes use_bias only where every shard carries a bias")
        bw = bias_weight
        if bw is not None and not isinstance(bw, torch.Tensor):
            _check(isinstance(bw, (int, float)) and not isinstance(bw, bool),
                   f"bias_weight must be None, a number or an f32 tensor [Q] (got {type(bw).__name__})")
            bw = torch.full((Q,), float(bw), dtype=torch.float32, device=dev)
        if bw is not None:
            require_gpu(bw)
            _check(bw.dtype == torch.float32 and tuple(bw.shape) == (Q,) and bw.device == dev,
                   f"bias_weight must be f32 [Q] on the queries' device (got {bw.dtype} {tuple(bw.shape)}, Q={Q})")
    else:
        _check(bias_weight is None, f"{who} takes a bias_weight only with use_bias")
    c = _retrieve_ivf_cursor(who, after_scores, after_ids, Q, dev)
    need = load().lthm_retrieve_ivf_shards_ws_bytes(ctypes.addressof(arr), S, Q, nprobe, k, X, int(c is not None))
    _check(need >= 0, f"{who}: no workspace size for S={S} Q={Q} nprobe={nprobe} k={k} X={X} "
                      f"(the probe slots of all shards together must stay within {RETRIEVE_MAX_PROBE})")
    _check((target_rows is None) == (target_scores is None), f"{who} takes target_rows and target_scores together or neither")
    rank = None
    if target_rows is not None:
        _check(target_rows.dtype == torch.int32 and tuple(target_rows.shape) == (S, Q) and target_rows.device == dev,
               f"target_rows must be int32 [S, Q] on the queries' device (got {target_rows.dtype} {tuple(target_rows.shape)})")
        _check(target_scores.dtype == torch.float32 and tuple(target_scores.shape) == (Q,) and target_scores.device == dev,
               f"target_scores must be f32 [Q] on the queries' device (got {target_scores.dtype} {tuple(target_scores.shape)})")
        rank = torch.empty(Q, dtype=torch.int64, device=dev)
    if out is not None:
        scores, ids = out
        require_gpu(scores, ids)
        _check(scores.dtype == torch.float32 and ids.dtype == torch.int64 and tuple(scores.shape) == (Q, k)
               and tuple(ids.shape) == (Q, k) and scores.device == dev and ids.device == dev,
               f"out must be (f32 [Q, k], int64 [Q, k]) on the queries' device")
    else:
        scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
        ids = torch.empty((Q, k), dtype=torch.int64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    P = sum(min(nprobe, s[3].shape[0]) for s in shards)
    work = float(q.numel() * q.element_size() + 24.0 * P * Q * k + 12.0 * Q * k + 4.0 * Q * (P + S * X))
    call("lthm_retrieve_ivf_topk_shards", ctypes.addressof(arr), S, ptr(q), dcode(q), int(bool(normalize_q)), Q, nprobe, k,
         ptr(exclude_rows), X, ptr(tag_filter), int(bool(use_bias)), ptr(bw),
         ctypes.addressof(c) if c is not None else None, ptr(target_rows), ptr(target_scores), ptr(scores), ptr(ids),
         ptr(rank), ptr(ws), need, stream(), _key="retr_ivf_topk_shards_k", _work=work, _unit="byte")
    return scores, ids, rank


RETRIEVE_MAX_POOL = RETRIEVE_MAX_DEEP  # RV_MMAX: the largest candidate pool of retrieve_diversify (a deep list)


def retrieve_diversify(items, rows, scores, k: int, *, lam=None, groups=None, cap: int = 1):
    """Greedy maximal-marginal-relevance selection of k out of a pool of M candidates per query, with
    at most `cap` selected items per group (lthm_retrieve_diversify, csrc/retrieve.hip retr_diversify_k).

    items bf16 [N, 128], the flat catalogue; rows int32 [Q, M] and scores f32 [Q, M], 1 <= M <= 1024,
    the pool in any order (what retrieve_topk returned, deep=True for more than 128): an entry with a
    row outside [0, N) or a score of -inf or NaN is no candidate.  k in 1..128.  lam f32 [Q] in [0, 1]
    or None (1 everywhere); groups int32 [N] or None, key 0 = never capped; cap >= 1 (ignored without
    groups).  k times per query the eligible candidate first under (m descending, row ascending) is
    selected, m_i = fmaf(-(1 - lam), d_i, lam s_i) with d_i the largest f32 dot of row i with a row
    selected so far (0 at the start).  Returns (rows int32 [Q, k], scores f32 [Q, k], objective f32
    [Q, k]) in selection order: the caller's score of every selected row and m at its selection; empty
    slots are (-1, -inf, -inf).  lam = 1 without groups is the pool's first k under (score descending,
    row ascending).  One block per query, no host sync, a pure function of the inputs."""
    who = "retrieve_diversify"
    require_gpu(items, rows, scores, lam, groups)
    _check(items.dim() == 2 and items.shape[1] == RETRIEVE_WIDTH and items.dtype == torch.bfloat16,
           f"{who} takes a bf16 [N, {RETRIEVE_WIDTH}] catalogue (got {items.dtype} {tuple(items.shape)})")
    _check(rows.dim() == 2 and rows.dtype == torch.int32, f"{who} takes int32 rows [Q, M] (got {rows.dtype} {tuple(rows.shape)})")
    _check(scores.dtype == torch.float32 and scores.shape == rows.shape,
           f"{who} takes f32 scores of the rows' shape (got {scores.dtype} {tuple(scores.shape)})")
    (Q, M), N, k, cap = rows.shape, items.shape[0], int(k), int(cap)
    _check(1 <= M <= RETRIEVE_MAX_POOL, f"{who} takes a pool of 1..{RETRIEVE_MAX_POOL} candidates (got M={M})")
    _check(1 <= k <= RETRIEVE_MAX_K, f"{who} takes k in 1..{RETRIEVE_MAX_K} (got {k})")
    _check(N >= 1 and Q >= 1, f"{who} takes a non-empty catalogue and at least one query (N={N}, Q={Q})")
    dev = items.device
    _check(rows.device == dev and scores.device == dev, "rows and scores must be on the catalogue's device")
    if lam is not None:
        _check(lam.dtype == torch.float32 and tuple(lam.shape) == (Q,), f"lam must be f32 [Q] (got {lam.dtype} {tuple(lam.shape)}, Q={Q})")
        _check(lam.device == dev, "lam must be on the catalogue's device")
    if groups is not None:
        _check(groups.dtype == torch.int32 and tuple(groups.shape) == (N,),
               f"groups must be int32 [N], one key per catalogue row (got {groups.dtype} {tuple(groups.shape)}, N={N})")
        _check(groups.device == dev, "groups must be on the catalogue's device")
        _check(cap >= 1, f"{who} takes cap >= 1 (got {cap})")
    need = load().lthm_retrieve_diversify_ws_bytes(Q, M, k)
    _check(need >= 0, f"{who}: no workspace size for Q={Q} M={M} k={k}")
    out_rows = torch.empty((Q, k), dtype=torch.int32, device=dev)
    out_scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_obj = torch.empty((Q, k), dtype=torch.float32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    call("lthm_retrieve_diversify", ptr(items), N, ptr(rows), ptr(scores), Q, M, k, ptr(lam), ptr(groups), max(cap, 1),
         ptr(out_rows), ptr(out_scores), ptr(out_obj), ptr(ws), need, stream(), _key="retr_diversify_k",
         _work=2.0 * Q * k * M * RETRIEVE_WIDTH, _unit="flop")
    return out_rows, out_scores, out_obj


RETRIEVE_Q8_MAX_POOL = RETRIEVE_MAX_DEEP  # the longest shortlist of retrieve_q8_topk and list of retrieve_rescore


def quantize_catalogue_q8(items):
    """A bf16 [N, 128] catalogue as e4m3 codes with one power-of-two scale per row
    (lthm_catalogue_quantize_q8, csrc/retrieve.hip retr_q8_quant_k).

    With a the largest magnitude of a row, e is the largest integer with a 2^e <= 448 (0 for a zero row,
    clamped to [-64, 64]), the codes are (x.float() * 2.0**e).to(torch.float8_e4m3fn) and the scale is
    2^-e, bit for bit.  Returns (codes uint8 [N, 128], scale f32 [N]).  A row with a non-finite element
    gets unspecified codes."""
    who = "quantize_catalogue_q8"
    require_gpu(items)
    _check(items.dim() == 2 and items.shape[1] == RETRIEVE_WIDTH and items.dtype == torch.bfloat16,
           f"{who} takes a bf16 [N, {RETRIEVE_WIDTH}] catalogue (got {items.dtype} {tuple(items.shape)})")
    _check(items.is_contiguous(), f"{who} takes a contiguous catalogue")
    N = items.shape[0]
    _check(N >= 1, f"{who} takes a non-empty catalogue (N={N})")
    codes = torch.empty((N, RETRIEVE_WIDTH), dtype=torch.uint8, device=items.device)
    scale = torch.empty(N, dtype=torch.float32, device=items.device)
    call("lthm_catalogue_quantize_q8", ptr(items), N, ptr(codes), ptr(scale), stream(), _key="retr_q8_quant_k",
         _bytes=float(N * (RETRIEVE_WIDTH * 3 + 4)))
    return codes, scale


def retrieve_q8_topk(q, codes, scale, pool: int, *, normalize_q: bool = True, exclude_rows=None, slab_rows: int = 0):
    """The shortlist of an e4m3 catalogue: the `pool` first rows per query under (approximate score
    descending, row ascending) (lthm_retrieve_q8_topk, csrc/retrieve.hip retr_q8_topk_k).

    q f32 / bf16 [Q, 128]; codes uint8 [N, 128] and scale f32 [N] from quantize_catalogue_q8; pool in
    1..1024.  The query becomes the bf16 row retrieve_topk forms (normalize_q as there), is quantised by
    the catalogue's rule, and the score of row j is acc * (scale_q * scale_j) with acc the f32 sum of the
    128 code products.  exclude_rows int32 [Q, X] follows retrieve_topk's rules.  Returns (scores f32
    [Q, pool], rows int32 [Q, pool]), padded with -inf / -1; a pure function of the inputs, whatever
    slab_rows (0, or a multiple of 64)."""
    import ctypes
    from ._lib import STRUCTS
    who = "retrieve_q8_topk"
    require_gpu(q, codes, scale, exclude_rows)
    _check(codes.dim() == 2 and codes.shape[1] == RETRIEVE_WIDTH and codes.dtype == torch.uint8,
           f"{who} takes uint8 [N, {RETRIEVE_WIDTH}] codes (got {codes.dtype} {tuple(codes.shape)})")
    N = codes.shape[0]
    _check(scale.dtype == torch.float32 and tuple(scale.shape) == (N,),
           f"{who} takes f32 [N] scales (got {scale.dtype} {tuple(scale.shape)}, N={N})")
    _check(codes.is_contiguous() and scale.is_contiguous(), f"{who} takes contiguous codes and scales")
    _check(q.dim() == 2 and q.shape[1] == RETRIEVE_WIDTH, f"{who} takes [Q, {RETRIEVE_WIDTH}] queries")
    Q, M = q.shape[0], int(pool)
    _check(1 <= M <= RETRIEVE_Q8_MAX_POOL, f"{who} takes a pool of 1..{RETRIEVE_Q8_MAX_POOL} rows (got {M})")
    _check(N >= 1 and Q >= 1, f"{who} takes a non-empty catalogue and at least one query (N={N}, Q={Q})")
    dev = q.device
    _check(codes.device == dev and scale.device == dev, "codes and scales must be on the queries' device")
    X = 0
    x = None
    if exclude_rows is not None:
        _check(exclude_rows.dtype == torch.int32 and exclude_rows.dim() == 2 and exclude_rows.shape[0] == Q,
               f"exclude_rows must be int32 [Q, X] (got {exclude_rows.dtype} {tuple(exclude_rows.shape)}, Q={Q})")
        X = exclude_rows.shape[1]
        _check(1 <= X <= RETRIEVE_MAX_EXCLUDE, f"exclude_rows takes 1..{RETRIEVE_MAX_EXCLUDE} rows per query (got {X})")
        _check(exclude_rows.is_contiguous(), "exclude_rows must be contiguous")
        _check(exclude_rows.device == dev, "exclude_rows must be on the queries' device")
        x = STRUCTS["lthm_retrieve_excl"]()
        x.rows, x.X = ptr(exclude_rows), X
    need = load().lthm_retrieve_q8_ws_bytes(Q, N, M, int(slab_rows), X)
    _check(need >= 0, f"{who}: slab_rows={slab_rows} is not 0 or a multiple of {RETRIEVE_MIN_SLAB_ROWS} "
                      f"that cuts N={N} into at most 65535 slabs")
    scores = torch.empty((Q, M), dtype=torch.float32, device=dev)
    rows = torch.empty((Q, M), dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call("lthm_retrieve_q8_topk", ptr(codes), ptr(scale), N, ptr(q), dcode(q), int(bool(normalize_q)), Q, M,
         int(slab_rows), ctypes.addressof(x) if x is not None else None, ptr(scores), ptr(rows), ptr(ws), need, stream(),
         _key="retr_q8_topk_k", _work=2.0 * Q * N * RETRIEVE_WIDTH, _unit="flop",
         _bytes=float(N * (RETRIEVE_WIDTH + 4) + q.numel() * q.element_size() + Q * M * 8) + 4.0 * Q * X)
    return scores, rows


def retrieve_rescore(q, items, rows, k: int, *, normalize_q: bool = True):
    """Exact scores for a list of rows per query, and the k first of them (lthm_retrieve_rescore,
    csrc/retrieve.hip retr_rescore_k).

    q f32 / bf16 [Q, 128]; items bf16 [N, 128]; rows int32 [Q, M], 1 <= M <= 1024, in any order; k in
    1..M.  Every entry in [0, N) gets the f32 bits retrieve_topk returns for that (query, row); an entry
    outside is no candidate; a row named twice appears twice.  Returns (scores f32 [Q, k], rows int32
    [Q, k]) under (score descending, row ascending), padded with -inf / -1."""
    who = "retrieve_rescore"
    require_gpu(q, items, rows)
    _check(items.dim() == 2 and items.shape[1] == RETRIEVE_WIDTH and items.dtype == torch.bfloat16,
           f"{who} takes a bf16 [N, {RETRIEVE_WIDTH}] catalogue (got {items.dtype} {tuple(items.shape)})")
    _check(q.dim() == 2 and q.shape[1] == RETRIEVE_WIDTH, f"{who} takes [Q, {RETRIEVE_WIDTH}] queries")
    Q, N, k = q.shape[0], items.shape[0], int(k)
    _check(rows.dim() == 2 and rows.dtype == torch.int32 and rows.shape[0] == Q,
           f"{who} takes int32 rows [Q, M] (got {rows.dtype} {tuple(rows.shape)}, Q={Q})")
    M = rows.shape[1]
    _check(1 <= M <= RETRIEVE_Q8_MAX_POOL, f"{who} takes lists of 1..{RETRIEVE_Q8_MAX_POOL} rows (got M={M})")
    _check(1 <= k <= M, f"{who} takes k in 1..M (got k={k}, M={M})")
    _check(N >= 1 and Q >= 1, f"{who} takes a non-empty catalogue and at least one query (N={N}, Q={Q})")
    _check(rows.is_contiguous(), "rows must be contiguous")
    dev = q.device
    _check(rows.device == dev and items.device == dev, "rows and the catalogue must be on the queries' device")
    need = load().lthm_retrieve_rescore_ws_bytes(Q, M, k)
    _check(need >= 0, f"{who}: no workspace size for Q={Q} M={M} k={k}")
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_rows = torch.empty((Q, k), dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call("lthm_retrieve_rescore", ptr(items), N, ptr(q), dcode(q), int(bool(normalize_q)), Q, ptr(rows), M, k,
         ptr(scores), ptr(out_rows), ptr(ws), need, stream(), _key="retr_rescore_k",
         _work=2.0 * Q * M * RETRIEVE_WIDTH, _unit="flop")
    return scores, out_rows


def retrieve_rescore_bias(q, items, rows, k: int, *, normalize_q: bool = True, bias=None, bias_weight=None, order_ids=None):
    """retrieve_rescore with a prior and an id order (lthm_retrieve_rescore_bias, csrc/retrieve.hip
    retr_rescore_k<true>): a listed row's score is fma(w[q], bias[row], dot), dot the bits retrieve_rescore
    returns, one explicit f32 fma as retrieve_topk does with a bias.

    bias f32 [N] or None; bias_weight None (1 for everyone), a number or f32 [Q], only with a bias;
    order_ids int64 [N] or None: with it the list comes out under (score descending, order_ids[row]
    ascending), the order of the clustered calls, whose rows do not ascend with their ids across lists.
    With neither a bias nor order_ids the call is retrieve_rescore, bit for bit.  Returns (scores f32
    [Q, k], rows int32 [Q, k]), padded with -inf / -1."""
    who = "retrieve_rescore_bias"
    require_gpu(q, items, rows, bias, order_ids)
    _check(items.dim() == 2 and items.shape[1] == RETRIEVE_WIDTH and items.dtype == torch.bfloat16,
           f"{who} takes a bf16 [N, {RETRIEVE_WIDTH}] catalogue (got {items.dtype} {tuple(items.shape)})")
    _check(q.dim() == 2 and q.shape[1] == RETRIEVE_WIDTH, f"{who} takes [Q, {RETRIEVE_WIDTH}] queries")
    Q, N, k = q.shape[0], items.shape[0], int(k)
    _check(rows.dim() == 2 and rows.dtype == torch.int32 and rows.shape[0] == Q,
           f"{who} takes int32 rows [Q, M] (got {rows.dtype} {tuple(rows.shape)}, Q={Q})")
    M = rows.shape[1]
    _check(1 <= M <= RETRIEVE_Q8_MAX_POOL, f"{who} takes lists of 1..{RETRIEVE_Q8_MAX_POOL} rows (got M={M})")
    _check(1 <= k <= M, f"{who} takes k in 1..M (got k={k}, M={M})")
    _check(N >= 1 and Q >= 1, f"{who} takes a non-empty catalogue and at least one query (N={N}, Q={Q})")
    _check(rows.is_contiguous(), "rows must be contiguous")
    dev = q.device
    _check(rows.device == dev and items.device == dev, "rows and the catalogue must be on the queries' device")
    b, bw = _retrieve_bias(who, bias, bias_weight, items, Q, "Q", dev)
    if order_ids is not None:
        _check(order_ids.dtype == torch.int64 and tuple(order_ids.shape) == (N,) and order_ids.is_contiguous(),
               f"order_ids must be contiguous int64 [N] (got {order_ids.dtype} {tuple(order_ids.shape)}, N={N})")
        _check(order_ids.device == items.device, "order_ids must be on the catalogue's device")
    need = load().lthm_retrieve_rescore_ws_bytes(Q, M, k)
    _check(need >= 0, f"{who}: no workspace size for Q={Q} M={M} k={k}")
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_rows = torch.empty((Q, k), dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call("lthm_retrieve_rescore_bias", ptr(items), N, ptr(q), dcode(q), int(bool(normalize_q)), Q, ptr(rows), M, k,
         ptr(bias), ptr(bw), ptr(order_ids), ptr(scores), ptr(out_rows), ptr(ws), need, stream(),
         _key="retr_rescore_bias_k", _work=2.0 * Q * M * RETRIEVE_WIDTH, _unit="flop")
    return scores, out_rows


def retrieve_ivf_q8_topk(q, codes, scale, row_ids, list_off, probes, pool: int, *, normalize_q: bool = True,
                         exclude_rows=None, tags=None, tag_filter=None, bias=None, bias_weight=None):
    """The shortlist of a clustered e4m3 catalogue: per query the `pool` first rows of the lists it probes
    under (approximate score descending, id ascending) (lthm_retrieve_ivf_q8_topk, csrc/retrieve.hip
    retr_ivf_q8_topk_k).

    q f32 / bf16 [Q, 128]; codes uint8 [N, 128] and scale f32 [N], quantize_catalogue_q8 of the
    list-major rows; row_ids int64 [N], list_off int64 [L + 1] and probes int32 [Q, P] as retrieve_ivf_topk
    takes them; pool in 1..1024.  The score of (query, row) is retrieve_q8_topk's, bit for bit; with a
    bias f32 [N] the ranked score is fma(w[q], bias[row], score) (bias_weight None, a number or f32 [Q]).
    exclude_rows int32 [Q, X] (clustered rows) and tags int32 [N] / tag_filter int32 [Q, 3] follow
    retrieve_ivf_topk: an ineligible row takes no slot.  Returns (scores f32 [Q, pool], rows int32
    [Q, pool]), the clustered rows, padded with -inf / -1; a pure function of the inputs.  Every (query,
    probe) pair holds 16 KiB of candidates in the workspace, so where one call would take more than
    RETRIEVE_IVF_DEEP_WS_BYTES the queries go through in consecutive chunks, each one call: a query's
    list does not depend on the other queries."""
    import ctypes
    from ._lib import STRUCTS
    who = "retrieve_ivf_q8_topk"
    require_gpu(q, codes, scale, row_ids, list_off, probes, exclude_rows, tags, tag_filter, bias)
    _check(codes.dim() == 2 and codes.shape[1] == RETRIEVE_WIDTH and codes.dtype == torch.uint8,
           f"{who} takes uint8 [N, {RETRIEVE_WIDTH}] codes (got {codes.dtype} {tuple(codes.shape)})")
    N = codes.shape[0]
    _check(scale.dtype == torch.float32 and tuple(scale.shape) == (N,),
           f"{who} takes f32 [N] scales (got {scale.dtype} {tuple(scale.shape)}, N={N})")
    _check(q.dim() == 2 and q.shape[1] == RETRIEVE_WIDTH, f"{who} takes [Q, {RETRIEVE_WIDTH}] queries (got {tuple(q.shape)})")
    Q, M = q.shape[0], int(pool)
    _check(1 <= M <= RETRIEVE_Q8_MAX_POOL, f"{who} takes a pool of 1..{RETRIEVE_Q8_MAX_POOL} rows (got {M})")
    _check(N >= 1 and Q >= 1, f"{who} takes a non-empty catalogue and at least one query (N={N}, Q={Q})")
    _check(row_ids.dtype == torch.int64 and tuple(row_ids.shape) == (N,),
           f"row_ids must be int64 [N], one id per catalogue row (got {row_ids.dtype} {tuple(row_ids.shape)}, N={N})")
    _check(list_off.dtype == torch.int64 and list_off.dim() == 1 and list_off.shape[0] >= 2,
           f"list_off must be int64 [L + 1], L >= 1 (got {list_off.dtype} {tuple(list_off.shape)})")
    L = list_off.shape[0] - 1
    _check(probes.dtype == torch.int32 and probes.dim() == 2 and probes.shape[0] == Q,
           f"probes must be int32 [Q, P] (got {probes.dtype} {tuple(probes.shape)}, Q={Q})")
    P = probes.shape[1]
    _check(1 <= P <= RETRIEVE_MAX_PROBE, f"{who} takes 1..{RETRIEVE_MAX_PROBE} probes per query (got P={P})")
    _check(codes.is_contiguous() and scale.is_contiguous() and row_ids.is_contiguous() and list_off.is_contiguous()
           and probes.is_contiguous(), "codes, scale, row_ids, list_off and probes must be contiguous")
    dev = q.device
    _check(all(t.device == dev for t in (codes, scale, row_ids, list_off, probes)),
           "codes, scale, row_ids, list_off and probes must be on the queries' device")
    X = 0
    if exclude_rows is not None:
        _check(exclude_rows.dtype == torch.int32 and exclude_rows.dim() == 2 and exclude_rows.shape[0] == Q,
               f"exclude_rows must be int32 [Q, X] (got {exclude_rows.dtype} {tuple(exclude_rows.shape)}, Q={Q})")
        X = exclude_rows.shape[1]
        _check(1 <= X <= RETRIEVE_MAX_EXCLUDE, f"exclude_rows takes 1..{RETRIEVE_MAX_EXCLUDE} rows per query (got {X})")
        _check(exclude_rows.is_contiguous(), "exclude_rows must be contiguous")
        _check(exclude_rows.device == dev, "exclude_rows must be on the queries' device")
    _retrieve_tags(who, tags, tag_filter, codes, Q, "Q")
    _, bw = _retrieve_bias(who, bias, bias_weight, codes, Q, "Q", dev)
    size = lambda n: load().lthm_retrieve_ivf_q8_ws_bytes(n, N, L, P, M, X)
    _check(size(Q) >= 0, f"{who}: no workspace size for Q={Q} N={N} L={L} P={P} pool={M} X={X} (Q P must stay below 2^31)")
    step = Q
    if size(Q) > RETRIEVE_IVF_DEEP_WS_BYTES:
        lo, hi = 1, Q  # the size ascends with the queries: the most queries that fit, by bisection
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if size(mid) <= RETRIEVE_IVF_DEEP_WS_BYTES else (lo, mid - 1)
        step = lo
    q = q.contiguous()
    scores = torch.empty((Q, M), dtype=torch.float32, device=dev)
    rows = torch.empty((Q, M), dtype=torch.int32, device=dev)
    ws = torch.empty(size(step), dtype=torch.uint8, device=dev)
    for q0 in range(0, Q, step):
        n = min(step, Q - q0)
        cut = lambda v: None if v is None else v[q0:q0 + n]  # a contiguous tensor's leading rows are contiguous
        x = t = b = None
        if exclude_rows is not None:
            x = STRUCTS["lthm_retrieve_excl"]()
            x.rows, x.X = ptr(cut(exclude_rows)), X
        if tags is not None:
            t = STRUCTS["lthm_retrieve_tags"]()
            t.tags, t.filter = ptr(tags), ptr(cut(tag_filter))
        if bias is not None:
            b = STRUCTS["lthm_retrieve_bias"]()
            b.bias, b.weight = ptr(bias), (ptr(cut(bw)) if bw is not None else None)
        parts = [ctypes.addressof(o) if o is not None else None for o in (x, t, b)]
        work = float(n * RETRIEVE_WIDTH * q.element_size() + 24.0 * P * n * M + 12.0 * n * M + 4.0 * n * (P + X))
        call("lthm_retrieve_ivf_q8_topk", ptr(codes), ptr(scale), N, ptr(row_ids), ptr(list_off), L, ptr(cut(q)), dcode(q),
             int(bool(normalize_q)), n, ptr(cut(probes)), P, M, *parts, ptr(cut(scores)), ptr(cut(rows)), ptr(ws),
             ws.numel(), stream(), _key="retr_ivf_q8_topk_k", _work=work, _unit="byte")
    return scores, rows


CATALOGUE_UPDATE_CHUNK = 256  # csrc/catalogue_update.hip CU_CHUNK (include/lthm.h LTHM_CATALOGUE_UPDATE_CHUNK)


def catalogue_update(ids, emb, list_off, dead, delta_ids, delta_emb, delta_off, *, tags=None, bias=None, groups=None,
                     delta_tags=None, delta_bias=None, delta_groups=None, n_out: Optional[int] = None):
    """A list-major catalogue without its dead rows and with the delta rows merged in, list by list
    (lthm_catalogue_update, csrc/catalogue_update.hip): the kernel of ``ItemCatalogue.update`` (L = 1) and
    ``ClusteredItemCatalogue.update``.

    ids int64 [N], emb bf16 [N, 128], list_off int64 [L + 1] and tags int32 [N] / bias f32 [N] / groups int32
    [N] (each or None): the old rows, the ids of a list ascending.  dead uint8 or bool [N]: the rows to drop.
    delta_ids int64 [M], delta_emb bf16 [M, 128], delta_off int64 [L + 1] and delta_tags / delta_bias /
    delta_groups [M], exactly the optional columns the old rows carry: the rows to merge in, in (list, id)
    order; no delta id equals a surviving id of its list.  M may be 0.  The offsets and the order are the
    caller's contract and are not read on the host; offsets that break it give wrong rows, no fault.

    Returns (ids, emb, list_off, tags, bias, groups) of the N' = N - dead + M output rows.  One device-to-host
    read, of N', sizes the outputs; nothing else synchronises, and a caller that has read N' already hands it
    in as ``n_out`` (it must be the true count) and the call reads nothing.  N' = 0 is refused.  No sort and
    no atomics: two calls give the same bytes."""
    import ctypes
    from ._lib import STRUCTS
    who = "catalogue_update"
    cols = (("tags", tags, delta_tags, torch.int32), ("bias", bias, delta_bias, torch.float32),
            ("groups", groups, delta_groups, torch.int32))
    require_gpu(ids, emb, list_off, dead, delta_ids, delta_emb, delta_off, *[t for _, a, b, _ in cols for t in (a, b)])
    _check(ids.dtype == torch.int64 and ids.dim() == 1 and ids.shape[0] >= 1,
           f"{who} takes int64 [N] ids, N >= 1 (got {ids.dtype} {tuple(ids.shape)})")
    N = ids.shape[0]
    _check(emb.dtype == torch.bfloat16 and tuple(emb.shape) == (N, RETRIEVE_WIDTH),
           f"{who} takes bf16 [N, {RETRIEVE_WIDTH}] rows (got {emb.dtype} {tuple(emb.shape)}, N={N})")
    _check(list_off.dtype == torch.int64 and list_off.dim() == 1 and list_off.shape[0] >= 2,
           f"{who} takes int64 [L + 1] list_off, L >= 1 (got {list_off.dtype} {tuple(list_off.shape)})")
    L = list_off.shape[0] - 1
    _check(dead.dtype in (torch.uint8, torch.bool) and tuple(dead.shape) == (N,),
           f"{who} takes a uint8 or bool [N] dead flag (got {dead.dtype} {tuple(dead.shape)}, N={N})")
    _check(delta_ids.dtype == torch.int64 and delta_ids.dim() == 1,
           f"{who} takes int64 [M] delta_ids (got {delta_ids.dtype} {tuple(delta_ids.shape)})")
    M = delta_ids.shape[0]
    _check(delta_emb.dtype == torch.bfloat16 and tuple(delta_emb.shape) == (M, RETRIEVE_WIDTH),
           f"{who} takes bf16 [M, {RETRIEVE_WIDTH}] delta rows (got {delta_emb.dtype} {tuple(delta_emb.shape)}, M={M})")
    _check(delta_off.dtype == torch.int64 and tuple(delta_off.shape) == (L + 1,),
           f"{who} takes int64 [L + 1] delta_off (got {delta_off.dtype} {tuple(delta_off.shape)}, L={L})")
    for name, old, new, dt in cols:
        _check((old is None) == (new is None), f"{who}: the old rows and the delta carry {name} together or not at all")
        _check(old is None or (old.dtype == dt and tuple(old.shape) == (N,)), f"{who} takes {dt} [N] {name}")
        _check(new is None or (new.dtype == dt and tuple(new.shape) == (M,)), f"{who} takes {dt} [M] delta_{name}")
    dev = ids.device
    _check(all(t is None or t.device == dev for t in (emb, list_off, dead, delta_ids, delta_emb, delta_off,
                                                      *[t for _, a, b, _ in cols for t in (a, b)])),
           f"{who} takes tensors of one device")
    _check(N + M <= 2 ** 31 - 2 and L <= 2 ** 30, f"{who} takes N + M <= 2^31 - 2 rows and L <= 2^30 lists")
    _check(emb.data_ptr() % 16 == 0 and delta_emb.data_ptr() % 16 == 0, f"{who} takes 16-byte aligned rows")
    n_out = int((dead == 0).sum()) + M if n_out is None else int(n_out)  # the one device-to-host read
    _check(M <= n_out <= N + M, f"{who}: n_out must lie in M..N + M (got {n_out}, N={N}, M={M})")
    _check(n_out >= 1, f"{who}: no row remains, and a catalogue is never empty")
    out_ids = torch.empty(n_out, dtype=torch.int64, device=dev)
    out_emb = torch.empty((n_out, RETRIEVE_WIDTH), dtype=torch.bfloat16, device=dev)
    out_off = torch.empty(L + 1, dtype=torch.int64, device=dev)
    outs = [None if old is None else torch.empty(n_out, dtype=dt, device=dev) for _, old, _, dt in cols]
    need = load().lthm_catalogue_update_ws_bytes(N, M, L)
    _check(need > 0, f"{who} refuses M={M}, L={L}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    dead8 = dead.view(torch.uint8) if dead.dtype == torch.bool else dead
    d = STRUCTS["lthm_catalogue_update_desc"]()
    d.N, d.M, d.L, d.N_out = N, M, L, n_out
    d.old_ids, d.old_emb, d.old_off, d.dead = ptr(ids), ptr(emb), ptr(list_off), ptr(dead8)
    d.old_tags, d.old_bias, d.old_groups = ptr(tags), ptr(bias), ptr(groups)
    d.delta_ids, d.delta_emb, d.delta_off = ptr(delta_ids), ptr(delta_emb), ptr(delta_off)
    d.delta_tags, d.delta_bias, d.delta_groups = ptr(delta_tags), ptr(delta_bias), ptr(delta_groups)
    d.out_ids, d.out_emb, d.out_off = ptr(out_ids), ptr(out_emb), ptr(out_off)
    d.out_tags, d.out_bias, d.out_groups = ptr(outs[0]), ptr(outs[1]), ptr(outs[2])
    d.workspace, d.ws_bytes = ptr(ws), need
    row = RETRIEVE_WIDTH * 2 + 8 + 4 * sum(o is not None for o in outs)
    call("lthm_catalogue_update", ctypes.addressof(d), stream(), _key="cat_upd_merge_k", _bytes=2.0 * n_out * row)
    return out_ids, out_emb, out_off, outs[0], outs[1], outs[2]


# ----------------------------------------------------------------- ranking stage (csrc/rank.hip)
RANK_MAX_LIST = RETRIEVE_MAX_DEEP  # LTHM_RANK_MAX_LIST: the longest candidate list, a deep retrieval list


def rank_assemble(user_dense, user_cat, item_dense, item_cat, rows):
    """The ranker's input batch of Q users x M candidates each (lthm_rank_assemble, csrc/rank.hip).

    user_dense f32 [Q, Du], user_cat int64 [Q, Fu], item_dense f32 [N, Di], item_cat int64 [N, Fi], rows
    int32 [Q, M] with M in 1..RANK_MAX_LIST; any width may be 0.  Returns (dense f32 [Q M, Du + Di], cat
    int64 [Q M, Fu + Fi]): row q M + m holds user q's columns, then the item columns of rows[q, m].  A row
    index outside [0, N) is a pad: it is never followed and its item columns are 0.0 and 0.  Exact copies,
    every element written once, no atomics; odd widths move element by element instead of in 16-byte
    units."""
    import ctypes
    from ._lib import STRUCTS
    who = "rank_assemble"
    require_gpu(user_dense, user_cat, item_dense, item_cat, rows)
    _check(rows.dtype == torch.int32 and rows.dim() == 2, f"{who} takes int32 [Q, M] rows (got {rows.dtype} {tuple(rows.shape)})")
    Q, M = rows.shape
    _check(Q >= 1 and 1 <= M <= RANK_MAX_LIST, f"{who} takes Q >= 1 lists of 1..{RANK_MAX_LIST} rows (got Q={Q}, M={M})")
    _check(Q * M <= 2 ** 31 - 1, f"{who} takes Q M <= 2^31 - 1 rows (got {Q * M})")
    _check(user_dense.dtype == torch.float32 and user_dense.dim() == 2 and user_dense.shape[0] == Q,
           f"{who} takes f32 [Q, Du] user_dense (got {user_dense.dtype} {tuple(user_dense.shape)}, Q={Q})")
    _check(user_cat.dtype == torch.int64 and user_cat.dim() == 2 and user_cat.shape[0] == Q,
           f"{who} takes int64 [Q, Fu] user_cat (got {user_cat.dtype} {tuple(user_cat.shape)}, Q={Q})")
    _check(item_dense.dtype == torch.float32 and item_dense.dim() == 2,
           f"{who} takes f32 [N, Di] item_dense (got {item_dense.dtype} {tuple(item_dense.shape)})")
    N = item_dense.shape[0]
    _check(item_cat.dtype == torch.int64 and item_cat.dim() == 2 and item_cat.shape[0] == N,
           f"{who} takes int64 [N, Fi] item_cat (got {item_cat.dtype} {tuple(item_cat.shape)}, N={N})")
    _check(N <= 2 ** 31 - 1, f"{who} takes N <= 2^31 - 1 item rows (got {N})")
    dev = rows.device
    _check(all(t.device == dev for t in (user_dense, user_cat, item_dense, item_cat)), f"{who} takes tensors of one device")
    Du, Di, Fu, Fi = user_dense.shape[1], item_dense.shape[1], user_cat.shape[1], item_cat.shape[1]
    _check(Du + Di <= 2 ** 20 and Fu + Fi <= 2 ** 20, f"{who} takes rows of at most 2^20 columns")
    # 16-byte units where both widths of a matrix allow them (a row slice of such a matrix stays aligned)
    da = 16 if Du % 4 == 0 and Di % 4 == 0 else 4
    ca = 16 if Fu % 2 == 0 and Fi % 2 == 0 else 8
    _check(user_dense.data_ptr() % da == 0 and item_dense.data_ptr() % da == 0,
           f"{who} takes {da}-byte aligned dense matrices of these widths")
    _check(user_cat.data_ptr() % ca == 0 and item_cat.data_ptr() % ca == 0,
           f"{who} takes {ca}-byte aligned categorical matrices of these widths")
    dense = torch.empty((Q * M, Du + Di), dtype=torch.float32, device=dev)
    cat = torch.empty((Q * M, Fu + Fi), dtype=torch.int64, device=dev)
    d = STRUCTS["lthm_rank_assemble_desc"]()
    d.Q, d.M, d.N, d.Du, d.Di, d.Fu, d.Fi = Q, M, N, Du, Di, Fu, Fi
    d.user_dense, d.user_cat, d.item_dense, d.item_cat = ptr(user_dense), ptr(user_cat), ptr(item_dense), ptr(item_cat)
    d.rows, d.out_dense, d.out_cat = ptr(rows), ptr(dense), ptr(cat)
    row = 4 * (Du + Di) + 8 * (Fu + Fi)
    call("lthm_rank_assemble", ctypes.addressof(d), stream(), _key="rank_assemble_k", _bytes=2.0 * Q * M * row + 4.0 * Q * M)
    return dense, cat


def rank_sort(logits, rows, k: int):
    """Every list's first k entries in the order (logit descending, row ascending, position ascending)
    (lthm_rank_sort, csrc/rank.hip).

    logits f32 [Q, M], rows int32 [Q, M], 1 <= k <= M <= RANK_MAX_LIST.  An entry is a candidate when its
    row is >= 0 and its logit is not NaN; +-inf are ordinary values and -0.0 orders as +0.0.  Returns
    (scores f32 [Q, k], rows int32 [Q, k], src int32 [Q, k]), src the position the entry had in its list;
    the slots behind the last candidate hold (-inf, -1, -1).  A pure function of the inputs: no atomics,
    no workspace."""
    who = "rank_sort"
    require_gpu(logits, rows)
    _check(logits.dtype == torch.float32 and logits.dim() == 2,
           f"{who} takes f32 [Q, M] logits (got {logits.dtype} {tuple(logits.shape)})")
    Q, M = logits.shape
    _check(rows.dtype == torch.int32 and tuple(rows.shape) == (Q, M),
           f"{who} takes int32 [Q, M] rows (got {rows.dtype} {tuple(rows.shape)}, Q={Q}, M={M})")
    _check(Q >= 1 and 1 <= M <= RANK_MAX_LIST, f"{who} takes Q >= 1 lists of 1..{RANK_MAX_LIST} entries (got Q={Q}, M={M})")
    _check(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= M, f"{who} takes k in 1..M (got k={k!r}, M={M})")
    _check(rows.device == logits.device, f"{who} takes tensors of one device")
    dev = logits.device
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_rows = torch.empty((Q, k), dtype=torch.int32, device=dev)
    src = torch.empty((Q, k), dtype=torch.int32, device=dev)
    call("lthm_rank_sort", ptr(logits), ptr(rows), Q, M, k, ptr(scores), ptr(out_rows), ptr(src), stream(),
         _key="rank_sort_k", _bytes=8.0 * Q * M + 12.0 * Q * k)
    return scores, out_rows, src
