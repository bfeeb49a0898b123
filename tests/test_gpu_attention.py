"""GPU parity of the attention kernels (recommendations_amd/csrc/attention.hip), row by row,
against the fp64 references of tests/attention_case.py.

Every bound comes from the references alone (attention_case.bounds, pinned on the CPU by
tests/test_attention_host.py): for out, dq, dk and dv the worst row of the kernel must stay
under 4 x the worst row of the bf16 rounding model, the same per table row for dtable, and lse
within 8 x the error of its float32 evaluation on the CPU.  A failure names the worst
(b, h, t).  DESIGN.md (attention, "per-row parity") lists the model maxima next to the values
achieved.
"""
import ctypes

import numpy as np
import pytest
import torch

import attention_case as C
from parity import check

pytestmark = pytest.mark.gpu


def _rows(x, dev):
    """[B, H', T, E] -> bf16 [B T, H' E] on the device"""
    B, H, T, E = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * E).to(torch.bfloat16).to(dev)


def _heads(x, B, T, H, E):
    """[B T, H E] -> f64 [B, H, T, E] on the CPU"""
    return x.detach().double().cpu().view(B, T, H, E).permute(0, 2, 1, 3)


def _mask_operand(K, c, dev):
    return K.attn_mask_operand(c.mask.to(dev), c.B, c.H, c.T, c.E) if c.mask is not None else None


def _run(dev, c, backward=True):
    """forward (and backward) through kernels.attn_fwd_qkv / attn_fwd_mqa / attn_bwd_qkv"""
    from recommendations_amd import kernels as K
    B, T, H, E = c.B, c.T, c.H, c.E
    C_ = H * E
    tab = c.table.to(dev) if c.table is not None else None
    mop = _mask_operand(K, c, dev)
    q, k, v = _rows(c.q, dev), _rows(c.k, dev), _rows(c.v, dev)
    if c.mqa:
        out, lse = K.attn_fwd_mqa(q, torch.cat([k, v], 1).contiguous(), B, T, H, E, tab, c.causal, mop)
        # the layer's backward: the multi-head kernel on K / V expanded per head
        qkv = torch.cat([q, k.repeat(1, H), v.repeat(1, H)], 1).contiguous()
    else:
        qkv = torch.cat([q, k, v], 1).contiguous()
        out, lse = K.attn_fwd_qkv(qkv, B, T, H, E, tab, c.causal, mop)
    got = {"out": _heads(out, B, T, H, E), "lse": lse.double().cpu()}
    if backward:
        dqkv, dtab = K.attn_bwd_qkv(qkv, out, _rows(c.dout, dev), lse, B, T, H, E, tab, c.causal, mop)
        for i, n in enumerate(("dq", "dk", "dv")):
            got[n] = _heads(dqkv[:, i * C_:(i + 1) * C_], B, T, H, E)
        if c.mqa:  # ... and their f32 sums over the heads
            got["dk"], got["dv"] = got["dk"].sum(1, keepdim=True), got["dv"].sum(1, keepdim=True)
        if dtab is not None:
            got["dtable"] = dtab.double().cpu()
    return got


def _check(b, got, names=None, tag=""):
    """every tensor of `got` against the reference of b (attention_case.bounds) by the rules above"""
    sid = tag + C.spec_id(b.spec)
    for n in names or got:
        g, w = got[n], getattr(b.ref, n)
        assert g.shape == w.shape, (n, g.shape, w.shape)
        assert bool(torch.isfinite(g).all()), f"{sid} {n}: not finite"
        if n == "lse":
            err = (g - w).abs()
            i = int(torch.argmax(err))
            check(f"{sid} lse max abs, worst at {tuple(int(x) for x in np.unravel_index(i, tuple(err.shape)))}",
                  float(err.max()), b.bound["lse"])
        elif n in b.zero:  # an all-zero reference (T = 1): absolute, attention_case.zero_bound
            check(f"{sid} {n} max abs (reference 0)", float(g.abs().max()), C.zero_bound(b.case)[n])
        else:
            mx, at = C.worst(C.row_err(g, w))
            print(f"{sid} {n}: row error {mx:.3e} at {at}, model {b.model_max[n]:.3e}, bound {b.bound[n]:.3e}")
            check(f"{sid} {n} row error, worst at {at}", mx, b.bound[n])


# ------------------------------------------------------------------ a. one case per dispatcher branch
@pytest.mark.parametrize("spec", C.MATRIX, ids=C.spec_id)
def test_attention_rows_vs_fp64(dev, spec):
    b = C.bounds(spec)
    _check(b, _run(dev, b.case))


# ------------------------------------------------------------------ b. general additive masks
@pytest.mark.parametrize("spec", C.MASKS, ids=C.spec_id)
def test_attention_masked_rows_vs_fp64(dev, spec):
    """attn_fwd_k / attn_bwd_k with every mask layout (batch and head strides 0 or not), NK = 1 .. 4
    and every E; (2, 149, 1, 128) is the largest E = 128 shape the masked backward holds"""
    b = C.bounds(spec)
    _check(b, _run(dev, b.case))


def test_attention_mask_limit_is_refused_up_front(dev):
    """The masked backward keeps Q, K, V and dO of one head in LDS: T (8 E + 72) + 16 bytes of
    160 KiB, so E = 128 stops at T = 149 (E <= 64 reaches T = 256).  Past it the mask operand and
    the forward itself refuse with the limit in the message, before anything is launched."""
    from recommendations_amd import kernels as K
    from recommendations_amd._lib import load
    lib = load()
    assert lib.lthm_attn_mask_ok(149, 128) == 1 and lib.lthm_attn_mask_ok(150, 128) == 0
    assert all(lib.lthm_attn_mask_ok(256, E) == 1 for E in (16, 32, 64)) and lib.lthm_attn_mask_ok(257, 64) == 0
    assert K.attn_mask_operand(torch.zeros(149, 149, device=dev), 1, 1, 149, 128) is not None
    for B, T, H, E in C.MASK_REFUSED:
        mask = torch.zeros(T, T, device=dev)
        with pytest.raises(K.OperandError, match=r"T <= 149 with E = 128"):
            K.attn_mask_operand(mask, B, H, T, E)
        # a caller that built the operand without E is stopped by the forward, with `out` untouched
        mop = K.attn_mask_operand(mask, B, H, T)
        qkv = torch.zeros(B * T, 3 * H * E, dtype=torch.bfloat16, device=dev)
        with pytest.raises(K.OperandError, match=r"T <= 149 with E = 128"):
            K.attn_fwd_qkv(qkv, B, T, H, E, None, True, mop)
        with pytest.raises(K.OperandError, match=r"T <= 149 with E = 128"):
            K.attn_fwd_mqa(qkv[:, : H * E].contiguous(), qkv[:, : 2 * E].contiguous(), B, T, H, E, None, True, mop)


# ------------------------------------------------------------------ c. multi-query forward
@pytest.mark.parametrize("spec", C.MQA, ids=C.spec_id)
def test_attention_mqa_rows_vs_fp64(dev, spec):
    """attn_fwd_mqa: K / V head stride 0 and token stride 2E through each forward kernel; the first
    two shapes also through the layer's expand-and-sum backward (dq, head-summed dk / dv)"""
    b = C.bounds(spec)
    bwd = spec in C.MQA_BACKWARD
    got = _run(dev, b.case, backward=bwd)
    _check(b, got, names=("out", "lse") + (("dq", "dk", "dv", "dtable") if bwd else ()))


# ------------------------------------------------------------------ d. softmax range
@pytest.mark.parametrize("spec", C.RANGE, ids=C.spec_id)
def test_attention_softmax_range(dev, spec):
    """max |score| in [100, 200] (asserted on the reference): exp without the running maximum
    overflows f32 at 88.  out and lse by the per-row rules; the gradients of a near one-hot
    softmax are ill-conditioned per row, so max |got - want| <= 4 max |model - want| per tensor."""
    b = C.bounds(spec)
    S = C.scores(b.case, torch.float64)
    smax = float(S[torch.isfinite(S)].abs().max())
    assert 100.0 <= smax <= 200.0, smax
    got = _run(dev, b.case)
    _check(b, got, names=("out", "lse"))
    sid = C.spec_id(spec)
    for n in ("dq", "dk", "dv", "dtable"):
        assert bool(torch.isfinite(got[n]).all()), f"{sid} {n}: not finite"
        check(f"{sid} {n} max abs", float((got[n] - getattr(b.ref, n)).abs().max()), 4.0 * b.model_abs[n])


# ------------------------------------------------------------------ e. guard rows
GUARD_ROWS = 32      # rows of out / dqkv on each side
GUARD_FLOATS = 64    # floats of lse / dtable_part on each side
SENT_BF16 = 24576.0  # finite, a bf16 value, far from anything the kernels produce
SENT_F32 = -12345.5


def _guarded(dev, inner, dtype, pad, sentinel):
    """(whole buffer, its middle slice of `inner` elements): pad elements of sentinel on each side"""
    whole = torch.full((pad + inner + pad,), sentinel, dtype=dtype, device=dev)
    return whole, whole[pad:pad + inner]


def _guards_intact(whole, pad, sentinel, what):
    want = torch.full((pad,), sentinel, dtype=whole.dtype, device=whole.device)
    bits = torch.int16 if whole.dtype == torch.bfloat16 else torch.int32
    for side, g in (("below", whole[:pad]), ("above", whole[-pad:])):
        assert torch.equal(g.view(bits), want.view(bits)), f"{what}: written {side} its rows"


@pytest.mark.parametrize("spec", C.GUARD, ids=C.spec_id)
def test_attention_writes_only_its_rows(dev, spec):
    """lthm_attn_fwd / lthm_attn_bwd with out, lse, dqkv and dtable_part as the middle of larger
    buffers filled with a sentinel: the guards stay bit-identical, nothing inside keeps the
    sentinel (all lthm_attn_bwd_parts partials are written), and each of dq / dk / dv meets its
    per-row bound, so the three column blocks of dqkv do not leak into each other."""
    from recommendations_amd import kernels as K
    from recommendations_amd._lib import load
    b = C.bounds(spec)
    c = b.case
    B, T, H, E = c.B, c.T, c.H, c.E
    C_ = H * E
    tab = c.table.to(dev)
    mop = _mask_operand(K, c, dev)
    qkv = torch.cat([_rows(c.q, dev), _rows(c.k, dev), _rows(c.v, dev)], 1).contiguous()
    dout = _rows(c.dout, dev)
    parts = int(load().lthm_attn_bwd_parts(B, T))
    out_w, out = _guarded(dev, B * T * C_, torch.bfloat16, GUARD_ROWS * C_, SENT_BF16)
    lse_w, lse = _guarded(dev, B * H * T, torch.float32, GUARD_FLOATS, SENT_F32)
    dqkv_w, dqkv = _guarded(dev, B * T * 3 * C_, torch.bfloat16, GUARD_ROWS * 3 * C_, SENT_BF16)
    part_w, part = _guarded(dev, parts * (2 * T + 1) * H, torch.float32, GUARD_FLOATS, SENT_F32)
    out, dqkv = out.view(B * T, C_), dqkv.view(B * T, 3 * C_)
    assert all(t.data_ptr() % 16 == 0 for t in (out, lse, dqkv, part))
    delta = torch.empty(B * H * T, dtype=torch.float32, device=dev) if T > 256 else None

    d = K._attn_desc(qkv, qkv[:, C_:], qkv[:, 2 * C_:], B, T, H, E, out, lse, tab, c.causal, 3 * C_, 3 * C_, E, mop)
    K.call("lthm_attn_fwd", ctypes.addressof(d), K.stream())
    d.dout, d.dq, d.dk, d.dv = K.ptr(dout), K.ptr(dqkv), K.ptr(dqkv[:, C_:]), K.ptr(dqkv[:, 2 * C_:])
    d.dtable_part, d.delta = K.ptr(part), K.ptr(delta)
    K.call("lthm_attn_bwd", ctypes.addressof(d), K.stream())
    torch.cuda.synchronize()

    _guards_intact(out_w, GUARD_ROWS * C_, SENT_BF16, "out")
    _guards_intact(lse_w, GUARD_FLOATS, SENT_F32, "lse")
    _guards_intact(dqkv_w, GUARD_ROWS * 3 * C_, SENT_BF16, "dqkv")
    _guards_intact(part_w, GUARD_FLOATS, SENT_F32, "dtable_part")
    for t, s, what in ((out, SENT_BF16, "out"), (lse, SENT_F32, "lse"), (dqkv, SENT_BF16, "dqkv"),
                       (part, SENT_F32, "dtable_part")):
        assert not bool((t == s).any()), f"{what}: an element was never written"
    got = {"out": _heads(out, B, T, H, E), "lse": lse.double().cpu().view(B, H, T),
           "dtable": part.double().cpu().view(parts, 2 * T + 1, H).sum(0)}
    for i, n in enumerate(("dq", "dk", "dv")):
        got[n] = _heads(dqkv[:, i * C_:(i + 1) * C_], B, T, H, E)
    _check(b, got, tag="guarded ")
