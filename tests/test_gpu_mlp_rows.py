"""Every kernel of the fused encoder MLP (csrc/mlp.hip) against the fp64 references and the
per-element bounds of tests/mlp_case.py (derived in DESIGN.md section 19, pinned on the CPU by
tests/test_mlp_host.py).  The geometry comes from kernels.mlp_plan with the device's CU count; a
test that names a path (several tiles per workgroup, a ring shorter than its slots, FULL slices)
asserts from the plan that it reached it.  The largest error / bound of every check is recorded
by tests/parity.py."""
import pytest
import torch

import mlp_case as C
from parity import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _d(t, dev, dtype=None):
    if t is None:
        return None
    return t.to(dev, dtype) if dtype is not None else t.to(dev)


def _ops(c, dev):
    b = torch.bfloat16
    return _d(c.x, dev, b), _d(c.dy, dev, b), _d(c.W1, dev, b), _d(c.b1, dev), _d(c.W2T, dev, b), _d(c.b2, dev)


def _ids(specs):
    return ["-".join(str(int(v)) for v in s) for s in specs]


N_FWD = len(C.fwd_specs(256))


@pytest.mark.parametrize("i", range(N_FWD))
def test_fwd_rows(dev, cus, i):
    """lthm_mlp_fwd, every output element"""
    from recommendations_amd import kernels as K
    spec = C.fwd_specs(cus)[i]
    c = C.make_case(spec)
    plan = K.mlp_plan("fwd", spec.M, spec.D, spec.HID)
    if spec.M == cus * 296:
        assert plan.grid == cus and plan.max_tiles == 2  # a full tile, then 40 rows: 2 waves, 6 idle
    x, _, w1, b1, w2t, b2 = _ops(c, dev)
    out = K.mlp_fwd(x, w1, b1, w2t, b2, *[_d(r, dev) for r in c.res])
    torch.cuda.synchronize()
    assert tuple(out.shape) == (spec.M, spec.D)
    hid = C.hidden(c)
    ref, e = C.fwd(c, hid=hid)
    check(f"mlp fwd {tuple(spec)} share {C.flagged_share(hid):.4f}", C.ratio(out.cpu(), ref, e), 1.0)


def _ln_cases(cus):
    """(spec, ln_b present): row edges, bias none, the rows-by-CU case (a full tile, then a ragged
    one), the largest HID and M = 0"""
    return [(C.Spec(33, 128, 32, True, 1), True), (C.Spec(257, 256, 96, True, 2), False),
            (C.Spec(1000, 128, 1024, True, 1), True), (C.Spec(255, 256, 64, True, 0), True),
            (C.Spec(1, 256, 128, True, 1), False), (C.Spec(257, 128, 96, False, 1), True),
            (C.Spec(256, 256, 64, False, 2), False), (C.Spec(cus * 296, 256, 64, True, 1), True),
            (C.Spec(cus * 296, 128, 96, True, 1), False), (C.Spec(33, 256, 7424, True, 1, 231), True),
            (C.Spec(33, 128, 8192, True, 1, 255), False), (C.Spec(0, 256, 64, True, 1), True)]


@pytest.mark.parametrize("i", range(len(_ln_cases(256))))
def test_fwd_ln_rows(dev, cus, i):
    """lthm_mlp_fwd_ln: mean, rstd and h against the LayerNorm bounds; out against the MLP reference
    on the RETURNED h (the operand the kernel used); save=False gives the same out bit for bit"""
    from recommendations_amd import kernels as K
    spec, with_b = _ln_cases(cus)[i]
    c = C.make_case(spec)
    plan = K.mlp_plan("fwd_ln", spec.M, spec.D, spec.HID)
    if spec.M == cus * 296:
        assert plan.grid == cus and plan.max_tiles == 2
    x32, lw, lb = C.ln_inputs(spec.M, spec.D, with_b)
    _, _, w1, b1, w2t, b2 = _ops(c, dev)
    res = [_d(r, dev) for r in c.res]
    out, h, mu, rs = K.mlp_fwd_ln(_d(x32, dev), _d(lw, dev), _d(lb, dev), w1, b1, w2t, b2, *res)
    out2, h2, mu2, rs2 = K.mlp_fwd_ln(_d(x32, dev), _d(lw, dev), _d(lb, dev), w1, b1, w2t, b2, *res, save=False)
    torch.cuda.synchronize()
    assert h2 is None and mu2 is None and rs2 is None and torch.equal(out, out2)
    r = C.ln(x32, lw, lb)
    check(f"mlp fwd_ln mean {tuple(spec)}", C.ratio(mu.cpu(), r.mean, r.e_mean), 1.0)
    check(f"mlp fwd_ln rstd {tuple(spec)}", C.ratio(rs.cpu(), r.rstd, r.e_rstd), 1.0)
    check(f"mlp fwd_ln h {tuple(spec)}", C.ratio(h.cpu(), r.y, r.e_h), 1.0)
    ref, e = C.fwd(c, x=h.float().cpu())
    check(f"mlp fwd_ln out {tuple(spec)}", C.ratio(out.cpu(), ref, e), 1.0)


def _bwd_case(dev, cus, spec, fused, monkeypatch):
    from recommendations_amd import kernels as K
    c = C.make_case(spec)
    hid = C.hidden(c, backward=True)
    x, dy, w1, b1, w2t, _ = _ops(c, dev)
    monkeypatch.setattr(K, "_MLP_BWD_SPLIT", not fused)
    one_kernel = fused or spec.HID > 4096
    plan = K.mlp_plan("bwd" if one_kernel else "bwd_hidden", spec.M, spec.D, spec.HID)
    if spec.M >= cus * 128:
        assert plan.grid == cus and plan.max_tiles == 2
    outs = {}
    for dt in (torch.float32, torch.bfloat16):
        dx, G, dP = K.mlp_bwd(x, dy, w1, b1, w2t, dx_dtype=dt)
        torch.cuda.synchronize()
        tag = f"{'fused' if one_kernel else 'split'} {tuple(spec)} {str(dt)[6:]}"
        check(f"mlp bwd G {tag} share {C.flagged_share(hid):.4f}", C.hidden_ratio(G.float().cpu(), hid.hb, hid.sg),
              C.HIDDEN_OK)
        check(f"mlp bwd dP {tag}", C.hidden_ratio(dP.float().cpu(), hid.dpb, hid.sd), C.HIDDEN_OK)
        ref, e = C.dx(c, hid, dt == torch.bfloat16)
        check(f"mlp bwd dX vs fp64 {tag}", C.ratio(dx.float().cpu(), ref, e), 1.0)
        ref2, e2 = C.dx_from_dp(c, dP.float().cpu(), dt == torch.bfloat16)
        check(f"mlp bwd dX vs returned dP {tag}", C.ratio(dx.float().cpu(), ref2, e2), 1.0)
        outs[dt] = (G, dP)
    assert torch.equal(outs[torch.float32][0], outs[torch.bfloat16][0])
    assert torch.equal(outs[torch.float32][1], outs[torch.bfloat16][1])
    return outs[torch.float32]


N_BWD = len(C.bwd_specs(256, False))


@pytest.mark.parametrize("i", range(N_BWD))
def test_bwd_rows_both_forms(dev, cus, i, monkeypatch):
    """lthm_mlp_bwd_hidden + the dX GEMM, and lthm_mlp_bwd: G, dP, dX (f32 and bf16) per element.
    Where both forms take the same rows, their G and dP agree off the flagged elements."""
    split = C.bwd_specs(cus, False)[i]
    fused = C.bwd_specs(cus, True)[i]
    Gs, Ps = _bwd_case(dev, cus, split, False, monkeypatch)
    Gf, Pf = _bwd_case(dev, cus, fused, True, monkeypatch)
    if split == fused:
        hid = C.hidden(C.make_case(split), backward=True)
        assert torch.equal(Gs.cpu()[hid.sg == 0], Gf.cpu()[hid.sg == 0])
        assert torch.equal(Ps.cpu()[hid.sd == 0], Pf.cpu()[hid.sd == 0])


N_DX = len(C.bwd_dx_specs(256))


@pytest.mark.parametrize("i", range(N_DX))
def test_bwd_dx_rows(dev, cus, i):
    """lthm_mlp_bwd_dx at 1 .. 5 hidden chunks against its 4-slot ring, one and two tiles per workgroup"""
    from recommendations_amd import kernels as K
    spec = C.bwd_dx_specs(cus)[i]
    c = C.make_case(spec)
    plan = K.mlp_plan("bwd_dx", spec.M, spec.D, spec.HID)
    if spec.M == cus * 168:
        assert plan.grid == cus and plan.max_tiles == 2
    hid = C.hidden(c, backward=True)
    x, dy, w1, b1, w2t, _ = _ops(c, dev)
    for dt in (torch.float32, torch.bfloat16):
        dx = K.mlp_bwd_dx(x, dy, w1, b1, w2t, dx_dtype=dt)
        torch.cuda.synchronize()
        ref, e = C.dx(c, hid, dt == torch.bfloat16)
        check(f"mlp bwd_dx dX {tuple(spec)} {str(dt)[6:]} share {C.flagged_share(hid):.4f}",
              C.ratio(dx.float().cpu(), ref, e), 1.0)


@pytest.mark.parametrize("D,HID,b1on,db1", C.WGRAD_FORMS)
def test_wgrad_rows(dev, cus, D, HID, b1on, db1):
    """lthm_mlp_wgrad: dW1, dW2, db1 per element at 1 .. 5 token tiles per slice, FULL and masked,
    M = 5 and M = 0; two runs bit-identical"""
    from recommendations_amd import kernels as K
    ns_big = K.mlp_plan("wgrad", 1 << 20, D, HID).nslice  # the slice count once every slice has a tile
    for M in C.wgrad_ms(ns_big) + [0]:
        spec = C.Spec(M, D, HID, b1on, 0)
        c = C.make_case(spec)
        plan = K.mlp_plan("wgrad", M, D, HID)
        assert plan.full == int(M % 32 == 0) and plan.nslice <= max(1, plan.ntiles)
        if M > 5:
            assert plan.nslice == ns_big and plan.max_tiles == -(-plan.ntiles // ns_big)
        x, dy, w1, b1, w2t, _ = _ops(c, dev)
        a = K.mlp_wgrad(x, dy, w1, b1, w2t, want_db1=db1)
        b = K.mlp_wgrad(x, dy, w1, b1, w2t, want_db1=db1)
        torch.cuda.synchronize()
        assert (a[2] is None) == (not db1)
        for u, v in zip(a, b):
            assert u is None or torch.equal(u, v)
        if M == 0:
            assert all(t is None or not bool(t.any()) for t in a)
            continue
        hid = C.hidden(c, backward=True)
        refs = C.wgrad(c, hid, plan.nslice)
        for name, got in zip(("dW1", "dW2", "db1"), a):
            if got is not None:
                check(f"mlp wgrad {name} M={M} D={D} HID={HID} tiles/slice {plan.max_tiles} full {plan.full}",
                      C.ratio(got.cpu(), *refs[name]), 1.0)


def test_refused_shapes(dev):
    """the predicate follows the plans: the forward's LDS ends D = 256 at HID = 7,424"""
    from recommendations_amd import kernels as K
    assert K.mlp_supported(256, 7424) and not K.mlp_supported(256, 7456) and K.mlp_supported(128, 8192)
    x = torch.zeros(33, 256, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(8192, 256, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError):
        K.mlp_fwd(x, w, None, w, None)  # refused by the Python check: nothing is launched
    with pytest.raises(RuntimeError):
        K.mlp_plan("fwd", 33, 256, 8192)


def test_m0_row_entry_points(dev, monkeypatch):
    """M = 0 through lthm_mlp_bwd, lthm_mlp_bwd_hidden and lthm_mlp_bwd_dx: nothing is launched,
    empty tensors (null data pointers) are taken"""
    from recommendations_amd import kernels as K
    c = C.make_case(C.Spec(0, 128, 64, True, 0))
    x, dy, w1, b1, w2t, _ = _ops(c, dev)
    monkeypatch.setattr(K, "_MLP_BWD_SPLIT", False)
    dx, G, dP = K.mlp_bwd(x, dy, w1, b1, w2t, dx_dtype=torch.float32)
    assert tuple(dx.shape) == (0, 128) and tuple(G.shape) == (0, 64) and tuple(dP.shape) == (0, 64)
    monkeypatch.setattr(K, "_MLP_BWD_SPLIT", True)
    dx, G, dP = K.mlp_bwd(x, dy, w1, b1, w2t, want_dx=False)  # lthm_mlp_bwd_hidden alone (no dX GEMM)
    assert dx is None and tuple(G.shape) == (0, 64) and tuple(dP.shape) == (0, 64)
    assert tuple(K.mlp_bwd_dx(x, dy, w1, b1, w2t).shape) == (0, 128)
    torch.cuda.synchronize()
    for e in ("bwd", "bwd_hidden", "bwd_dx", "fwd_ln"):
        assert K.mlp_plan(e, 0, 128, 64).grid == 0


# ------------------------------------------------------------------ the block's routes to these kernels
def _block_step(dev, d, H, bias, seed):
    """one TransformerBlock training step (B = 3, T = 37): output, dx and every parameter gradient"""
    from recommendations_amd.commons.transformers.configs import TransformerConfig
    from recommendations_amd.commons.transformers.layers import TransformerBlock
    B, T = 3, 37
    torch.manual_seed(seed)
    cfg = TransformerConfig(rotator_config={"ff_mult": 4}, is_causal=True,
                            attn_config=dict(attn_dropout=0.0, bias=bias, dropout=0.0, n_head=H, n_embd=d,
                                             attn_type="multi_head", pos_bias={"context_window": T}))
    blk = TransformerBlock(cfg)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if "pos_bias" in n or "ln_" in n or n.endswith("bias"):
                p.add_(0.1 * torch.randn(p.shape))
    x = torch.randn(B, T, d)
    dy = torch.randn(B, T, d) / (B * T * d) ** 0.5
    blk = blk.to(dev)
    xd = x.to(dev).requires_grad_(True)
    y = blk(xd)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    out = {"y - x": (y.detach() - xd.detach()).cpu(), "dx": xd.grad.cpu()}
    out.update({"d" + n: p.grad.cpu() for n, p in blk.named_parameters()})
    return out


@pytest.mark.parametrize("route", ["_MLP_LN", "_MLP_WG"])
@pytest.mark.parametrize("d,H,bias", [(128, 2, True), (256, 4, False)])
def test_block_routes_match_the_default(dev, monkeypatch, route, d, H, bias):
    """A TransformerBlock training step with layers._MLP_LN (ln_2 inside lthm_mlp_fwd_ln) or
    layers._MLP_WG (lthm_mlp_bwd_dx + lthm_mlp_wgrad) patched on against the default route on the
    same weights and inputs.  The test asserts the route reached its kernels.  A block does not
    expose the MLP kernels' operands, so the per-element bounds of mlp_case do not apply to its
    tensors; both routes round the same quantities to bf16 at the same points and differ by f32 sum
    order and by single bf16 steps of h2 / dh2, so they are held to each other by the bounds the suite
    holds the default route to its oracle with (relative Frobenius error 1e-3 on the output,
    1e-2 on every gradient: test_gpu_encoder.py test_block_c2_c5_shapes_vs_bf16_oracle)."""
    from recommendations_amd import kernels as K
    from recommendations_amd.commons.transformers import layers
    from parity import relerr
    ref = _block_step(dev, d, H, bias, seed=d + H)
    calls = []
    names = ("mlp_fwd_ln",) if route == "_MLP_LN" else ("mlp_bwd_dx", "mlp_wgrad")
    for name in names:
        fn = getattr(K, name)
        monkeypatch.setattr(K, name, lambda *a, _fn=fn, _n=name, **kw: (calls.append(_n), _fn(*a, **kw))[1])
    monkeypatch.setattr(layers, route, True)
    got = _block_step(dev, d, H, bias, seed=d + H)
    assert set(calls) == set(names), calls
    assert set(got) == set(ref)
    for k in ref:
        check(f"block {route} d={d} {k} vs the default route", relerr(got[k], ref[k]), 1e-3 if k == "y - x" else 1e-2)
