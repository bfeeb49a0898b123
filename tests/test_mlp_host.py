"""CPU checks of the fused-MLP tests' own tools and of lthm_mlp_plan.  No kernel is launched.

  * tests/mlp_case.py: at every case shape the GPU tests use (for a 256-CU device), the bounds
    accept a float32 CPU evaluation of the kernels' arithmetic and reject each small fault a
    kernel can make, element-wise; the share of hidden elements whose radius holds a bf16
    rounding boundary is pinned;
  * lthm_mlp_plan (csrc/mlp.hip) against a restatement of its rules.
"""
import ctypes
import itertools

import pytest
import torch

import mlp_case as C
from recommendations_amd import _lib

CUS = 256
FWD = C.fwd_specs(CUS)
BWD = sorted(set(C.bwd_specs(CUS, False) + C.bwd_specs(CUS, True) + C.bwd_dx_specs(CUS)))


def _nslice(M, HID, cus=CUS):
    return max(1, min(max(1, cus // max(1, HID // 128)), -(-M // 32)))


# the shapes test_wgrad_rows runs on a 256-CU device: 1 .. 5 token tiles per slice, FULL and ragged, M = 5
WG = [C.Spec(M, D, HID, b1on, 0) for D, HID, b1on, _ in C.WGRAD_FORMS for M in C.wgrad_ms(_nslice(1 << 20, HID))]


def _ids(specs):
    return ["-".join(str(int(v)) for v in s) for s in specs]


# ------------------------------------------------------------------ forward
def fwd_corruptions(c, hid):
    """name -> out (float64) of the reference with one fault; only those that apply to the spec"""
    M, D, HID = c.spec[:3]
    NC = HID // 32
    j = c.spec.hot if c.spec.hot >= 0 else NC - 1
    r0 = 32 * ((M - 1) // 32)  # the last 32-row wave tile (ragged unless M % 32 == 0)
    W2T, W1 = c.W2T.double(), c.W1.double()
    adds = ([c.b2.expand(M, -1)] if c.b2 is not None else []) + list(c.res)
    tail = sum((t.double() for t in adds), torch.zeros(M, D, dtype=torch.float64))
    y = hid.hb @ W2T
    ref = y + tail
    out = {}
    hb = hid.hb.clone()
    hb[r0:, 32 * j:32 * j + 32] = 0
    out["chunk_dropped"] = hb @ W2T + tail
    if NC > 1:
        W = W2T.clone()
        W[32 * j:32 * j + 32] = W2T[32 * (j - 1):32 * j]
        out["stale_w2t"] = hid.hb @ W + tail
        pre = hid.pre.clone()
        pre[:, 32 * j:32 * j + 32] += c.x.double() @ (W1[32 * (j - 1):32 * j] - W1[32 * j:32 * j + 32]).t()
        out["stale_w1"] = C.bf(C.G.gelu(pre)) @ W2T + tail
    if c.b1 is not None:
        pre = hid.pre.clone()
        pre[:, 32 * j:32 * j + 32] -= c.b1.double()[32 * j:32 * j + 32]
        out["b1_chunk_omitted"] = C.bf(C.G.gelu(pre)) @ W2T + tail
    if M >= 2:
        o = ref.clone()
        o[[M - 2, M - 1]] = o[[M - 1, M - 2]]
        out["rows_swapped"] = o
        o = ref.clone()
        o[M - 2] = ref[M - 1]  # the clamped row index reads x and the residuals of row M - 1 (mlp_fwd_epi)
        out["tail_row_clamped"] = o
    o = ref.clone()
    o[:, D - 32:] = 0
    out["column_tile_zeroed"] = o
    if c.res:
        out["residual_omitted"] = ref - c.res[-1].double()
    if c.b2 is not None:
        out["b2_omitted"] = ref - c.b2.double()
    return out


@pytest.mark.parametrize("spec", [s for s in FWD if s.M > 0], ids=_ids([s for s in FWD if s.M > 0]))
def test_forward_bound_accepts_f32_and_rejects_faults(spec):
    c = C.make_case(spec)
    hid = C.hidden(c)
    ref, e = C.fwd(c, hid=hid)
    share = C.flagged_share(hid)
    print(spec, "flagged share %.4f" % share)
    # 1 % wherever an input can reach it; without b1 at D = 256 the floor of a product-only hidden
    assert C.share_ok(hid.sg > 0, C.share_limit(spec.D, spec.bias, "h")), (spec, share)
    assert C.ratio(C.evaluate_f32(c).out, ref, e) < 1.0, spec
    for what, bad in fwd_corruptions(c, hid).items():
        assert C.ratio(bad, ref, e) >= 1.0, (spec, what)


# ------------------------------------------------------------------ backward
def bwd_corruptions(c, hid):
    """name -> dict of the outputs (G, dP, dX float64) one fault changes"""
    M, D, HID = c.spec[:3]
    NC = HID // 32
    j = NC - 1
    r0 = 32 * ((M - 1) // 32)
    W1 = c.W1.double()
    dX = hid.dpb @ W1
    sl = slice(32 * j, 32 * j + 32)
    out = {}
    d = hid.dpb.clone()
    d[r0:, sl] = 0
    out["chunk_dropped"] = dict(dX=d @ W1)
    if NC > 1:
        W = W1.clone()
        W[sl] = W1[32 * (j - 1):32 * j]
        out["stale_w1_second"] = dict(dX=hid.dpb @ W)
        pre = hid.pre.clone()
        pre[:, sl] += c.x.double() @ (W1[32 * (j - 1):32 * j] - W1[sl]).t()
        out["stale_w1"] = dict(G=C.bf(C.G.gelu(pre)), dP=C.bf(hid.dH * C.G.gelu_grad(pre)))
        dH = hid.dH.clone()
        W2T = c.W2T.double()
        dH[:, sl] = c.dy.double() @ W2T[32 * (j - 1):32 * j].t()
        out["stale_w2t"] = dict(dP=C.bf(dH * C.G.gelu_grad(hid.pre)))
    if c.b1 is not None:
        pre = hid.pre.clone()
        pre[:, sl] -= c.b1.double()[sl]
        out["b1_chunk_omitted"] = dict(G=C.bf(C.G.gelu(pre)), dP=C.bf(hid.dH * C.G.gelu_grad(pre)))
    if M >= 2:
        sw = [M - 1, M - 2]
        f = lambda t: torch.cat([t[:M - 2], t[sw]])  # noqa: E731
        out["rows_swapped"] = dict(G=f(hid.hb), dP=f(hid.dpb), dX=f(dX))
        g = lambda t: torch.cat([t[:M - 2], t[[M - 1, M - 1]]])  # noqa: E731
        out["tail_row_clamped"] = dict(G=g(hid.hb), dP=g(hid.dpb), dX=g(dX))
    o = dX.clone()
    o[:, D - 32:] = 0
    out["column_tile_zeroed"] = dict(dX=o)
    return out


@pytest.mark.parametrize("spec", [s for s in BWD if s.M > 0], ids=_ids([s for s in BWD if s.M > 0]))
def test_backward_bounds_accept_f32_and_reject_faults(spec):
    c = C.make_case(spec)
    hid = C.hidden(c, backward=True)
    share_h = float((hid.sg > 0).sum()) / hid.sg.numel()
    share_dp = float((hid.sd > 0).sum()) / hid.sd.numel()
    print(spec, "flagged share h %.4f dp %.4f" % (share_h, share_dp))
    assert C.share_ok(hid.sg > 0, C.share_limit(spec.D, spec.bias, "h")), (spec, share_h)
    # dp = dH GELU'(pre) always carries the radius of a D-term sum (dH has no bias): 1 % at D = 128
    # with b1, the floor elsewhere (mlp_case.share_limit)
    assert C.share_ok(hid.sd > 0, C.share_limit(spec.D, spec.bias, "dp")), (spec, share_dp)
    ev = C.evaluate_f32(c)
    refs = {"G": (hid.hb, hid.sg), "dP": (hid.dpb, hid.sd)}
    assert C.hidden_ratio(ev.G, *refs["G"]) < C.HIDDEN_OK and C.hidden_ratio(ev.dP, *refs["dP"]) < C.HIDDEN_OK
    for out_bf16 in (False, True):
        ref, e = C.dx(c, hid, out_bf16)
        got = C.bf(ev.dX) if out_bf16 else ev.dX
        assert C.ratio(got, ref, e) < 1.0
        ref2, e2 = C.dx_from_dp(c, ev.dP, out_bf16)
        assert C.ratio(got, ref2, e2) < 1.0
    ref, e = C.dx(c, hid, False)
    for what, bad in bwd_corruptions(c, hid).items():
        r = 0.0
        for k, v in bad.items():
            r = max(r, C.ratio(v, ref, e) if k == "dX" else C.hidden_ratio(v, *refs[k]))
        assert r >= 1.0 and r >= C.HIDDEN_OK, (spec, what, r)
    # the second check sees a dropped chunk at any HID: dX without it against the returned dP
    ref2, e2 = C.dx_from_dp(c, hid.dpb, False)
    assert C.ratio(bwd_corruptions(c, hid)["chunk_dropped"]["dX"], ref2, e2) >= 1.0


# ------------------------------------------------------------------ weight gradients
def wgrad_corruptions(c, hid, nslice):
    M, D, HID = c.spec[:3]
    x, dy = c.x.double(), c.dy.double()
    tiles = -(-M // 32)
    full = lambda rows: dict(dW1=hid.dpb[rows].t() @ x[rows], dW2=dy[rows].t() @ hid.hb[rows],  # noqa: E731
                             db1=hid.dp[rows].sum(0))
    allr = torch.arange(M)
    out = {}
    if tiles > 1:
        t = tiles - 2  # one whole token tile left out
        out["token_tile_left_out"] = full(torch.cat([allr[:32 * t], allr[32 * t + 32:]]))
    if M % 32:
        out["masked_rows_included"] = full(torch.cat([allr, torch.full((32 - M % 32,), M - 1)]))
    if nslice > 1:
        s = nslice - 1
        lo = 32 * (tiles * s // nslice)
        out["slice_not_folded"] = full(allr[:lo])
    ref = full(allr)
    o = ref["dW2"].clone()
    o[D - 32:, HID - 32:] = o[D - 32:, HID - 32:].t()
    out["dw2_tile_not_transposed"] = dict(ref, dW2=o)
    return out


@pytest.mark.parametrize("spec", WG, ids=_ids(WG))
def test_wgrad_bounds_accept_f32_and_reject_faults(spec):
    c = C.make_case(spec)
    hid = C.hidden(c, backward=True)
    ns = _nslice(spec.M, spec.HID)
    refs = C.wgrad(c, hid, ns)
    ev = C.evaluate_f32(c, ns)
    for k, (ref, e) in refs.items():
        assert C.ratio(getattr(ev, k), ref, e) < 1.0, (spec, k)
    for what, bad in wgrad_corruptions(c, hid, ns).items():
        for k, (ref, e) in refs.items():
            if what == "dw2_tile_not_transposed" and k != "dW2":
                continue
            assert C.ratio(bad[k], ref, e) >= 1.0, (spec, what, k)


# ------------------------------------------------------------------ LayerNorm prologue
@pytest.mark.parametrize("M,D,with_b", [(33, 128, True), (257, 256, False)])
def test_ln_bounds_accept_f32_and_reject_faults(M, D, with_b):
    x, lw, lb = C.ln_inputs(M, D, with_b)
    r = C.ln(x, lw, lb)
    mu = x.mean(1)
    d = x - mu[:, None]
    var = (d * d).mean(1)
    rs = 1.0 / torch.sqrt(var + 1e-5)
    y = d * rs[:, None] * lw + (lb if lb is not None else 0.0)
    assert C.ratio(mu, r.mean, r.e_mean) < 1.0 and C.ratio(rs, r.rstd, r.e_rstd) < 1.0
    assert C.ratio(C.bf(y), r.y, r.e_h) < 1.0
    assert C.ratio(1.0 / torch.sqrt(var.double()), r.rstd, r.e_rstd) >= 1.0        # no eps
    assert C.ratio(x[:, :D // 2].double().mean(1), r.mean, r.e_mean) >= 1.0         # half the row


# ------------------------------------------------------------------ the plan
ENTRIES = dict(FWD=0, FWD_LN=1, BWD=2, BWD_HIDDEN=3, BWD_DX=4, WGRAD=5)
LDS_MAX = 160 * 1024


def plan_c(lib, entry, M, D, HID, cus):
    p = _lib.STRUCTS["lthm_mlp_plan_out"]()
    rc = lib.lthm_mlp_plan(ENTRIES[entry], M, D, HID, cus, ctypes.addressof(p))
    if rc != 0:
        assert rc == 1
        return None
    return {k: getattr(p, k) for k, _ in p._fields_ if k != "pad0"}


def plan_py(entry, M, D, HID, cus):
    """The rules restated from the kernels' declarations (csrc/mlp.hip).  None: refused."""
    if D not in (128, 256) or HID < 32 or HID % 32 or HID > 8192 or M < 0 or cus < 1:
        return None
    img, strip = 32 * D * 2, 4096
    waves, ring, extra, dyn = {"FWD": (8, 3, 0, (HID + 3 * D) * 4), "FWD_LN": (8, 3, 0, (HID + 3 * D) * 4),
                               "BWD": (4, 2, 8192 * 4, 0), "BWD_HIDDEN": (8, 2, 4096 * 4, 0),
                               "BWD_DX": (4, 4, 4096 * 4, 0), "WGRAD": (4, 3, 0, 0)}[entry]
    if entry in ("BWD_HIDDEN", "BWD_DX") and HID > 4096:
        return None
    if entry == "WGRAD":
        if HID % 128:
            return None
        static = ring * 2 * img + waves * img
    else:
        static = ring * 2 * img + waves * strip + extra
    if static + dyn > LDS_MAX:
        return None
    out = dict(waves=waves, nslice=0, ngroup=0, full=0, ws_bytes=0, lds_static=static, lds_dynamic=dyn)
    if entry == "WGRAD":
        tiles = -(-M // 32)
        ng = HID // 128
        ns = max(1, min(max(1, cus // ng), tiles))
        return dict(out, tile_rows=32, ntiles=tiles, ngroup=ng, nslice=ns, full=int(M % 32 == 0),
                    ws_bytes=ns * HID * (2 * D + 1) * 4, grid=ns * ng if M else 0, max_tiles=-(-tiles // ns))
    tr = 32 * waves
    tiles = -(-M // tr)
    grid = min(tiles, cus)
    most = max((M * (b + 1) // grid - M * b // grid for b in range(grid)), default=0)
    return dict(out, tile_rows=tr, ntiles=tiles, grid=grid, max_tiles=-(-most // tr))


def test_plan_matches_the_restated_rules():
    lib = _lib.load()
    n = refused = 0
    for cus in (32, 64, 256, 304):
        for M, D, HID, entry in itertools.product((0, 1, 255, 256, 257, cus * 256 - 1, cus * 256 + 1, 528384), (128, 256),
                                                  (32, 96, 128, 1024, 4096, 4128, 7424, 7456, 8192), ENTRIES):
            want, got = plan_py(entry, M, D, HID, cus), plan_c(lib, entry, M, D, HID, cus)
            n += 1
            assert got == want, (entry, M, D, HID, cus, got, want)
            if want is None:
                refused += 1
                continue
            assert want["lds_static"] + want["lds_dynamic"] <= LDS_MAX
            if entry == "WGRAD":
                assert want["nslice"] <= max(1, want["ntiles"]) and want["nslice"] * want["max_tiles"] * 32 >= M
            else:
                assert want["grid"] * want["max_tiles"] * want["tile_rows"] >= M
    assert refused > 100 and n - refused > 1000


def test_plan_refusals_and_the_predicate():
    lib = _lib.load()
    for D, HID in itertools.product((64, 128, 256, 512), (0, 16, 32, 96, 4096, 4128, 7424, 7456, 8192, 8224)):
        both = plan_py("FWD", 0, D, HID, 256) is not None and plan_py("BWD", 0, D, HID, 256) is not None
        assert bool(lib.lthm_mlp_supported(D, HID)) == both, (D, HID)
    # mlp_fwd_k<256, 8>: 98,304 B of images + 32,768 B of strips + (HID + 768) 4 B > 160 KiB past HID = 7,424
    assert lib.lthm_mlp_supported(256, 7424) and not lib.lthm_mlp_supported(256, 7456)
    assert lib.lthm_mlp_supported(128, 8192)
    assert plan_c(lib, "FWD", 33, 256, 8192, 256) is None and plan_c(lib, "BWD", 33, 256, 8192, 256) is not None
    assert plan_c(lib, "BWD_DX", 5, 128, 4128, 256) is None and plan_c(lib, "BWD_HIDDEN", 5, 128, 4128, 256) is None
    assert plan_c(lib, "WGRAD", 5, 128, 96, 256) is None and plan_c(lib, "FWD", -1, 128, 96, 256) is None
    p = _lib.STRUCTS["lthm_mlp_plan_out"]()
    assert lib.lthm_mlp_plan(6, 5, 128, 96, 256, ctypes.addressof(p)) == 1
    assert lib.lthm_mlp_plan(0, 5, 128, 96, 0, ctypes.addressof(p)) == 1
    assert lib.lthm_mlp_plan(0, 5, 128, 96, 256, None) == 1
    assert lib.lthm_mlp_wgrad_ws_bytes(5, 128, 96) == -1
    # the C2 step's shapes: every workgroup walks several tiles
    assert plan_c(lib, "FWD", 528384, 256, 1024, 256)["max_tiles"] == 9
    assert plan_c(lib, "BWD_HIDDEN", 528384, 256, 1024, 256)["max_tiles"] == 9
