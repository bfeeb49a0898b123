"""Every kernel path of lthm_gemm (csrc/gemm.hip) against the fp64 reference of tests/gemm_case.py,
element by element.  Each test asks kernels.gemm_plan which kernel the call takes and asserts it is
the one the test is named for, runs kernels.gemm, holds every element of C (and of aux_out) to the
per-element bound, and checks that every byte of the destinations outside the [M, N] windows
(leading-dimension padding, a guard row above and below, the slabs between batch entries) is
unchanged.  Row counts scale with the device's CU count, so the plan assertions hold on any.
"""
import pytest
import torch

import gemm_case as G
import parity
from gemm_case import Spec

pytestmark = pytest.mark.gpu

BF, F = torch.bfloat16, torch.float32
LAYOUTS = ((True, True), (True, False), (False, True), (False, False))


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def run(spec, dev, kernel, workspace_splits=0, **expect):
    """plan + launch + per-element check of one spec; -> the plan"""
    from recommendations_amd import kernels as K
    s, c = spec, G.make_case(spec)
    lda, ldb, ldc, ldaux, ldr = G.lds(s)
    sA, sB, sC = G.strides(s)
    shape = (s.batch, s.M, s.N)
    flat = (1, s.batch * s.M, s.N)  # the epilogue tensors: batch entries follow each other
    od = G.DT[s.out_dtype]
    bA, oA, _ = G.place((s.batch, s.M, s.K), lda, sA, s.off_a, BF, c.A, kcontig=s.ka)
    bB, oB, _ = G.place((s.batch, s.N, s.K), ldb, sB, s.off_b, BF, c.B, kcontig=s.kb)
    bC, oC, iC = G.place(shape, ldc, sC, s.off_c, od)
    dC = bC.to(dev)
    kw = dict(a_kcontig=s.ka, b_kcontig=s.kb, lda=lda, ldb=ldb, ldc=ldc, out=dC[oC:], alpha=s.alpha, act=s.act,
              batch=s.batch, sA=sA, sB=sB, sC=sC, splits=s.splits, ldaux=ldaux, ldr1=ldr, ldr2=ldr)
    if c.bias is not None:
        bb = torch.zeros(s.N + 8)
        bb[s.off_bias:s.off_bias + s.N] = c.bias
        kw["bias"] = bb.to(dev)[s.off_bias:]
    if c.aux is not None:
        b, o, _ = G.place(flat, ldaux, 0, 0, BF, c.aux)
        kw["aux"] = b.to(dev)[o:]
    dX = iX = None
    if s.act in G.AUX_OUT_ACTS:
        bX, oX, iX = G.place(flat, ldaux, 0, 0, BF)
        dX = bX.to(dev)
        kw["aux_out"] = dX[oX:]
    for name, r, kind in (("res1", c.res1, s.res1), ("res2", c.res2, s.res2)):
        if r is not None:
            b, o, _ = G.place(flat, ldr, 0, 0, G.DT[kind], r)
            kw[name] = b.to(dev)[o:]
    if workspace_splits:  # the weight-gradient kernel sizes its splits by the caller's workspace
        kw["workspace"] = torch.empty(workspace_splits * s.M * s.N, dtype=F, device=dev)
    amax = torch.zeros(1, dtype=torch.int32, device=dev) if s.amax else None
    if amax is not None:
        kw["amax_out"] = amax
    dA, dB = bA.to(dev), bB.to(dev)
    plan = K.gemm_plan(dA[oA:], dB[oB:], s.M, s.N, s.K, **kw)
    assert plan.kernel == kernel, plan
    for k, v in expect.items():
        assert getattr(plan, k) == v, (k, plan)
    K.gemm(dA[oA:], dB[oB:], s.M, s.N, s.K, **kw)
    torch.cuda.synchronize()

    ref = G.reference(c)
    e, ea = G.bound(c, ref)
    hC = dC.cpu()
    assert G.untouched(hC, iC), "C: a write outside the [M, N] windows"
    got = hC[iC.reshape(-1)].reshape(shape)
    form = f"{kernel}<{plan.ka},{plan.kb},{plan.bres},{plan.epi},{plan.spread}> {plan.combine}"
    parity.check(f"gemm {form} {s.out_dtype} C err/bound", G.ratio(got, ref.C, e), 1.0)
    if dX is not None:
        hX = dX.cpu()
        assert G.untouched(hX, iX), "aux_out: a write outside the [M, N] windows"
        parity.check(f"gemm {form} aux_out err/bound",
                     G.ratio(hX[iX.reshape(-1)].reshape(shape), ref.aux_out, ea), 1.0)
    if amax is not None:
        # max |C| over the values as stored, as f32 bits (order-independent, so exact)
        want = got.float().abs().max().reshape(1).view(torch.int32)
        assert plan.amax == ("kernel" if kernel == "PS" else "after")
        assert int(amax.cpu()) == int(want), (int(amax.cpu()), int(want))
    return plan


# ------------------------------------------------------------------ gemm_k<KA, KB>
K128_SHAPES = {
    "interior": Spec(256, 128, 128),
    "ragged": Spec(200, 136, 72, bias=True, alpha=0.5),
    "k100_element_loads": Spec(136, 72, 100, bias=True, out_dtype="bf16"),
    "k1": Spec(70, 40, 1),
    "k7": Spec(70, 40, 7, out_dtype="bf16"),
    "m1": Spec(1, 136, 72, bias=True),
    "n1": Spec(200, 1, 72, bias=True, out_dtype="bf16"),
    "batch3": Spec(130, 72, 72, batch=3, pad_s=24, bias=True, res1="f32"),
    "batch3_odd_strides": Spec(130, 72, 72, batch=3, pad_s=3, pad_c=3, out_dtype="bf16", act=G.ACT_GELU),
}


@pytest.mark.parametrize("ka,kb", LAYOUTS)
@pytest.mark.parametrize("name", sorted(K128_SHAPES))
def test_gemm_k_shapes(dev, name, ka, kb):
    s = K128_SHAPES[name]._replace(ka=ka, kb=kb)
    plan = run(s, dev, "K128", ka=int(ka), kb=int(kb), combine="none")
    if name == "interior":
        assert plan.fast_ok == 1
    if name == "k100_element_loads" and (ka or kb):
        assert plan.fast_ok == 0  # rows of 200 bytes: only 8-byte aligned


K128_STRIDES = [dict(off_a=1), dict(off_b=1), dict(off_c=1), dict(off_c=1, out_dtype="bf16"), dict(off_bias=1)]
K128_STRIDES += [{f: p} for f in ("pad_a", "pad_b", "pad_c", "pad_aux", "pad_r") for p in (8, 3)]


@pytest.mark.parametrize("i", range(len(K128_STRIDES)))
def test_gemm_k_offsets_and_leading_dims(dev, i):
    ka, kb = LAYOUTS[i % 4]
    out_dtype = "bf16" if i % 2 else "f32"
    s = Spec(200, 136, 72, ka=ka, kb=kb, bias=True, act=G.ACT_GELU, res1="f32", out_dtype=out_dtype)
    run(s._replace(**K128_STRIDES[i]), dev, "K128")


RES_MIXES = ((None, None), ("f32", None), ("bf16", None), ("f32", "bf16"), ("bf16", "f32"))


@pytest.mark.parametrize("out_dtype", ("f32", "bf16"))
@pytest.mark.parametrize("act", range(7))
def test_gemm_k_epilogues(dev, act, out_dtype):
    for j, (r1, r2) in enumerate(RES_MIXES):
        ka, kb = LAYOUTS[(act + j) % 4]
        run(Spec(200, 136, 72, ka=ka, kb=kb, alpha=0.5, bias=act not in G.GRAD_ACTS or j % 2 == 0, act=act, res1=r1,
                 res2=r2, out_dtype=out_dtype), dev, "K128")


# ------------------------------------------------------------------ split-K through gemm_k
SPLITK = {
    "k200_three_asked_two_run": (Spec(200, 136, 200, splits=3, bias=True), dict(splits=2, combine="reduce4")),
    "k1024_four": (Spec(130, 72, 1024, splits=4, alpha=0.5, bias=True), dict(splits=4, combine="reduce4")),
    "n137_scalar_combine": (Spec(130, 137, 1024, splits=4, bias=True), dict(splits=4, combine="reduce")),
    "batch2": (Spec(130, 72, 1024, splits=4, batch=2, pad_s=16, alpha=0.5, bias=True, res1="f32"),
               dict(splits=4, combine="reduce")),
    "batch2_bf16_padded": (Spec(130, 70, 200, splits=2, batch=2, pad_c=3, pad_r=3, out_dtype="bf16", res1="bf16"),
                           dict(splits=2, combine="reduce")),
    "bf16_out": (Spec(200, 136, 1024, splits=4, out_dtype="bf16", bias=True), dict(splits=4, combine="reduce4")),
    "gelu_res_in_combine": (Spec(200, 136, 1024, splits=4, bias=True, act=G.ACT_GELU, res1="f32", res2="bf16",
                                 pad_aux=8, pad_c=8), dict(splits=4, combine="reduce4")),
    "grad_in_combine": (Spec(130, 137, 448, splits=2, act=G.ACT_QGELU_GRAD, res1="bf16", out_dtype="bf16", alpha=2.0),
                        dict(splits=2, combine="reduce")),
    "strided_operands": (Spec(200, 136, 1024, ka=False, kb=False, splits=4, bias=True), dict(splits=4, combine="reduce4")),
    "strided_b": (Spec(200, 136, 1000, kb=False, splits=3, out_dtype="bf16"), dict(splits=3, combine="reduce4")),
}


@pytest.mark.parametrize("name", sorted(SPLITK))
def test_gemm_k_split_k(dev, name):
    s, expect = SPLITK[name]
    run(s, dev, "K128", **expect)


# ------------------------------------------------------------------ gemm_wg_k
def _wg_splits(M, N, K, cus, cap):
    tiles = -(-M // 256) * -(-N // 256)
    sp = min(max(1, cus // tiles), cap, K // 256)
    kpw = -(-(-(-K // sp)) // 32) * 32
    return -(-K // kpw)


WG = [Spec(256, 256, 512), Spec(256, 256, 1000, alpha=0.25), Spec(256, 256, 777, res1="f32"),
      Spec(264, 520, 512, res1="bf16", alpha=0.25), Spec(264, 520, 1000, out_dtype="bf16"),
      Spec(264, 520, 777, out_dtype="bf16", res1="f32", res2="bf16", pad_c=8, pad_r=8)]


@pytest.mark.parametrize("i", range(len(WG)))
def test_gemm_wg(dev, i):
    s = WG[i]._replace(ka=False, kb=False)
    want = _wg_splits(s.M, s.N, s.K, _cus(dev), 4)
    assert want >= 2
    run(s, dev, "WG", workspace_splits=4, splits=want, combine="reduce4")


# ------------------------------------------------------------------ gemm_pp_k<false, SPREAD>
PP_SHAPES = ((300, 256, 512, 0, 0), (513, 520, 576, 1, 0), (256, 259, 512, 1, 0))  # M, N, K, SPREAD, pad_c
PP_EPIS = [dict(), dict(bias=True, out_dtype="bf16"), dict(bias=True, off_bias=1),
           dict(bias=True, res1="f32", res2="f32"), dict(res1="bf16", res2="bf16", out_dtype="bf16", alpha=0.5)]
PP_EPIS += [dict(act=a, bias=a not in G.GRAD_ACTS, out_dtype=("bf16", "f32")[a % 2]) for a in range(1, 7)]


@pytest.mark.parametrize("j", range(len(PP_EPIS)))
@pytest.mark.parametrize("shape", PP_SHAPES)
def test_gemm_pp(dev, shape, j):
    M, N, K, spread, pad_c = shape
    run(Spec(M, N, K, pad_c=pad_c, **PP_EPIS[j]), dev, "PP", spread=spread, ka=1, kb=1)


@pytest.mark.parametrize("out_dtype", ("f32", "bf16"))
def test_gemm_pp_amax_after(dev, out_dtype):
    run(Spec(300, 256, 512, bias=True, out_dtype=out_dtype, amax=True), dev, "PP", amax="after")
    run(Spec(512, 520, 576, act=G.ACT_GELU, out_dtype=out_dtype, amax=True), dev, "PP", amax="after", spread=1)


# ------------------------------------------------------------------ gemm_ps_k<KB, BRES, EPI>
PS_EPI = {  # EPI -> the spec fields that select it (two choices each, taken in turn)
    0: (dict(bias=True), dict(out_dtype="bf16")),
    1: (dict(bias=True, act=G.ACT_GELU, out_dtype="bf16"), dict(act=G.ACT_QGELU), dict(bias=True, act=G.ACT_GELU_D)),
    2: (dict(act=G.ACT_MUL_AUX, out_dtype="bf16"), dict(act=G.ACT_GELU_GRAD), dict(act=G.ACT_QGELU_GRAD)),
    3: (dict(bias=True, res1="f32"), dict(res1="f32", out_dtype="bf16", alpha=0.5)),
    4: (dict(bias=True, res1="f32", res2="f32"), dict(res1="f32", res2="f32", out_dtype="bf16")),
}
# (KB, K, EPI, choice): K = 64 / 256 hold B in LDS (BRES), K = 320 / 576 stream it
PS_FORMS = [(kb, k, epi, (kb + (k > 256) + epi) % len(PS_EPI[epi])) for kb in (1, 0) for k in (64, 320) for epi in range(5)]


def _ps_rows(dev, which):
    cus = _cus(dev)
    return {"whole": (4 * cus * 128, 128), "ragged_rows": (4 * cus * 128 + 37, 128),
            "two_column_tiles": (2 * cus * 128 + 5, 136)}[which]


def test_gemm_ps_forms_cover_all_twenty():
    assert {(kb, int(k <= 256), epi) for kb, k, epi, _ in PS_FORMS} == \
        {(kb, bres, epi) for kb in (0, 1) for bres in (0, 1) for epi in range(5)}


@pytest.mark.parametrize("kb,k,epi,choice", PS_FORMS)
def test_gemm_ps_forms(dev, kb, k, epi, choice):
    M, N = _ps_rows(dev, "whole")
    run(Spec(M, N, k, kb=bool(kb), **PS_EPI[epi][choice]), dev, "PS", kb=kb, bres=int(k <= 256), epi=epi,
        combine="none")


PS_MORE = [  # rows, K, spec fields, the plan
    ("ragged_rows", 256, dict(bias=True, amax=True), dict(kb=1, bres=1, epi=0, amax="kernel")),
    ("ragged_rows", 576, dict(kb=False, out_dtype="bf16", act=G.ACT_GELU, amax=True),
     dict(kb=0, bres=0, epi=1, amax="kernel")),
    ("two_column_tiles", 256, dict(kb=False, res1="f32", pad_c=8, pad_r=8, bias=True), dict(kb=0, bres=1, epi=3)),
    ("two_column_tiles", 576, dict(act=G.ACT_GELU_D, pad_aux=8, pad_c=8, out_dtype="bf16", bias=True),
     dict(kb=1, bres=0, epi=1)),
    ("two_column_tiles", 64, dict(act=G.ACT_MUL_AUX, pad_aux=8, alpha=0.5), dict(kb=1, bres=1, epi=2)),
    ("ragged_rows", 320, dict(res1="f32", res2="f32", pad_c=8), dict(kb=1, bres=0, epi=4)),
]


@pytest.mark.parametrize("i", range(len(PS_MORE)))
def test_gemm_ps_ragged_and_amax(dev, i):
    which, k, fields, expect = PS_MORE[i]
    M, N = _ps_rows(dev, which)
    run(Spec(M, N, k, **fields), dev, "PS", **expect)


def test_gemm_ps_falls_back_where_its_form_does_not_fit(dev):
    """a bf16 residual, an unaligned C and a 2-byte aligned operand leave the persistent kernel"""
    M, N = _ps_rows(dev, "two_column_tiles")
    run(Spec(M, N, 64, res1="bf16", out_dtype="bf16"), dev, "K128", epi=-1)
    run(Spec(M, N, 64, off_c=1, bias=True), dev, "K128", epi=-1)
    run(Spec(M, N, 64, off_a=1, kb=False), dev, "K128", fast_ok=0)
