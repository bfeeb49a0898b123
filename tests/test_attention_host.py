"""The references of tests/attention_case.py against autograd through the oracle's SDPA, and the
conditions the attention GPU tests rely on in their inputs and bounds.  CPU only."""
import math

import pytest
import torch

import attention_case as C
from oracle import ref


def _close(got, want, what):
    err = float((got - want).abs().max()) / max(float(want.abs().max()), 1.0)
    assert err < 1e-10, f"{what}: {err:.3e}"


@pytest.mark.parametrize("table", [True, False])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("kind", C.MASK_KINDS)
def test_explicit_backward_equals_autograd(kind, causal, table):
    _vs_autograd(kind, causal, table, False)


@pytest.mark.parametrize("kind", [None, "B,H"])
def test_explicit_backward_equals_autograd_shared_kv(kind):
    """one K/V head: dk / dv are the sums over the query heads"""
    _vs_autograd(kind, True, True, True)


def _vs_autograd(kind, causal, table, mqa):
    B, T, H, E = 2, 17, 2, 16
    c = C.make_case(B, T, H, E, causal, table, kind, seed=7, mqa=mqa)
    r = C.reference(c)
    q, k, v = (x.double().requires_grad_(True) for x in (c.q, c.k, c.v))
    tab = c.table.double().requires_grad_(True) if table else None
    mask = c.mask.double() if kind else None
    if causal:
        mask = ref.causal_mask(T).double() + (mask if mask is not None else 0.0)
    o = ref.sdpa(q, k.expand(B, H, T, E), v.expand(B, H, T, E), mask, tab)
    o.backward(c.dout.double())
    _close(r.out, o.detach(), "out")
    _close(r.dq, q.grad, "dq")
    _close(r.dk, k.grad, "dk")
    _close(r.dv, v.grad, "dv")
    if table:
        _close(r.dtable, tab.grad[: 2 * T + 1], "dtable")
        assert float(tab.grad[2 * T + 1:].abs().max()) == 0.0
    # lse against the scores the oracle builds (its causal_mask holds 1, not 0, on the kept keys:
    # the softmax does not see that, the lse would, so the causal rule is restated with zeros)
    with torch.no_grad():
        S = (q @ k.transpose(-2, -1)) / math.sqrt(float(E))
        S = ref.rel_pos_bias(S, tab) if table else S
        S = S + c.mask.double() if kind else S
        if causal:
            S = S + torch.zeros(T, T, dtype=torch.float64).masked_fill(ref.causal_mask(T)[0, 0] != 1.0, -float("inf"))
    _close(r.lse, torch.logsumexp(S, -1), "lse")
    # the model is the same code with roundings: it stays near the reference and is not it
    m = C.bf16_model(c)
    e = float(C.row_err(m.dq, r.dq).max())
    assert 0.0 < e < 1.0, e


def test_row_err_names_one_wrong_row():
    """one row of 1,000 scaled by 1.5 is invisible to the Frobenius 1e-2 bound's order of magnitude
    and has per-row error 0.5; an all-zero reference row is held to the floor"""
    g = torch.Generator().manual_seed(0)
    want = torch.randn(2, 2, 250, 16, generator=g, dtype=torch.float64)
    want[0, 0, 0] = 0.0
    got = want.clone()
    got[1, 0, 249] *= 1.5
    got[0, 0, 0] += 1e-4
    e = C.row_err(got, want)
    mx, at = C.worst(e)
    assert at == (1, 0, 249) and abs(mx - 0.5) < 1e-12
    assert float((got - want).norm() / want.norm()) < 2e-2
    assert 0.0 < float(e[0, 0, 0]) < 1e-2
    with pytest.raises(ValueError):
        C.row_err(got, torch.zeros_like(want))


def test_case_lists_cover_what_the_gpu_file_says():
    from collections import Counter
    assert len(set(C.ALL)) == len(C.ALL)
    assert all(s.B <= 3 and s.T <= 4096 for s in C.ALL)
    # every matrix case with and without the table but the 4096 one
    n = Counter(s._replace(table=True) for s in C.MATRIX)
    assert all(v == 2 or k.T == 4096 for k, v in n.items()) and sum(k.T == 4096 for k in n) == 1
    nk = {(s.T + 63) // 64 for s in C.MASKS}
    assert nk == {1, 2, 3, 4} and {s.E for s in C.MASKS} == {16, 32, 64, 128}
    assert {s.mask_kind for s in C.MASKS if s.T == 21} == set(C.MASK_KINDS[1:])
    # the masked backward's LDS: T (8 E + 72) + 16 bytes of 160 KiB
    lds = lambda T, E: T * (8 * E + 72) + 16
    assert all(lds(s.T, s.E) <= 160 * 1024 for s in C.MASKS + C.MQA + C.RANGE + C.GUARD if s.mask_kind)
    assert lds(149, 128) <= 160 * 1024 < lds(150, 128) and lds(256, 64) <= 160 * 1024
    assert all(lds(T, E) > 160 * 1024 for _, T, _, E in C.MASK_REFUSED)


@pytest.mark.parametrize("spec", C.ALL, ids=C.spec_id)
def test_generator_conditions_and_model_maxima(spec):
    b = C.bounds(spec)
    c, r = b.case, b.ref
    S = C.scores(c, torch.float32)
    assert bool(torch.isfinite(S).any(-1).all()), "a fully masked row"
    if spec.mask_kind:
        dead = torch.isinf(c.mask)
        assert not bool(dead[..., 0].any()), "key 0 is masked"
        frac = float(dead.float().mean())
        assert bool(dead.any()) and frac < 0.25, frac
        assert bool(torch.isfinite(c.mask[~dead]).all())
    if spec.scale != 1.0:
        smax = float(S[torch.isfinite(S)].abs().max())
        assert 100.0 <= smax <= 200.0, smax
    names = C.TENSORS + (("dtable",) if spec.table else ())
    for n in names:
        w = getattr(r, n)
        assert bool(torch.isfinite(w).all()), n
        if n in b.zero:
            assert float(w.abs().max()) == 0.0, n
            continue
        assert float(w.norm()) > 0.0, n
        # finite; of order 1e-2 for out / dk / dv, up to a few 1e-1 for the dq and dtable rows that
        # the bf16 O in delta = rowsum(dO o O) leaves ill-conditioned (near one-hot rows)
        assert math.isfinite(b.model_max[n]) and (b.model_max[n] < 1.0 or spec.scale != 1.0), (n, b.model_max[n])
        assert n != "out" or b.model_max[n] < 2e-2, b.model_max[n]
        assert b.model_max[n] > 0.0 or (spec.T == 1 and n in C.EXACT_AT_T1), n
        assert b.bound[n] > 0.0
    assert bool(torch.isfinite(r.lse).all()) and 0.0 < b.model_max["lse"] < 1e-3
    if b.zero:
        zb = C.zero_bound(c)
        assert all(0.0 < zb[n] < 1e-3 for n in b.zero)
    print(C.spec_id(spec), " ".join(f"{n}={e:.2e}" for n, e in b.model_max.items()))
