"""CPU checks of tests/loss_case.py, the reference the contrastive-loss kernels are held to
(tests/test_gpu_loss_rows.py):

  * its fp64 reference equals autograd through oracle/lthm_ref.py::contrastive_loss run in
    float64 (loss, every statistic the oracle reports and both gradients to 1e-10) and reproduces
    the stored loss of two committed goldens;
  * the case list has the valid counts, lengths and sizes it names, every temperature lies on the
    side of the 2 / tau <= 80 switch it is meant for, and the softmax-range rows are what they
    claim to be;
  * the bounds are not vacuous (4 x the model's worst row <= 0.1) and every reference tensor that
    is zero is exactly zero.
"""
import math
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

import loss_case as LC

sys.path.insert(0, GOLDEN)
from contrastive_inputs import CASES, make_inputs  # noqa: E402

from oracle.lthm_ref import contrastive_loss  # noqa: E402

ids = lambda s: s.name  # noqa: E731


def _close(got, want, what):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    tol = 1e-10 * max(1.0, float(want.abs().max()))
    assert float((got - want).abs().max()) <= tol, (what, float((got - want).abs().max()), tol)


# the adversarial case holds exact ties: the oracle's hits@k come from topk, whose order among equal
# logits is arbitrary, so its hits are compared everywhere but there (the ranks still are)
@pytest.mark.parametrize("name,hits", [("m-left", True), ("geo", True), ("n129", True), ("logq-tau0.05", True),
                                       ("adv-tau0.025", False), ("ybf16-tbf16", True), ("mbs1", True)])
def test_reference_equals_fp64_oracle(name, hits):
    b = LC.bounds(LC.BY_NAME[name])
    c, ref = b.case, b.ref
    y = c.y.double().requires_grad_(True)
    t = c.t.double().requires_grad_(True)
    loss, stats = contrastive_loss(y, t, c.mask, c.offs, c.mbs, c.tau, list(c.ks),
                                   logq=None if c.logq is None else c.logq.double())
    _close(float(loss.detach()) if torch.is_tensor(loss) else loss, ref.loss, "loss")
    if torch.is_tensor(loss) and loss.requires_grad:
        (loss * c.g).backward()
        _close(y.grad, ref.dy, "dy")
        _close(t.grad, ref.dt, "dt")
    else:
        assert b.zero == ("dy", "dt")
    for mb, per_head in enumerate(stats):
        for h, st in enumerate(per_head):
            row = ref.stats[h, mb]
            if st is None:
                assert float(row[LC.ST_USED]) == 0.0
                continue
            assert st["used"] == int(row[LC.ST_USED]) == int(row[LC.ST_TOKENS])
            _close(st["loss"], row[LC.ST_CE], "CE")
            _close(st["neg"], row[LC.ST_NEG], "negatives")
            _close(st["mean_rank"], row[LC.ST_RANK], "mean rank")
            _close(st["median_rank"], row[LC.ST_MEDIAN], "median rank")
            if hits:
                _close(st["hits"], row[LC.ST_HITS:], "hits")


@pytest.mark.parametrize("name", ["train_ragged", "train_logq"])
def test_reference_reproduces_golden_loss(name):
    """the bound of tests/test_loss_goldens_cpu.py: 1e-5 relative to the stored loss"""
    case, fx = CASES[name], golden("contrastive_" + name)
    inp = make_inputs(case)
    logq = None if case["beta"] == 0.0 else -case["beta"] * torch.from_numpy(inp["logq"])
    c = SimpleNamespace(y=torch.from_numpy(inp["y"]), t=torch.from_numpy(inp["tgt"]), mask=torch.from_numpy(inp["mask"]),
                        offs=np.asarray(fx["offsets"]), mbs=case["mbs"], tau=case["tau"], ks=tuple(case["ks"]),
                        logq=logq, g=1.0)
    ref_loss = float(fx["loss"][0])
    assert abs(LC.reference(c).loss - ref_loss) <= 1e-5 * abs(ref_loss)


def test_valid_counts():
    for s in LC.VALID:
        m = LC.valid_counts(LC.bounds(s).case)
        assert tuple(row[0] for row in m) == LC.M_VALUES, s.name
    assert set(LC.M_VALUES) >= {1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257}
    mixed = LC.bounds(LC.VALID[1]).case.mask
    assert bool((mixed[:, 1:] & ~mixed[:, :-1]).any()), "the mixed case has no interior pad"


def test_full_sizes():
    for s in LC.FULL:
        c = LC.bounds(s).case
        n = int(s.name[1:])
        assert s.mbs * s.T == n and s.B == s.mbs + 1 and not bool(c.mask.any())
        assert LC.valid_counts(c) == [[n], [s.T]]
    assert {int(s.name[1:]) for s in LC.FULL} >= {63, 64, 65, 127, 128, 129}


def test_geometry_lengths():
    s = LC.GEOMETRY[0]
    assert tuple(max(s.T - o, 0) for row in s.offs for o in row) == LC.GEO_L
    assert {1, 2, 63, 65, 100, 129, 300} <= set(LC.GEO_L) and max(LC.GEO_L) > 128 + 64
    assert any(o >= s.T for row in s.offs for o in row)
    v = LC.GEOMETRY[0].valid
    assert 0 in v and 1 in v and 2 in v
    # mini-batch 0 holds the sequences with 0, 1 and 2 valid tokens: the row of the full sequence sees
    # their 3 tokens only, below k = 5 of ks
    st = LC.bounds(s).ref.stats
    assert float(st[0, 0, LC.ST_MINNEG]) == 3.0 < sorted(s.ks)[1] and float(st[0, 0, LC.ST_USED]) == 303.0
    short = {x.name: x for x in LC.SHORT}
    assert 64 // short["mbs130-T3"].T >= 21 and short["mbs130-T3"].mbs == 130
    assert short["mbs40-T8"].mbs == 40 > 32
    for x in LC.ALL:
        B, T, NH, n_mb, n_max = LC.geometry(LC.bounds(x).case)
        assert x.mbs * T <= 4224 and (NH <= 3 or x.name == "nh6") and max(x.ks) > x.mbs * T
    assert LC.geometry(LC.bounds(LC.BY_NAME["n4096"]).case)[4] == 4096
    assert 2049 <= 32 * 65 <= 2112 < LC.geometry(LC.bounds(LC.BY_NAME["n2080"]).case)[4] + 1


def test_min_negatives_below_smallest_k():
    """sequences with one and two valid tokens next to a fully padded one: in the m = 2
    mini-batch of the valid-count cases each row has a single negative, below k = 5"""
    ref = LC.bounds(LC.VALID[0]).ref
    assert float(ref.stats[0, 1, LC.ST_MINNEG]) == 1.0 and float(ref.stats[0, 1, LC.ST_USED]) == 2.0
    assert float(ref.stats[0, 0, LC.ST_USED]) == 0.0  # m = 1: no negative at all


def test_dispatcher_side_of_every_tau():
    assert 2.0 / LC.TAU_LAST_FIXED == 80.0
    assert np.float32(LC.TAU_FIRST_RUNNING) == np.nextafter(np.float32(0.025), np.float32(0))
    assert float(np.float32(LC.TAU_FIRST_RUNNING)) == LC.TAU_FIRST_RUNNING
    for s in LC.ALL:
        kernel, wrapper = LC.takes_fixed_shift(s.tau, s.logq)
        assert kernel == wrapper, s.name  # both sides of the call take the same branch
        want = not s.logq and s.tau >= 0.025
        assert kernel == want, (s.name, s.tau)
    assert LC.takes_fixed_shift(LC.TAU_LAST_FIXED) == (True, True)
    assert LC.takes_fixed_shift(LC.TAU_FIRST_RUNNING) == (False, False)
    assert LC.takes_fixed_shift(0.01) == (False, False)


@pytest.mark.parametrize("spec", LC.RANGE, ids=ids)
def test_softmax_range_rows(spec):
    b = LC.bounds(spec)
    ref, it = b.ref, 1.0 / spec.tau
    ce = (ref.lse - ref.pos)
    # (a) head 0, mini-batch 0, sequence 0, even t: positive at +1/tau, 50 negatives at -1/tau
    r = torch.arange(0, 50, 2)
    assert bool(ref.used[0, 0, r].all()) and bool((ref.pos[0, 0, r] == it).all())
    assert bool((ref.cnt[0, 0, r] == 51).all()) and bool((ref.rank[0, 0, r] == 0).all())
    assert float(ce[0, 0, r].abs().max()) <= 51 * math.exp(-2 * it) + 1e-12  # 50 e^(-2/tau): at 2/tau = 80 below an f64 ulp
    # (b) sequence 1, even t: positive at -1/tau, negatives at +1/tau: CE = 2/tau + log(cnt - 1)
    r = 50 + torch.arange(0, 50, 2)
    assert bool((ref.pos[0, 0, r] == -it).all()) and bool((ref.rank[0, 0, r] == 50).all())
    assert float((ce[0, 0, r] - (2 * it + math.log(50))).abs().max()) <= 1e-9
    # (c) mini-batch 1, sequence 1: 50 negatives above (even t) and 45 that tie with the positive
    r = 50 + torch.arange(0, 50, 2)
    assert bool((ref.cnt[0, 1, r] - 1 == 95).all()) and bool((ref.rank[0, 1, r] == 50).all())
    # (d) mini-batch 2 (offset 0): every row of sequences 7 and 8 has cnt - 1 = 100 negatives, one of
    # them tied with the positive at a generic dot (the ranks then stay below 99)
    assert bool(torch.equal(b.case.t[7].double() / b.case.t[7].double().norm(dim=-1, keepdim=True),
                            b.case.t[8].double() / b.case.t[8].double().norm(dim=-1, keepdim=True)))
    assert bool((ref.cnt[0, 2, 50:150] - 1 == 100).all()) and int(ref.rank[0, 2, 50:150].max()) <= 99
    r = 50 + torch.arange(1, 50, 4)  # ties at the top: rank 0
    assert bool((ref.pos[0, 1, r] == it).all()) and bool((ref.rank[0, 1, r] == 0).all())


def test_logq_spread():
    for s in LC.LOGQ:
        q = LC.bounds(s).case.logq
        assert float(q.min()) < -6.0 and float(q.max()) > 6.0 and float(q.abs().max()) <= 6.5


@pytest.mark.parametrize("spec", LC.ALL, ids=ids)
def test_bounds_cap_and_zeros(spec):
    b = LC.bounds(spec)
    c, ref = b.case, b.ref
    B, T, NH, n_mb, n_max = LC.geometry(c)
    if spec.name in LC.NO_USED_ROW:
        assert not bool(ref.used.any()) and ref.loss == 0.0 and b.zero == ("dy", "dt")
        assert float(ref.stats[:, :, LC.ST_USED].abs().max()) == 0.0
    else:
        assert bool(ref.used.any()) and b.zero == ()
    assert 1e-2 <= LC.FLOOR <= 1e-1
    for key, m in b.model_max.items():
        if key != "lse":
            assert 0.0 < 4.0 * m <= 0.1, (spec.name, key, m)
            assert b.bound[key] == 4.0 * m
    assert b.bound["lse"] <= 1e-4
    # the bound is worth something for the typical row of every (mini-batch, head) of dy and of every
    # mini-batch of dt, not only for the largest: bound x max(1, floor / median row) <= 0.1, over the
    # groups with at least 8 non-zero rows.  In the softmax-range cases more than half of the rows of
    # mini-batches 0 and 1 cancel by construction (their median is e^-80 of the largest): there the
    # random mini-batch 2 is asserted, and the cancelling rows are held absolutely through the floor
    for (n, kind), bd in ((k, v) for k, v in b.bound.items() if isinstance(k, tuple)):
        want, scale, group = getattr(ref, n), getattr(ref, "s" + n), getattr(ref, "g" + n)
        allowed = LC.typical_allowed(want, scale, group, bd, min_rows=8)
        if spec.adv:
            allowed = {g: a for g, a in allowed.items() if (g // NH if n == "dy" else g) == 2}
        assert allowed and max(allowed.values()) <= 0.1, (spec.name, n, kind, allowed)
    # structural zeros of the reference: pad rows of dt, dy[:, T], dy rows with t >= L, and every
    # row of a mini-batch that holds a single sequence
    assert float(ref.dt[c.mask].abs().max() if bool(c.mask.any()) else 0.0) == 0.0
    assert float(ref.dy[:, T].abs().max()) == 0.0
    for mb in range(n_mb):
        sl = slice(mb * c.mbs, min((mb + 1) * c.mbs, B))
        for h in range(NH):
            L = max(T - int(c.offs[mb, h]), 0)
            assert float(ref.dy[sl, L:, h].abs().max()) == 0.0
        if sl.stop - sl.start == 1:
            assert float(ref.dy[sl].abs().max()) == 0.0 and float(ref.dt[sl].abs().max()) == 0.0
            assert float(ref.stats[:, mb, LC.ST_USED].abs().max()) == 0.0
