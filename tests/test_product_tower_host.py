"""CPU checks of the product-tower tests' own tools and of lthm_product_tower_plan.  No kernel is launched.

  * tests/product_tower_case.py: at every case the GPU test uses, the conditions on the inputs hold
    (ambiguous shares printed and pinned), the bounds accept a float32 CPU evaluation of the kernels'
    arithmetic in three summation orders, and reject each small fault a kernel can make, element-wise;
  * lthm_product_tower_plan (csrc/towers.hip) against a restatement of its rules, and against the
    plan every case names.
"""
import ctypes
import itertools

import pytest
import torch

import product_tower_case as C
from recommendations_amd import _lib

IDS = [s.name for s in C.SPECS]
AMBIGUOUS_PAIRS = {"ring16_s9": 1, "cross_f32img": 1}  # every other case: none


@pytest.fixture(scope="module")
def cases():
    out = {}
    for s in C.SPECS:
        c = C.make_case(s)
        out[s.name] = (c, C.reference(c))
    return out


def trunc_bf16(t):
    return C.trunc16(t.float()).double()


# ------------------------------------------------------------------ inputs
@pytest.mark.parametrize("name", IDS)
def test_inputs_meet_the_ambiguity_conditions(cases, name):
    c, r = cases[name]
    share, mask_amb, hist_amb = C.ambiguity(c, r)
    pairs = int(r.amb[~r.mask].sum())
    print(f"{name}: ambiguous pairs {pairs} (share {share:.2e}), mask {mask_amb}, histogram {hist_amb}")
    assert C.inputs_ok(c, r) and share <= 1e-3 and mask_amb == 0 and hist_amb == 0
    assert pairs == AMBIGUOUS_PAIRS.get(name, 0)
    assert not (r.amb & c.exact[:, None]).any()
    s = c.spec
    # the planted tokens do what they are there for
    w = C.ref_rows(c, r)
    if "tie" in c.plant:
        t = c.plant["tie"]
        assert not r.mask[t]
        for j, (np_, nb) in enumerate(s.mods):  # z sits on a grid value: the lower bucket
            p0 = sum(m[0] for m in s.mods[:j])
            for p in range(min(np_, 3)):
                assert float(r.z[t, p0 + p]) == float(c.grid[j][(5 * p + 1) % nb]) and int(r.bucket[t, p0 + p]) == (5 * p + 1) % nb
    if not s.cve_only and s.n >= len(C.PLANTS) * 2:
        assert not r.mask[c.plant["thr"]] and r.mask[c.plant["below"]] and r.mask[c.plant["zero"]] and r.mask[c.plant["id0"]]
        assert (w[c.plant["id0"]] == 0xffff).all()
        if s.nbins:
            assert int(r.hbin[c.plant["half"]]) == s.nbins // 2
            assert int(r.hbin[c.plant["one"]]) == int(r.hbin[c.plant["two"]]) == s.nbins - 1
    if name == "nf4_p256":  # a masked token in every position of a 16-token tile
        assert set((torch.nonzero(r.mask).view(-1) % 16).tolist()) == set(range(16))


# ------------------------------------------------------------------ bounds accept
@pytest.mark.parametrize("name", IDS)
def test_bounds_accept_a_float32_evaluation(cases, name):
    c, r = cases[name]
    s = c.spec
    for order in (0, 1, 2):
        e = C.evaluate_f32(c, order)
        problem, rows = C.check_discrete(c, r, e.rows, None if s.cve_only else e.mask)
        assert problem is None, (name, order, problem)
        ref, b = C.emb_reference(c, r, rows)
        xr, xb = C.xn_reference(c, r)
        re_, rx = C.ratio(e.emb, ref, b), C.ratio(e.xn, xr, xb)
        print(f"{name} order {order}: emb {re_:.4f} xn {rx:.4f} of the bound")
        assert re_ < 1.0 and rx < 1.0, (name, order, re_, rx)


# ------------------------------------------------------------------ bounds reject
def faults(c, r):
    """name -> (kind, value): the reference with one fault; only those that apply to the case"""
    s = c.spec
    n, Dout, mf = s.n, s.Dout, s.plan.path == "mfma"
    rows = C.ref_rows(c, r)
    t = C.terms(c, r, rows)
    pre = t.bias + t.map + t.bag + t.hist
    zero = lambda e: torch.where(r.mask[:, None], torch.zeros_like(e), e)
    tab = c.tab.double()
    live = torch.nonzero(~r.mask).view(-1)
    tok = int(live[-1])
    tile = slice(16 * (tok // 16), min(n, 16 * (tok // 16) + 16))
    safe = torch.where(r.mask[:, None], torch.zeros_like(rows), rows)
    G = tab[safe]  # [n, total, Dout]
    out = {}
    if mf:
        sd = int(rows[tok, 0]) // 32
        e = pre.clone()
        e[tile] -= (G[tile] * (safe[tile] // 32 == sd)[:, :, None]).sum(1)
        out["slab_dropped_last_tile"] = ("emb", zero(e))
        s1 = int(rows[tok].max()) // 32
        if s1 >= 1:
            hit = (safe // 32 == s1)[:, :, None]
            out["stale_slab"] = ("emb", zero(pre + ((tab[(safe - 32).clamp_min(0)] - G) * hit).sum(1)))
        e = pre.clone()
        e[tile] += tab[c.R]
        out["rows_beyond_R_nonzero"] = ("emb", zero(e))
        hh = trunc_bf16(r.xn) @ trunc_bf16(c.w_map).t()
        out["mapper_hi_hi_only"] = ("emb", zero(pre - t.map + hh))
        if s.bias:
            e = pre.clone()
            e[:, Dout - 16:] -= t.bias[:, Dout - 16:]
            out["bias_fragment_omitted"] = ("emb", zero(e))
        if n >= 32:
            b0 = 32 * (n // 32 - 1)
            e = zero(pre)
            e[b0:b0 + 32] = torch.cat([e[b0 + 16:b0 + 32], e[b0:b0 + 16]])
            out["tiles_swapped"] = ("emb", e)
        if Dout == 512:
            e = pre.clone()
            e[:, 256:] += r.xn @ (c.w_map.double()[:256] - c.w_map.double()[256:]).t()
            out["upper_slice_lower_weights"] = ("emb", zero(e))
    if s.nbins:
        out["histogram_twice"] = ("emb", zero(pre + t.hist))
    if r.mask.any():
        out["masked_not_zeroed"] = ("emb", pre)
    if not s.cve_only and n > 1:  # nf1_n1's only token is e_0: nothing to round
        out["xn_truncated"] = ("xn", trunc_bf16(r.xn))
    # discrete faults
    ok = torch.nonzero(~r.amb[tok]).view(-1)
    p = int(ok[0])
    bk = r.bucket.clone()
    nb_p = [nb for (np_, nb) in s.mods for _ in range(np_)][p]
    bk[tok, p] += 1 if int(bk[tok, p]) < nb_p else -1
    out["bucket_off_by_one"] = ("rows", C.ref_rows(c, r, bk))
    le, p0 = [], 0
    for j, (np_, nb) in enumerate(s.mods):
        le.append((c.grid[j].double()[None, None, :] <= r.z[:, p0:p0 + np_, None]).sum(-1))
        p0 += np_
    out["le_in_bucketize"] = ("rows", C.ref_rows(c, r, torch.cat(le, 1)))
    if "tiny" in c.plant and (s.cve_only or s.thr < 2.0 ** -50):
        other = r.xn / r.xn.pow(2).sum(1).sqrt().clamp_min(C.EPS)[:, None] if s.cve_only else r.xn
        oz, p0 = [], 0
        for j, (np_, nb) in enumerate(s.mods):
            oz.append((c.grid[j].double()[None, None, :] < (other @ c.proj[j].double())[:, :, None]).sum(-1))
        out["second_normalisation_" + ("applied" if s.cve_only else "omitted")] = ("rows", C.ref_rows(c, r, torch.cat(oz, 1)))
    return out


APPLIES = {"mfma": {"slab_dropped_last_tile", "rows_beyond_R_nonzero", "mapper_hi_hi_only", "bucket_off_by_one",
                    "le_in_bucketize"},
           "token": {"bucket_off_by_one", "le_in_bucketize"}}


@pytest.mark.parametrize("name", IDS)
def test_bounds_reject_each_fault(cases, name):
    c, r = cases[name]
    s = c.spec
    rows = C.ref_rows(c, r)
    ref, b = C.emb_reference(c, r, rows)
    xr, xb = C.xn_reference(c, r)
    fs = faults(c, r)
    assert APPLIES[s.plan.path] <= set(fs), name
    for what, (kind, bad) in fs.items():
        if kind == "emb":
            q = C.ratio(bad, ref, b)
            assert q >= 1.0, (name, what, q)
        elif kind == "xn":
            assert C.ratio(bad, xr, xb) >= 1.0, (name, what)
        else:
            problem, _ = C.check_discrete(c, r, bad, None)
            assert problem is not None, (name, what)
    print(name, "rejects", sorted(fs))


def test_every_fault_is_applied_somewhere(cases):
    seen = set()
    for c, r in cases.values():
        seen |= set(faults(c, r))
    assert seen == {"slab_dropped_last_tile", "stale_slab", "rows_beyond_R_nonzero", "bucket_off_by_one", "le_in_bucketize",
                    "second_normalisation_omitted", "second_normalisation_applied", "bias_fragment_omitted", "tiles_swapped",
                    "masked_not_zeroed", "mapper_hi_hi_only", "xn_truncated", "histogram_twice", "upper_slice_lower_weights"}


# ------------------------------------------------------------------ the plan
LDS_MAX = 160 * 1024
FIELDS = [f for f, _ in _lib.STRUCTS["lthm_ptower_plan_out"]._fields_ if f != "pad0"]


def make_desc(n, Din, Dout, mods, nbins, xbf=False, tabbf=True, embbf=True, cve_only=False, ids=True, rows_out=True,
              mask_out=True):
    d = _lib.STRUCTS["lthm_ptower_desc"]()
    d.ids, d.x, d.x_dtype, d.Din, d.n, d.Dout, d.n_mod = (64 if ids else None), 64, int(xbf), Din, n, Dout, len(mods)
    d.w_map = d.b_map = d.proj = d.grids = d.tables = d.emb_out = d.xn_out = 64
    d.tab_dtype, d.emb_dtype, d.cve_only, d.norm_bins, d.norm_threshold = int(tabbf), int(embbf), int(cve_only), nbins, 0.0625
    d.proj_total, d.grid_total = Din * sum(m[0] for m in mods), sum(m[1] for m in mods)
    d.cve_rows = sum((nb + 1) * np_ for np_, nb in mods)
    for j, (np_, nb) in enumerate(mods[:8]):
        d.mod_nproj[j], d.mod_nbins[j] = np_, nb
    d.rows_out, d.mask_out = (64 if rows_out else None), (64 if mask_out else None)
    return d


def plan_c(lib, d):
    p = _lib.STRUCTS["lthm_ptower_plan_out"]()
    rc = lib.lthm_product_tower_plan(ctypes.addressof(d), ctypes.addressof(p))
    if rc != 0:
        assert rc == 1
        return None
    return {f: getattr(p, f) for f in FIELDS}


def plan_py(n, Din, Dout, mods, nbins, xbf=False, tabbf=True, embbf=True, cve_only=False, ids=True, rows_out=True,
            mask_out=True):
    """The rules restated from the kernels' declarations (csrc/towers.hip).  None: refused."""
    if n < 0 or not 1 <= Din <= 256 or not 1 <= Dout <= 512 or len(mods) > 8:
        return None
    out = dict.fromkeys(FIELDS, 0)
    if n == 0:
        return out
    nproj, maxnb = sum(m[0] for m in mods), max([m[1] for m in mods], default=0)
    total = nproj + (1 if nbins > 0 else 0)
    if total > 1024:
        return None
    tok_lds = (Din * Dout + Din * nproj + sum(m[1] for m in mods) + 8 * Din) * 4 + 4 * total * 2 + 16
    opl = 1 if Dout <= 64 else 2 if Dout <= 128 else 4 if Dout <= 256 else 8
    if tok_lds > LDS_MAX or Dout % opl:
        return None
    R = sum((nb + 1) * np_ for np_, nb in mods) + max(nbins, 0)
    R32 = -(-R // 32) * 32
    nsl = 2 if Dout == 512 else 1
    Ds = Dout // nsl
    stage = (Din + 4) * Ds * 4 + 128 * (Din + 4) * 4       # mapper weights + normalised x
    emb_lds = 2 * 32 * Ds * 2 + stage + 512 * 8 + 128 * (R32 // 32 + 1) * 4
    mfma = (not cve_only and tabbf and embbf and ids and rows_out and mask_out and Ds in (16, 32, 64, 128, 256)
            and 1 <= R <= 4096 and emb_lds <= LDS_MAX and Din <= 64 and Din % 4 == 0 and maxnb <= 32 and nproj <= 256)
    out.update(path=int(mfma), total=total, R=R, R32=R32, nslab=R32 // 32, nslice=nsl, opl=opl, emb_lds_dynamic=emb_lds,
               tok_lds_dynamic=tok_lds)
    if mfma:
        dm = 32 if Din <= 32 else 64
        out.update(rows_dm=dm, rows_full=int(Din == dm), nf=Ds // 16, dma=int(Ds >= 128 and stage >= 2 * 32 * Ds * 2),
                   rows_grid=min(-(-n // 256), 4096), emb_grid_x=-(-n // 128), emb_grid_y=nsl,
                   rows_lds_static=256 * (dm + 4) * 4 + 256)
    else:
        out.update(tok_grid=max(1, min(-(-n // 4), 2048)))
    return out


MODS = {"r4096": (((124, 32),), 4), "r4097": (((124, 32),), 5), "p256": (((256, 1),), 0), "p257": (((257, 1),), 0),
        "nb32": (((4, 32), (1, 1)), 16), "nb33": (((4, 33),), 16), "none": ((), 0), "hist_only": ((), 8),
        "small": (((3, 4),), 8), "r512": (((30, 16),), 2), "p1024": (((128, 1),) * 8, 1), "nine": (((1, 1),) * 9, 0)}


def test_plan_matches_the_restated_rules():
    lib = _lib.load()
    seen, n_cases, refused = set(), 0, 0
    flags = [dict(), dict(xbf=True), dict(tabbf=False), dict(embbf=False), dict(cve_only=True), dict(ids=False),
             dict(rows_out=False), dict(mask_out=False)]
    for Din, Dout, mk, n, fl in itertools.product((0, 4, 8, 12, 16, 20, 30, 32, 36, 64, 68, 200, 256, 257),
                                                  (0, 16, 24, 32, 64, 100, 128, 256, 384, 512, 513), MODS,
                                                  (0, 1, 129, 257, 256 * 4096 + 1), flags):
        mods, nbins = MODS[mk]
        want = plan_py(n, Din, Dout, mods, nbins, **fl)
        got = plan_c(lib, make_desc(n, Din, Dout, mods, nbins, **fl))
        n_cases += 1
        assert got == want, (Din, Dout, mk, n, fl, got, want)
        if want is None:
            refused += 1
        elif n:
            seen.add((want["path"], want["rows_dm"], want["rows_full"], want["nf"], want["dma"], want["opl"]))
            assert want["emb_lds_dynamic"] <= LDS_MAX or not want["path"]
    assert refused > 1000 and n_cases - refused > 10000
    # every rows form, every NF with and without the ring where it exists, every OPL
    assert {(1, dm, f) for dm in (32, 64) for f in (0, 1)} <= {k[:3] for k in seen}
    assert {(nf, dma) for nf in (1, 2, 4) for dma in (0,)} | {(8, 0), (8, 1), (16, 0), (16, 1)} == {k[3:5] for k in seen if k[0]}
    assert {k[5] for k in seen if not k[0]} == {1, 2, 4, 8}


def test_plan_at_the_named_edges():
    lib = _lib.load()
    P = lambda *a, **k: plan_c(lib, make_desc(*a, **k))
    small = MODS["small"]
    # the two sides of the DMA inequality: (Din + 4) (4 Ds + 512) >= 128 Ds
    assert [P(9, Din, 256, *small)["dma"] for Din in (8, 16, 20)] == [0, 0, 1]
    assert [P(9, Din, 128, *small)["dma"] for Din in (8, 12)] == [0, 1]
    assert P(9, 68, 128, *small)["path"] == 0 and P(9, 30, 128, *small)["path"] == 0 and P(9, 64, 128, *small)["path"] == 1
    assert P(9, 32, 64, *MODS["r4096"])["path"] == 1 and P(9, 32, 64, *MODS["r4096"])["nslab"] == 128
    assert P(9, 32, 64, *MODS["r4097"])["path"] == 0
    assert P(9, 32, 64, *MODS["p256"])["path"] == 1 and P(9, 32, 64, *MODS["p257"])["path"] == 0
    assert P(9, 32, 64, *MODS["nb32"])["path"] == 1 and P(9, 32, 64, *MODS["nb33"])["path"] == 0
    assert P(9, 32, 64, *small, tabbf=False)["path"] == 0 and P(9, 32, 64, *small, rows_out=False)["path"] == 0
    p = P(9, 32, 384, *small)
    assert p["path"] == 0 and p["opl"] == 8 and p["nslice"] == 1
    p = P(300, 32, 512, *small)
    assert (p["path"], p["nslice"], p["nf"], p["emb_grid_x"], p["emb_grid_y"], p["rows_grid"]) == (1, 2, 16, 3, 2, 2)
    # the embedding kernel's LDS at Din 64, Dout 256: 141,312 B + 512 (R32 / 32 + 1) B, so R <= 1376 fits
    assert P(9, 64, 256, ((41, 32),), 23)["path"] == 1 and P(9, 64, 256, ((41, 32),), 23)["R"] == 1376
    assert P(9, 64, 256, ((41, 32),), 24)["path"] == 0 and P(9, 64, 256, *MODS["r4096"])["path"] == 0
    assert P(9, 64, 256, *MODS["r4096"])["emb_lds_dynamic"] == 207360
    # refusals, and the empty batch
    assert P(9, 257, 64, *small) is None and P(9, 32, 513, *small) is None and P(-1, 32, 64, *small) is None
    assert P(9, 200, 384, *small) is None           # the per-token kernel's LDS is asked of every descriptor
    assert P(9, 32, 64, *MODS["nine"]) is None
    assert P(0, 32, 64, *small) == dict.fromkeys(FIELDS, 0)
    p = _lib.STRUCTS["lthm_ptower_plan_out"]()
    assert lib.lthm_product_tower_plan(None, ctypes.addressof(p)) == 1
    assert lib.lthm_product_tower_plan(ctypes.addressof(make_desc(9, 32, 64, *small)), None) == 1


def plan_of_case(lib, c):
    d = C.fill_desc(_lib.STRUCTS["lthm_ptower_desc"](), c, C.host_ptrs(c))
    p = plan_c(lib, d)
    return C.Plan("mfma" if p["path"] else "token", p["rows_dm"], p["rows_full"], p["nf"], p["dma"], p["nslice"], p["nslab"],
                  p["opl"]), p


@pytest.mark.parametrize("name", IDS)
def test_every_case_runs_the_kernel_it_names(cases, name):
    c, _ = cases[name]
    got, p = plan_of_case(_lib.load(), c)
    assert got == c.spec.plan, (name, got)
    assert p["R"] == c.R and p["total"] == c.total


def test_the_cases_reach_every_kernel_instance(cases):
    plans = {s.name: s.plan for s in C.SPECS}
    mf = [p for p in plans.values() if p.path == "mfma"]
    assert {(p.dm, p.full) for p in mf} == {(32, 0), (32, 1), (64, 0), (64, 1)}
    assert {(p.nf, p.dma) for p in mf} == {(1, 0), (2, 0), (4, 0), (8, 0), (8, 1), (16, 0), (16, 1)}
    assert {p.nslab for p in mf if p.dma} >= {1, 2, 3, 4, 5, 9} and {p.nslab for p in mf if not p.dma} >= {1, 2, 3}
    assert {p.nslice for p in mf} == {1, 2}
    tk = [s for s in C.SPECS if s.plan.path == "token"]
    assert {s.plan.opl for s in tk} == {1, 2, 4, 8}
    assert {(s.xbf, s.tab == "bf16") for s in tk} == {(False, False), (False, True), (True, False), (True, True)}
    assert {s.embf32 for s in tk} == {False, True} and any(s.cve_only for s in tk)
    assert {s.n for s in C.MFMA_SPECS} >= {1, 127, 128, 129, 255, 256, 257, 513}
    assert {s.Din for s in C.MFMA_SPECS} >= {4, 8, 16, 28, 32, 36, 60, 64} and {s.Din for s in tk} >= {30, 37, 200}
    assert {s.Dout for s in tk} >= {24, 100, 384}
    assert any(s.xbf for s in C.MFMA_SPECS) and any(not s.bias for s in C.MFMA_SPECS) and any(s.nbins == 0 for s in C.MFMA_SPECS)
    assert any(c.R % 32 == 0 for c, _ in cases.values()) and any(c.R % 32 for c, _ in cases.values())
