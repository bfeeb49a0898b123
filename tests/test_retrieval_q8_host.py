"""Host-side tests of the e4m3 catalogue: the CPU restatement (tests/retrieval_q8_case.py) against
brute force, the quantiser's edge cases, the ABI surface, the container round trip, the refusals that
fire before any device work, and the recall of the format itself on the clustered unit case."""
import re

import numpy as np
import pytest
import torch

import retrieval_q8_case as C

D = C.D


def test_quantiser_edge_cases():
    x = C.edge_rows()
    codes, scale, e = C.quantize_ref(x)
    a = x.double().abs().amax(dim=1)
    for i in range(x.shape[0]):
        ei, ai = int(e[i]), float(a[i])
        if ai == 0:
            assert ei == 0 and float(scale[i]) == 1.0 and int(codes[i].max()) == 0
            continue
        assert -64 <= ei <= 64
        if ei == 64:  # the row near 2^-60 reaches the upper clamp (the rule asks for 69)
            assert i == 10 and ai * 2.0 ** 65 <= 448
        else:
            assert ai * 2.0 ** ei <= 448 < ai * 2.0 ** (ei + 1), (i, ai, ei)
        assert float(scale[i]) == 2.0 ** -ei
    f = codes.view(torch.float8_e4m3fn).float()
    assert torch.isfinite(f).all()
    # amax = 0.875 2^p lands on 448 exactly; the next bf16 above it scales to 225, which rounds to 224
    assert float(f[1].abs().max()) == 448.0 and float(f[2].abs().max()) == 224.0
    # a single non-zero element; every other code is +0
    assert int((codes[7] != 0).sum()) == 1
    # 1.0 -> 256 (e = 8): 2^-18, -2^-19 and 2^-30 scale to 2^-10 (a tie, to even: 0), -2^-11 and 2^-22, all 0
    assert f[8, 0] == 256.0 and torch.equal(f[8, 1:4].abs(), torch.zeros(3))
    # 2^-17 -> 2^-9, the smallest subnormal; 3 2^-18 -> 1.5 2^-9, a tie, to even: 2 2^-9; 2^-16 -> 2^-8
    assert f[9, 1] == 2.0 ** -9 and f[9, 2] == 2.0 ** -8 and f[9, 3] == 2.0 ** -8
    # dequantised rows reproduce what e4m3 can hold: relative error of the largest element <= 2^-4
    dq = C.dequant(codes, scale)
    big = x.double().abs().argmax(dim=1)
    ar = torch.arange(x.shape[0])
    assert ((dq[ar, big] - x.double()[ar, big]).abs() <= 2.0 ** -4 * a).all()


def test_restatement_against_brute_force():
    g = torch.Generator().manual_seed(3)
    items = torch.nn.functional.normalize(torch.randn(37, D, generator=g), dim=-1).to(torch.bfloat16)
    q = torch.nn.functional.normalize(torch.randn(5, D, generator=g), dim=-1).to(torch.bfloat16)
    ci, si, _ = C.quantize_ref(items)
    cq, sq, _ = C.quantize_ref(q)
    fi, fq = ci.view(torch.float8_e4m3fn).float().tolist(), cq.view(torch.float8_e4m3fn).float().tolist()
    s_hat = C.approx_scores(q, items)
    s = C.exact_scores(q, items)
    excl = np.array([[3, 3, -1, 99], [0, 1, 2, 36], [-5, 37, 40, -1], [5, 6, 7, 8], [36, 35, 34, 33]])
    sc, rows = C.shortlist_ref(q, items, 40, excl)
    for i in range(5):
        brute = [sum(fq[i][k] * fi[j][k] for k in range(D)) * float(sq[i]) * float(si[j]) for j in range(37)]
        assert np.allclose(brute, s_hat[i], rtol=0, atol=1e-12)
        ok = [j for j in range(37) if j not in set(excl[i].tolist())]
        order = sorted(ok, key=lambda j: (-brute[j], j))
        assert rows[i, :len(order)].tolist() == order and (rows[i, len(order):] == -1).all()
        assert np.isneginf(sc[i, len(order):]).all()
        # the two-stage list is the flat list restricted to the shortlist
        short = sorted(ok, key=lambda j: (-brute[j], j))[:12]
        want = sorted(short, key=lambda j: (-s[i, j], j))[:7]
        got_s, got_r = C.two_stage_ref(q, items, 12, 7, excl)
        assert got_r[i].tolist() == want
        assert np.array_equal(got_s[i], s[i, want].astype(np.float32))
    # re-scoring: invalid entries are absent, a duplicate appears twice
    rs, rr = C.rescore_ref(s, np.array([[4, -1, 37, 4, 9]] * 5), 5)
    for i in range(5):
        assert sorted(rr[i, :3].tolist()) == [4, 4, 9] and rr[i, 3:].tolist() == [-1, -1]
    assert np.abs(s_hat - s).max() < 0.03  # the format's own error on unit rows


def test_abi_surface():
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    protos = _lib.parse_header()
    assert protos["lthm_catalogue_quantize_q8"] == ("int", ["void*", "int64_t", "uint8_t*", "float*", "void*"])
    assert protos["lthm_retrieve_q8_ws_bytes"] == ("int64_t", ["int64_t", "int64_t", "int32_t", "int32_t", "int64_t"])
    assert protos["lthm_retrieve_q8_topk"] == ("int", ["uint8_t*", "float*", "int64_t", "void*", "int32_t", "int32_t", "int64_t",
                                                       "int32_t", "int32_t", "lthm_retrieve_excl*", "float*", "int32_t*",
                                                       "void*", "int64_t", "void*"])
    assert protos["lthm_retrieve_rescore_ws_bytes"] == ("int64_t", ["int64_t", "int32_t", "int32_t"])
    assert protos["lthm_retrieve_rescore"] == ("int", ["void*", "int64_t", "void*", "int32_t", "int32_t", "int64_t", "int32_t*",
                                                       "int32_t", "int32_t", "float*", "int32_t*", "void*", "int64_t", "void*"])
    lib = _lib.load()
    with open(_lib.HEADER) as f:
        assert int(re.search(r"#define\s+LTHM_ABI_VERSION\s+(\d+)", f.read()).group(1)) == 44
    assert lib.lthm_abi_version() == 44  # additive
    assert K.RETRIEVE_Q8_MAX_POOL == 1024
    for fn in (K.quantize_catalogue_q8, K.retrieve_q8_topk, K.retrieve_rescore):
        assert callable(fn)
    ws = lib.lthm_retrieve_q8_ws_bytes
    for ok in ((1, 1, 1, 0, 0), (256, 2_000_000, 1024, 0, 1024), (70, 3000, 100, 64, 37), (4096, 2_000_000, 256, 0, 0)):
        assert ws(*ok) > 0, ok
    for bad in ((0, 10, 1, 0, 0), (1 << 31, 10, 1, 0, 0), (1, 0, 1, 0, 0), (1, 1 << 31, 1, 0, 0), (1, 10, 0, 0, 0),
                (1, 10, 1025, 0, 0), (1, 10, 5, 32, 0), (1, 10, 5, 100, 0), (1, 10, 5, -64, 0), (1, 10, 5, 0, -1),
                (1, 10, 5, 0, 1025), (1, 1 << 30, 5, 64, 0)):
        assert ws(*bad) == -1, bad
    # the workspace grows with the list and with the exclusion lists
    assert ws(70, 3000, 100, 64, 37) > ws(70, 3000, 100, 64, 0) > 0
    rws = lib.lthm_retrieve_rescore_ws_bytes
    for ok in ((1, 1, 1), (33, 1024, 1024), ((1 << 31) - 1, 300, 10)):
        assert rws(*ok) > 0, ok
    for bad in ((0, 10, 1), (1 << 31, 10, 1), (1, 0, 1), (1, 1025, 1), (1, 10, 0), (1, 10, 11), (-1, 10, 1)):
        assert rws(*bad) == -1, bad
    # invalid arguments are refused before any launch, with the library's error code (no GPU here)
    base = 1 << 12
    big = 1 << 40
    assert lib.lthm_catalogue_quantize_q8(None, 4, base, base, None) == 1
    for args in ((base, 0, base, base), (base + 8, 4, base, base), (base, 4, base + 4, base), (base, 4, base, base + 2),
                 (base, 4, None, base), (base, 4, base, None), (base, 1 << 31, base, base)):
        assert lib.lthm_catalogue_quantize_q8(*args, None) == 1, args
    x = _lib.STRUCTS["lthm_retrieve_excl"]()
    import ctypes

    def q8(**kw):
        return lib.lthm_retrieve_q8_topk(kw.get("codes", base), kw.get("scale", base), kw.get("N", 100), kw.get("q", base),
                                         kw.get("dt", 0), 1, kw.get("Q", 4), kw.get("M", 10), kw.get("slab", 0),
                                         kw.get("x", None), kw.get("os", base), kw.get("orr", base), kw.get("ws", base),
                                         kw.get("wsb", big), None)
    x.rows, x.X = base, 0
    bad_x0 = ctypes.addressof(x)
    for kw in (dict(codes=None), dict(scale=None), dict(q=None), dict(os=None), dict(orr=None), dict(ws=None),
               dict(codes=base + 8), dict(q=base + 4), dict(ws=base + 8), dict(scale=base + 2), dict(os=base + 1),
               dict(orr=base + 3), dict(dt=2), dict(M=0), dict(M=1025), dict(slab=32), dict(slab=-64), dict(Q=0), dict(N=0),
               dict(wsb=16), dict(x=bad_x0)):
        assert q8(**kw) == 1, kw  # hipErrorInvalidValue
    for X, rows in ((1025, base), (5, None), (5, base + 2)):
        x.rows, x.X = rows, X
        assert q8(x=ctypes.addressof(x)) == 1, (X, rows)

    def rs(**kw):
        return lib.lthm_retrieve_rescore(kw.get("items", base), kw.get("N", 100), kw.get("q", base), kw.get("dt", 0), 1,
                                         kw.get("Q", 4), kw.get("rows", base), kw.get("M", 10), kw.get("k", 5),
                                         kw.get("os", base), kw.get("orr", base), kw.get("ws", base), kw.get("wsb", big), None)
    for kw in (dict(items=None), dict(q=None), dict(rows=None), dict(os=None), dict(orr=None), dict(ws=None),
               dict(items=base + 8), dict(q=base + 4), dict(ws=base + 8), dict(rows=base + 2), dict(os=base + 1),
               dict(orr=base + 3), dict(dt=2), dict(M=0), dict(M=1025), dict(k=0), dict(k=11), dict(Q=0), dict(N=0),
               dict(N=1 << 31), dict(wsb=16)):
        assert rs(**kw) == 1, kw


def _quantised(keep_exact=True, N=40):
    from recommendations_amd.models.lthm.sequence.retrieval import QuantizedItemCatalogue
    g = torch.Generator().manual_seed(5)
    ids = torch.arange(1, N + 1, dtype=torch.int64) * 3
    emb = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1).to(torch.bfloat16)
    codes, scale, _ = C.quantize_ref(emb)
    return QuantizedItemCatalogue(ids, codes, scale, emb if keep_exact else None), emb


def test_save_load_round_trip(tmp_path):
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue, QuantizedItemCatalogue
    for keep in (True, False):
        cat, emb = _quantised(keep)
        p = str(tmp_path / f"q8_{keep}.safetensors")
        cat.save(p)
        back = QuantizedItemCatalogue.load(p)
        assert len(back) == len(cat) == 40 and back.keep_exact == keep
        assert torch.equal(back.ids, cat.ids) and torch.equal(back.codes, cat.codes) and torch.equal(back.scale, cat.scale)
        assert (back.emb is None) == (not keep) and (not keep or torch.equal(back.emb, emb))
        if keep:  # the flat loader reads the same file as the exact catalogue
            flat = ItemCatalogue.load(p)
            assert torch.equal(flat.ids, cat.ids) and torch.equal(flat.emb, emb)
            assert torch.equal(back.to_flat().emb, emb)
    cat, _ = _quantised()
    assert cat.rows_of(torch.tensor([3, 4, 120, 0])).tolist() == [0, -1, 39, -1]
    assert cat.holds(torch.tensor([[6, 7]])).tolist() == [[True, False]]
    assert cat.to("cpu").ids.data_ptr() == cat.ids.data_ptr() or torch.equal(cat.to("cpu").ids, cat.ids)
    flat_path = str(tmp_path / "flat.safetensors")
    cat.to_flat().save(flat_path)
    with pytest.raises(ValueError, match="not a quantised item catalogue"):
        QuantizedItemCatalogue.load(flat_path)


def test_refusals_with_their_messages():
    from recommendations_amd import kernels as K
    from recommendations_amd.models.lthm.sequence.retrieval import (ClusteredItemCatalogue, ItemCatalogue,
                                                                    QuantizedItemCatalogue)
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    cat, emb = _quantised()
    lossy, _ = _quantised(False)
    q = torch.zeros((2, D))
    assert QuantizedItemCatalogue.default_shortlist(10) == 128 and QuantizedItemCatalogue.default_shortlist(100) == 400
    assert QuantizedItemCatalogue.default_shortlist(500) == 1024
    with pytest.raises(ValueError, match=r"takes k in 1\.\.1024 \(got 0\)"):
        cat.topk(q, 0)
    with pytest.raises(ValueError, match=r"takes k in 1\.\.1024 \(got 1025\)"):
        cat.topk(q, 1025)
    with pytest.raises(ValueError, match=r"shortlist must lie in k\.\.1024 \(got shortlist=5, k=10\)"):
        cat.topk(q, 10, shortlist=5)
    with pytest.raises(ValueError, match=r"shortlist must lie in k\.\.1024 \(got shortlist=1025, k=10\)"):
        cat.topk(q, 10, shortlist=1025)
    with pytest.raises(ValueError, match=r"rescore=True needs the exact rows"):
        lossy.topk(q, 10)
    with pytest.raises(ValueError, match=r"to_flat needs the exact rows"):
        lossy.to_flat()
    with pytest.raises(ValueError, match=r"to_flat needs the exact rows"):
        lossy.recall(q, 5)
    with pytest.raises(ValueError, match=r"takes \[Q, 128\] queries, one per row"):
        cat.topk(torch.zeros((2, 2, D)), 5)
    with pytest.raises(ValueError, match=r"exclude_ids must be int64 \[Q, X\]"):
        cat.topk(q, 5, exclude_ids=torch.zeros((2, 3), dtype=torch.int32))
    for bad, msg in ((dict(codes=cat.codes[:, :64]), "codes must be uint8"), (dict(scale=cat.scale[:5]), "scales must be f32"),
                     (dict(emb=emb.float()), "embeddings must be bf16"), (dict(ids=cat.ids.flip(0)), "strictly ascending"),
                     (dict(ids=cat.ids - 3), "must not hold 0")):
        kw = dict(ids=cat.ids, codes=cat.codes, scale=cat.scale, emb=emb)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            QuantizedItemCatalogue(**kw)
    # the wrapper: every argument the quantised path does not implement is refused by name, before the forward
    retrieve = LTHMModelWrapper.retrieve
    for kw, names in ((dict(heads=[0, 1]), "heads"), (dict(tag_all=1), "tag_all"), (dict(tag_any=1), "tag_any"),
                      (dict(tag_none=1), "tag_none"), (dict(after=(q[:, 0], q[:, 0].long())), "after"),
                      (dict(bias_weight=0.5), "bias_weight"), (dict(nprobe=2), "nprobe"), (dict(diversity=0.5), "diversity"),
                      (dict(pool=64), "pool"), (dict(group_cap=2), "group_cap"),
                      (dict(tag_any=1, bias_weight=2.0, pool=9), "tag_any, bias_weight, pool")):
        with pytest.raises(ValueError, match=rf"quantised catalogue does not take {names}: use catalogue.to_flat\(\)"):
            retrieve(None, {}, cat, 5, **kw)
    for sl in (4, 1025, 128.0, True):
        with pytest.raises(ValueError, match=r"shortlist takes k\.\.1024 rows"):
            retrieve(None, {}, cat, 5, shortlist=sl)
    with pytest.raises(ValueError, match=r"a quantised catalogue takes k in 1\.\.1024 \(got 2000\)"):
        retrieve(None, {}, cat, 2000)
    flat = ItemCatalogue(cat.ids, emb)
    with pytest.raises(ValueError, match=r"shortlist given, but this catalogue is not quantised"):
        retrieve(None, {}, flat, 5, shortlist=128)
    with pytest.raises(ValueError, match=r"shortlist given, but this catalogue is not quantised"):
        retrieve(None, {}, ClusteredItemCatalogue.from_assignment(flat, emb[:1].contiguous(), torch.zeros(len(flat), dtype=torch.int64)),
                 5, shortlist=128)
    # no CPU fall-back for the kernels themselves
    for call in (lambda: K.quantize_catalogue_q8(emb), lambda: K.retrieve_q8_topk(q, cat.codes, cat.scale, 5),
                 lambda: K.retrieve_rescore(q, emb, torch.zeros((2, 4), dtype=torch.int32), 2), lambda: cat.topk(q, 5),
                 lambda: flat.quantize()):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()


@pytest.mark.parametrize("k,shortlist", [(10, 128), (100, 256)])
def test_recall_of_the_format(k, shortlist):
    """Clustered unit rows (16 centres, noise 0.3, N = 4,096, Q = 64): the restatement's two-stage list
    is the exact top-k for every query.  A condition on the inputs (the seed), not on the device."""
    q, items = C.unit_case(64, 4096, True, 1)
    qb = q.to(torch.bfloat16)
    got_s, got_r = C.two_stage_ref(qb, items, shortlist, k)
    want_s, want_r = C.first_m(C.exact_scores(qb, items), k)
    assert np.array_equal(got_r, want_r)
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32))
