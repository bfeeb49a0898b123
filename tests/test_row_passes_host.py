"""The references of tests/row_passes_case.py against brute force, and the conditions the row-pass
GPU tests rely on in their inputs.  CPU only."""
import math

import numpy as np
import pytest
import torch

import row_passes_case as C


# ------------------------------------------------------------------ floor-div / mod
def test_time_index_vs_python_ints():
    vals = C.TS_SPECIAL + [-(2 ** 40) + 1, 2 ** 40 - 1, -2, 2, -59, -62, 6, -6, 8, -8, 119, -119, 120, -120]
    ts = torch.tensor(vals, dtype=torch.int64)
    for div, mod in list(C.DIVMOD.values()) + [(3600, 24), (86400, 7)]:
        got = C.time_index(ts, div, mod).tolist()
        assert got == [(v // div) % mod for v in vals], (div, mod)
        assert all(0 <= i < mod for i in got)
    labs = list(range(-13, 14))
    for n in (4, 3):
        assert torch.remainder(torch.tensor(labs), n).tolist() == [v % n for v in labs]
    # the cases C's truncation gets wrong are present: a negative non-multiple for every div
    for div, _ in C.DIVMOD.values():
        assert any(v < 0 and v % div != 0 and int(v / div) != v // div for v in vals), div


# ------------------------------------------------------------------ token assembly
@pytest.mark.parametrize("shape", C.TOKEN_SHAPES)
def test_token_inputs_hold_the_edges(shape):
    B, T_full, trim = shape
    labels, ts, mask = C.token_inputs(B, T_full, trim)
    divs = [d for d, _ in C.DIVMOD.values()]
    kept = mask[:, trim:] != 0
    assert bool(kept.any()), "no pad row"
    assert bool((ts < 0).any()) and bool((labels < 0).any())
    assert any(bool(((ts % d == 0) & (ts != 0)).any()) for d in divs)
    if B * T_full == 1:
        return
    # on live tokens (not padded, not trimmed), whose values reach the kernel's arithmetic
    live = ~kept
    lts, llab = ts[:, trim:][live], labels[:, trim:][live]
    assert bool((lts < 0).any()) and bool((llab < 0).any()) and bool((llab >= 4).any())
    for d in divs:
        assert bool(((lts % d == 0) & (lts != 0)).any()), d
        assert bool(((lts < 0) & (lts % d != 0)).any()), d
    assert bool((lts.abs() >= 2 ** 40).any()) and bool(((lts - 1_700_000_000).abs() < 100).any())
    assert bool((lts == 0).any()) and bool((lts == -1).any())
    # the mask: not a left prefix, one fully padded sequence, pads inside the trimmed columns
    m = mask.numpy() != 0
    assert any(m[b, trim + t] and not m[b, trim + t - 1] for b in range(B) for t in range(1, T_full - trim))
    assert m[B - 1].all() and (trim == 0 or m[:, :trim].any())
    assert (~m[:, trim:]).any(axis=1).sum() >= 2


@pytest.mark.parametrize("shape", C.TOKEN_SHAPES)
def test_token_rows_vs_triple_loop(shape):
    B, T_full, trim = shape
    labels, ts, mask = C.token_inputs(B, T_full, trim)
    T = T_full - trim
    off = C.token_offsets(T_full)
    want = []
    for b in range(B):
        for tp in range(T + 1):
            row = [0xFFFF] * 4 + [off["wpe"] + T - tp]
            if tp > 0:
                c = trim + tp - 1
                if int(mask[b, c]):
                    row[0] = off["pad"]
                else:
                    v = int(ts[b, c])
                    row[0] = off["act"] + int(labels[b, c]) % 4
                    for s, k in enumerate(("hod", "how", "dow")):
                        div, mod = C.DIVMOD[k]
                        row[1 + s] = off[k] + (v // div) % mod
            want.append(row)
    got = C.ref_token_rows(labels, ts, mask, trim)
    assert got.tolist() == want
    # the tables do not overlap and every index is a row of the stacked table
    R = C.table_rows(T_full)
    used = got[got != 0xFFFF]
    assert int(used.min()) >= 0 and int(used.max()) < R < 0xFFFF
    assert off["wpe"] + T < off["pad"] - 1, "the position table keeps unused rows"


def test_tokens_x0_vs_loops():
    B, T_full, trim, d = 5, 13, 3, 6
    labels, ts, mask = C.token_inputs(B, T_full, trim)
    tab = C.token_tables(B, T_full, trim, d, torch.float32)
    T = T_full - trim
    for use_ctx in (True, False):
        x, mag = C.ref_tokens_x0(tab, labels, ts, mask, trim, use_ctx)
        for b in range(B):
            for tp in range(T + 1):
                for c in range(d):
                    terms = [float(tab["wpe"][T - tp, c])]
                    if tp == 0:
                        if use_ctx:
                            terms.append(float(tab["ctx"][b, c]))
                    elif int(mask[b, trim + tp - 1]):
                        terms.append(float(tab["pad"][c]))
                    else:
                        v, lab = int(ts[b, trim + tp - 1]), int(labels[b, trim + tp - 1])
                        terms += [float(tab["P"][b, tp - 1, c]), float(tab["act"][lab % 4, c])]
                        terms += [float(tab[k][(v // C.DIVMOD[k][0]) % C.DIVMOD[k][1], c]) for k in ("hod", "how", "dow")]
                    assert abs(float(x[b, tp, c]) - math.fsum(terms)) <= 1e-14 * sum(abs(t) for t in terms)
                    assert abs(float(mag[b, tp, c]) - sum(abs(t) for t in terms)) <= 1e-13 * float(mag[b, tp, c])


def test_tokens_bwd_reference_and_ties():
    B, T_full, trim, d = 5, 13, 3, 8
    _, _, mask = C.token_inputs(B, T_full, trim)
    T = T_full - trim
    dx0 = C.tokens_bwd_dx0(B, T, d, 3)
    bits = C.bits32(dx0).to(torch.int64) & 0xFFFF
    tie = bits == 0x8000
    assert 0.3 < float(tie.float().mean()) < 0.7
    up = (C.bits32(dx0).to(torch.int64) >> 16) & 1  # kept mantissa bit odd: the tie rounds away
    assert bool((tie & (up == 1)).any()) and bool((tie & (up == 0)).any())
    dP, dctx = C.ref_tokens_bwd(dx0, mask, trim)
    assert dP.dtype == torch.bfloat16 and torch.equal(dctx, dx0[:, 0])
    for b in range(B):
        for t in range(T):
            if int(mask[b, trim + t]):
                assert bool((C.bits16(dP[b, t]) == 0).all())  # +0, not -0
            else:
                assert torch.equal(dP[b, t], dx0[b, t + 1].to(torch.bfloat16))
    # round to nearest even on a tie: the result's last mantissa bit is 0
    r = C.bits16(dP[:, :][~(mask[:, trim:] != 0)]).to(torch.int64)
    t = tie[:, 1:][~(mask[:, trim:] != 0)]
    assert bool(((r[t] & 1) == 0).all())


def test_table_grads_vs_loop():
    B, T_full, trim, d = 3, 21, 0, 4
    labels, ts, mask = C.token_inputs(B, T_full, trim)
    rows = C.ref_token_rows(labels, ts, mask, trim)
    dx = C.tokens_bwd_dx0(B, T_full - trim, d, 5).view(-1, d)
    R = C.table_rows(T_full)
    got, mag = C.ref_table_grads(rows, dx, R)
    want = np.zeros((R, d))
    for n in range(rows.shape[0]):
        for i in range(5):
            if int(rows[n, i]) != 0xFFFF:
                want[int(rows[n, i])] += dx[n].double().numpy()
    assert np.abs(got.numpy() - want).max() <= 1e-12 * float(mag.max())
    unused = sorted(set(range(R)) - set(rows[rows != 0xFFFF].tolist()))
    assert unused and bool((got[unused] == 0).all())


# ------------------------------------------------------------------ outcome conditioning
def test_outcome_index_vs_loop():
    for B, T_full, trim in ((5, 13, 3), (3, 21, 0)):
        labels, _, _ = C.token_inputs(B, T_full, trim)
        T = T_full - trim
        assert B * (T + 1) in (55, 66)
        assert bool((labels[:, trim:] < 0).any())
        for n_out, future in ((4, -3), (3, -7), (4, 2)):
            got = C.ref_outcome_index(labels, trim, future, n_out)
            want = [[int(labels[b, trim + tp]) % n_out if tp < T else future % n_out for tp in range(T + 1)]
                    for b in range(B)]
            assert got.tolist() == want


# ------------------------------------------------------------------ trim statistics
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("T", C.TRIM_TS)
def test_trim_stats_vs_loop(B, T):
    masks = C.trim_masks(B, T)
    for name, m in masks.items():
        first, n_all = T, 0
        for t in range(T):
            col_live = any(m[b, t] == 0 for b in range(B))
            if col_live and first == T:
                first = t
            n_all += 0 if col_live else 1
        assert C.ref_trim_stats(m) == (first, n_all), name
    assert C.ref_trim_stats(masks["all_pad"]) == (T, T)
    assert C.ref_trim_stats(masks["no_pad"]) == (0, 0)
    assert C.ref_trim_stats(masks["last_column_only"]) == (T - 1, T - 1)
    if T >= 255:
        f, n = C.ref_trim_stats(masks["non_prefix"])
        assert 0 < f < T and n > f, "all-pad columns after the first live one"


# ------------------------------------------------------------------ row normalisation
def test_rownorm_reference_and_inputs():
    for rows in C.ROWNORM_ROWS:
        for D in (3, 136):
            for dtype in (torch.float32, torch.bfloat16):
                ins = C.rownorm_inputs(rows, D, dtype)
                assert len(ins) == (3 if rows == 1 else 1)
                allx = torch.cat([x for x, _ in ins]).double()
                n = allx.pow(2).sum(-1).sqrt()
                assert int((n == 0).sum()) == 1
                # no square of a non-zero element underflows in f32
                nz = allx[allx != 0].abs()
                assert float(nz.min()) ** 2 > 2.0 ** -126
                for x, g in ins:
                    y, nr = C.ref_rownorm(x)
                    dx, mag = C.ref_rownorm_bwd(x, g)
                    for r in range(rows):
                        xr = [float(v) for v in x[r].double()]
                        nn = math.sqrt(math.fsum(v * v for v in xr))
                        assert abs(float(nr[r]) - nn) <= 1e-15 * nn
                        gr = [float(v) for v in g[r]]
                        if nn == 0.0:
                            assert bool((y[r] == 0).all())
                            assert all(abs(float(dx[r, i]) - gr[i] / 1e-12) <= 1e-15 * abs(gr[i] / 1e-12) for i in range(D))
                            continue
                        yr = [v / nn for v in xr]
                        dot = math.fsum(a * b for a, b in zip(yr, gr))
                        for i in range(D):
                            assert abs(float(y[r, i]) - yr[i]) <= 1e-15
                            assert abs(float(dx[r, i]) - (gr[i] - yr[i] * dot) / nn) <= 1e-12 * float(mag[r, i])
        big, flat = C.rownorm_mask(rows)
        assert big.stride(0) > C.ROWNORM_T and flat.shape == (rows,) and bool(flat[0])
        if rows > 1:
            assert bool(flat[1]) and bool(flat[2]) and not bool(flat[rows - 1]) and not bool(flat.all())


# ------------------------------------------------------------------ casts
def test_cast_data_holds_the_edges():
    x = C.cast_data()
    assert x.numel() == 1027 == max(C.CAST_NS)
    b = C.bits32(x).to(torch.int64) & 0xFFFFFFFF
    tie = (b & 0xFFFF) == 0x8000
    kept_odd = ((b >> 16) & 1) == 1
    fin = torch.isfinite(x)
    assert bool((tie & kept_odd & fin).any()) and bool((tie & ~kept_odd & fin).any())
    assert bool(tie[-3:].all()), "ties in the scalar tail"
    y = x.to(torch.bfloat16)
    assert bool(torch.isinf(y[x == torch.finfo(torch.float32).max]).all())
    sub = (x != 0) & (x.abs() < 2.0 ** -126)
    assert int(sub.sum()) >= 4
    assert bool(((b == 0x80000000)).any()) and int(torch.isinf(x).sum()) == 2 and int(torch.isnan(x).sum()) >= 1
    # torch's own rounding is round to nearest even: spot values
    for bits, want in ((0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x7F7FFFFF, 0x7F80), (0x00008000, 0x0000),
                       (0x00018000, 0x0002), (0x80000000, 0x8000)):
        got = int(C.bits16(C._f32_from_bits([bits]).to(torch.bfloat16))[0]) & 0xFFFF
        assert got == want, hex(bits)


# ------------------------------------------------------------------ dropout
def test_keep_hash_vs_python_ints():
    for seed in C.SEEDS + [0, 2 ** 64 - 1]:
        idx = [0, 1, 2, 63, 64, 4999, 2 ** 31, 2 ** 40 + 3]
        for p in C.DROP_PS + [0.3]:
            got = C.keep_ref(seed, np.array(idx, dtype=np.uint64), p).tolist()
            assert got == [C.keep_py(seed, i, p) for i in idx], (seed, p)
    assert max(C.SEEDS) > 2 ** 61
    # the threshold is taken from the f32 value of p
    assert C.drop_thresh(0.0) == 0 and C.drop_thresh(0.5) == 2 ** 23
    assert C.drop_thresh(0.999) == 16760439 and C.drop_thresh(0.1) == 1677721
    assert bool(C.keep_ref(C.SEEDS[0], np.arange(5000), 0.0).all())
    s = C.drop_scale(0.3)
    assert s.dtype == torch.float32 and float(s) == float(np.float32(1) / (np.float32(1) - np.float32(0.3)))


def test_keep_rate_of_the_restatement():
    n, p, seed = C.KEEP_RATE["n"], C.KEEP_RATE["p"], C.KEEP_RATE["seed"]
    want, tol = C.keep_rate_window(n, p)
    assert abs(tol - 5 * math.sqrt(p * (1 - p) / n)) < 1e-15
    frac = float(C.keep_ref(seed, np.arange(n), p).mean())
    assert abs(frac - want) <= tol, (frac, want, tol)


def test_dropout_references_vs_loops():
    g = torch.Generator().manual_seed(1)
    n, p, seed = 257, 0.5, C.SEEDS[1]
    x, r1, r2 = (torch.randn(n, generator=g) for _ in range(3))
    s = np.float32(1) / (np.float32(1) - np.float32(p))
    y = C.ref_dropout(x, p, seed, r1, r2)
    for i in range(n):
        v = np.float32(x[i].item()) * s if C.keep_py(seed, i, p) else np.float32(0)
        v = np.float32(np.float32(v + np.float32(r1[i].item())) + np.float32(r2[i].item()))
        assert np.float32(y[i].item()) == v
    assert torch.equal(C.ref_dropout(x, 0.0, seed), x)
    rows, cols, groups = 37, 24, 3
    xr = torch.randn(rows, groups * cols, generator=g)
    yr = C.ref_dropout_rows(xr, groups, p, seed)
    for r in range(rows):
        for gi in range(groups):
            f = s if C.keep_py(seed, gi * rows + r, p) else np.float32(0)
            want = xr[r, gi * cols:(gi + 1) * cols].numpy() * f
            assert np.array_equal(yr[r, gi * cols:(gi + 1) * cols].numpy(), want)
    # g * rows + r and r * groups + g name different decisions
    keep_a = C.keep_ref(seed, np.arange(groups)[None, :] * rows + np.arange(rows)[:, None], p)
    keep_b = C.keep_ref(seed, np.arange(rows)[:, None] * groups + np.arange(groups)[None, :], p)
    assert (keep_a != keep_b).any()
