"""Inputs and plain references for the training step's row passes (tests/test_row_passes_host.py
pins the references on the CPU, tests/test_gpu_row_passes.py holds the kernels to them).

Everything here is numpy / torch on the CPU in int64, fp64, or -- where a kernel's result is
defined bit for bit -- IEEE f32 in the documented order.  Nothing is imported from
recommendations_amd: the references restate include/lthm.h and the comments above the kernels,
they share no code with them.
"""
import numpy as np
import torch

U24 = 2.0 ** -24  # unit roundoff of f32 (round to nearest)

# ------------------------------------------------------------------ token assembly
# small, non-production (div, mod) pairs keep the tables tiny
DIVMOD = {"hod": (7, 5), "how": (3, 11), "dow": (60, 4)}
N_ACT = 4
TOKEN_SHAPES = [(3, 21, 0), (5, 13, 3), (1, 1, 0)]  # (B, T_full, trim): 66, 55 and 2 rows
TOKEN_DS = [256, 64, 72, 70]

# timestamps: negatives, 0, -1, +-div and exact multiples of each div, values near 1.7e9, +-2^40.
# -7 comes first: the one-token case takes it (negative and an exact multiple of a div).
TS_SPECIAL = [-7, 0, -1, 1, 7, -3, 3, -60, 60, 420, -420, 1_700_000_040, 1_699_999_999, 1_700_000_001,
              2 ** 40, -(2 ** 40), 2 ** 40 + 1, -(2 ** 40) - 1, -1_700_000_000, -5, -61, 59, 61]
LABEL_SPECIAL = [-1, 4, -4, 7, -9, 12, 0, 3, 5, -8]


def n_wpe(T_full):
    """rows of the position table: three more than any position uses, so some stay unused"""
    return T_full + 4


def token_offsets(T_full):
    """row offsets of the stacked table [act | hod | how | dow | wpe | pad] that rows_out indexes"""
    off = {"act": 0}
    off["hod"] = off["act"] + N_ACT
    off["how"] = off["hod"] + DIVMOD["hod"][1]
    off["dow"] = off["how"] + DIVMOD["how"][1]
    off["wpe"] = off["dow"] + DIVMOD["dow"][1]
    off["pad"] = off["wpe"] + n_wpe(T_full)
    return off


def table_rows(T_full):
    return token_offsets(T_full)["pad"] + 1


def time_index(ts, div, mod):
    """PatternFromTimelocal: (ts // div) % mod with Python's floor semantics, int64"""
    return torch.remainder(torch.floor_divide(ts, div), mod)


def token_inputs(B, T_full, trim):
    """labels, ts (int64 [B, T_full]) and mask (uint8 [B, T_full], 1 = pad).  The mask is
    arbitrary (no left prefix), holds one fully padded sequence where B > 1 and pads inside the
    trimmed columns; the special timestamps and labels sit on live (non-pad, untrimmed) tokens.
    With a single token (B = T_full = 1) that token is the pad and carries the specials."""
    g = torch.Generator().manual_seed(1000 * B + 10 * T_full + trim)
    T = T_full - trim
    mask = (torch.rand(B, T_full, generator=g) < 0.3).to(torch.uint8)
    if B > 1:
        mask[B - 1] = 1
    if trim > 0:
        mask[0, 0] = 1
        mask[min(1, B - 1), trim - 1] = 1
    if T >= 3:
        mask[0, trim], mask[0, trim + 1], mask[0, trim + 2] = 0, 1, 0
    if B * T_full == 1:
        mask[0, 0] = 1
    n = B * T_full
    ts = torch.randint(-10 ** 6, 10 ** 6, (n,), generator=g, dtype=torch.int64)
    ts[torch.rand(n, generator=g) < 0.3] += 1_700_000_000
    labels = torch.randint(-9, 13, (n,), generator=g, dtype=torch.int64)
    live = ((mask == 0) & (torch.arange(T_full)[None, :] >= trim)).reshape(-1).nonzero().reshape(-1)
    if live.numel() == 0:
        live = torch.zeros(1, dtype=torch.int64)
    live = live[torch.randperm(live.numel(), generator=g)]
    k = min(live.numel(), len(TS_SPECIAL))
    ts[live[:k]] = torch.tensor(TS_SPECIAL[:k], dtype=torch.int64)
    live = live.flip(0)  # the labels' specials on other tokens than the timestamps' first ones
    k = min(live.numel(), len(LABEL_SPECIAL))
    labels[live[:k]] = torch.tensor(LABEL_SPECIAL[:k], dtype=torch.int64)
    return labels.view(B, T_full), ts.view(B, T_full), mask


def token_tables(B, T_full, trim, d, p_dtype):
    """P [B, T, d] (p_dtype) and the f32 tables; magnitudes differ so that the terms of a sum do"""
    g = torch.Generator().manual_seed(7 * B + T_full + 31 * d + (p_dtype == torch.bfloat16))
    T = T_full - trim
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"P": (3.0 * r(B, T, d)).to(p_dtype), "act": r(N_ACT, d), "hod": 0.5 * r(DIVMOD["hod"][1], d),
            "how": 2.0 * r(DIVMOD["how"][1], d), "dow": r(DIVMOD["dow"][1], d), "wpe": 0.1 * r(n_wpe(T_full), d),
            "pad": r(d), "ctx": r(B, d)}


def ref_token_rows(labels, ts, mask, trim):
    """rows_out [B (T + 1), 5] int64: slots 0..3 = off_act + label % 4, off_hod / how / dow + time
    index for an item token; (off_pad, 0xffff x 3) for a pad; 0xffff x 4 for position 0; slot 4 =
    off_wpe + T - t' for every position t'."""
    B, T_full = labels.shape
    T = T_full - trim
    off = token_offsets(T_full)
    rows = torch.full((B, T + 1, 5), 0xFFFF, dtype=torch.int64)
    rows[:, :, 4] = off["wpe"] + T - torch.arange(T + 1)[None, :]
    lab, t, m = labels[:, trim:], ts[:, trim:], mask[:, trim:] != 0
    item = torch.stack([off["act"] + torch.remainder(lab, N_ACT)] +
                       [off[k] + time_index(t, *DIVMOD[k]) for k in ("hod", "how", "dow")], dim=-1)
    pad = torch.tensor([off["pad"], 0xFFFF, 0xFFFF, 0xFFFF], dtype=torch.int64)
    rows[:, 1:, :4] = torch.where(m[:, :, None], pad, item)
    return rows.view(B * (T + 1), 5)


def ref_tokens_x0(tab, labels, ts, mask, trim, use_ctx):
    """x0 as the comment above tokens_fwd_k states it, summed in fp64, and the sum of the terms'
    magnitudes:  x0[b, 0] = wpe[T] (+ ctx[b]);
    x0[b, t + 1] = (mask ? pad : P[b, t] + act[lab] + hod[.] + how[.] + dow[.]) + wpe[T - 1 - t]"""
    B, T_full = labels.shape
    T = T_full - trim
    f = {k: v.double() for k, v in tab.items()}
    d = f["pad"].numel()
    lab, t, m = labels[:, trim:], ts[:, trim:], mask[:, trim:] != 0
    terms = [f["P"], f["act"][torch.remainder(lab, N_ACT)]]
    terms += [f[k][time_index(t, *DIVMOD[k])] for k in ("hod", "how", "dow")]
    item, item_abs = sum(terms), sum(x.abs() for x in terms)
    pad = f["pad"].view(1, 1, d).expand(B, T, d)
    wp = f["wpe"][T - 1 - torch.arange(T)][None]
    x = torch.empty(B, T + 1, d, dtype=torch.float64)
    mag = torch.empty_like(x)
    x[:, 1:] = torch.where(m[:, :, None], pad, item) + wp
    mag[:, 1:] = torch.where(m[:, :, None], pad.abs(), item_abs) + wp.abs()
    x[:, 0] = f["wpe"][T] + (f["ctx"] if use_ctx else 0.0)
    mag[:, 0] = f["wpe"][T].abs() + (f["ctx"].abs() if use_ctx else 0.0)
    return x, mag


def tie_f32(shape, g):
    """f32 values exactly half way between two neighbouring bf16 values (low half 0x8000), the
    kept mantissa bit even and odd alike: round to nearest even goes down for one, up for the other"""
    hi = torch.randint(0x3000, 0x4800, shape, generator=g, dtype=torch.int64)  # moderate exponents
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) << 31
    bits = (sign | (hi << 16) | 0x8000).to(torch.int64)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return bits.view(torch.float32)


def tokens_bwd_dx0(B, T, d, seed):
    """dx0 [B, T + 1, d] f32, every second element a bf16 rounding tie"""
    g = torch.Generator().manual_seed(seed)
    dx0 = torch.randn(B, T + 1, d, generator=g)
    ties = tie_f32((B, T + 1, d), g)
    sel = torch.rand(B, T + 1, d, generator=g) < 0.5
    return torch.where(sel, ties, dx0)


def ref_tokens_bwd(dx0, mask, trim):
    """dP = dx0[:, 1:] rounded to bf16 with exact zeros at the masked positions; dctx = dx0[:, 0]"""
    m = mask[:, trim:] != 0
    dP = torch.where(m[:, :, None], torch.zeros((), dtype=torch.float32), dx0[:, 1:]).to(torch.bfloat16)
    return dP, dx0[:, 0].clone()


def ref_table_grads(rows, dx0_2d, R):
    """fp64 index_add of dx0's rows into the stacked table, and the sum of magnitudes"""
    out = torch.zeros(R, dx0_2d.shape[1], dtype=torch.float64)
    mag = torch.zeros_like(out)
    dy = dx0_2d.double()
    for i in range(rows.shape[1]):
        keep = rows[:, i] != 0xFFFF
        out.index_add_(0, rows[keep, i], dy[keep])
        mag.index_add_(0, rows[keep, i], dy[keep].abs())
    return out, mag


# ------------------------------------------------------------------ outcome conditioning
def ref_outcome_index(labels, trim, future, n_outcomes):
    """[B, T + 1] int64: position t' < T carries labels[b, trim + t'], position T the future
    outcome; torch.remainder (floor) by n_outcomes"""
    B = labels.shape[0]
    oc = torch.cat([labels[:, trim:], torch.full((B, 1), future, dtype=torch.int64)], dim=1)
    return torch.remainder(oc, n_outcomes)


def ref_outcome(x, table, idx):
    """one f32 add, then round to nearest even: bf16 [B (T + 1), D]"""
    return (x + table[idx.reshape(-1)]).to(torch.bfloat16)


# ------------------------------------------------------------------ trim statistics
def ref_trim_stats(mask):
    """(first column holding a non-pad entry, T if none; number of all-pad columns)"""
    mask = np.asarray(mask)
    T = mask.shape[1]
    live = (mask == 0).any(axis=0) if mask.shape[0] else np.zeros(T, dtype=bool)
    return (int(np.argmax(live)) if live.any() else T), int(T - live.sum())


TRIM_TS = [1, 255, 256, 257, 700]


def trim_masks(B, T):
    """name -> uint8 [B, T]"""
    rng = np.random.default_rng(B * 1000 + T)
    out = {"all_pad": np.ones((B, T), np.uint8), "no_pad": np.zeros((B, T), np.uint8)}
    m = np.ones((B, T), np.uint8)
    m[B - 1, T - 1] = 0
    out["last_column_only"] = m
    m = (rng.random((B, T)) < 0.6).astype(np.uint8)
    m[:, : T // 3] = 1           # leading all-pad columns
    m[:, T // 2] = 1             # an all-pad column after the first live one: not a prefix
    m[0, T - 1] = 1
    out["non_prefix"] = m
    return out


# ------------------------------------------------------------------ row normalisation
ROWNORM_DS = [128, 256, 8, 136, 100, 3, 255]
ROWNORM_ROWS = [1, 17, 67]
ROWNORM_T = 5  # mask_group


def rownorm_inputs(rows, D, dtype):
    """list of (x [rows, D] dtype, g [rows, D] f32).  With rows >= 17 one input holds a zero row
    (row 1), a row of magnitude 1e3 (row 2) and one of 1e-3 (the last); with rows = 1 each of the
    three is an input of its own.  No row's squares underflow in f32."""
    g = torch.Generator().manual_seed(rows * 1000 + D)
    x = torch.randn(rows, D, generator=g)
    gr = torch.randn(rows, D, generator=g)
    if rows == 1:
        return [((x * s if s else torch.zeros_like(x)).to(dtype), gr) for s in (0.0, 1e-3, 1e3)]  # +0, never -0
    x[1] = 0.0
    x[2] *= 1e3
    x[rows - 1] *= 1e-3
    return [(x.to(dtype), gr)]


def rownorm_mask(rows):
    """uint8 [G, ROWNORM_T + 3] whose columns 2 .. 2 + T are the mask (a column-sliced view like
    mask[:, trim:]: row stride > T); the columns around the view are set, so a read outside it
    zeroes rows that must stay.  Rows 1 (zero), 2 and every fifth are masked."""
    G = (rows + ROWNORM_T - 1) // ROWNORM_T
    big = torch.ones(G, ROWNORM_T + 3, dtype=torch.uint8)
    flat = torch.zeros(G * ROWNORM_T, dtype=torch.uint8)
    flat[0::5] = 1
    flat[1:3] = 1
    big[:, 2:2 + ROWNORM_T] = flat.view(G, ROWNORM_T)
    return big, flat[:rows] != 0


def ref_rownorm(x):
    x = x.double()
    n = x.pow(2).sum(-1).sqrt()
    return x / n.clamp(min=1e-12)[:, None], n


def ref_rownorm_bwd(x, g):
    """dx = (g - y (y.g)) / |x| in fp64 (g / 1e-12 where |x| = 0: F.normalize's clamp) and the
    magnitude the bound is stated over: (|g_i| + |y_i| sum_j |y_j g_j|) / |x|"""
    y, n = ref_rownorm(x)
    g = g.double()
    den = n.clamp(min=1e-12)[:, None]
    dx = (g - y * (y * g).sum(-1, keepdim=True)) / den
    mag = (g.abs() + y.abs() * (y * g).abs().sum(-1, keepdim=True)) / den
    return dx, mag


# ------------------------------------------------------------------ column sums
COLSUM_SHAPES = [(1, 1), (63, 64), (65, 65), (257, 130), (5000, 70), (0, 5)]


def ref_colsum(x):
    return x.double().sum(0), x.double().abs().sum(0)


# ------------------------------------------------------------------ casts
CAST_NS = [1, 3, 4, 5, 1027]


def _f32_from_bits(bits):
    a = np.asarray(bits, dtype=np.uint32)
    return torch.from_numpy(a.view(np.float32).copy())


def cast_data():
    """1027 f32 values: ties in both directions, the largest finite f32 (rounds to inf),
    subnormals, -0.0, +-inf and NaN first; ties and ordinary values after them, ties at the end
    (the tail elements past the 4-wide vector body)."""
    g = torch.Generator().manual_seed(77)
    special = _f32_from_bits([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: down, up, and negative
                              0x7F7FFFFF, 0xFF7FFFFF,                          # +-max finite -> +-inf
                              0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x80000001,  # subnormals (two ties)
                              0x80000000, 0x00000000, 0x7F800000, 0xFF800000,  # -0, +0, +-inf
                              0x7FC00000, 0x7F7F8000, 0x3F7FFFFF, 0x00800000, 0x7F7F7FFF])
    body = torch.randn(1027 - special.numel() - 200, generator=g) * 100.0
    return torch.cat([special, body, tie_f32((200,), g)])


def bits16(t):
    return t.contiguous().view(torch.int16)


def bits32(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ hash-mask dropout
GOLDEN64 = 0x9E3779B97F4A7C15
SEEDS = [12345, 2 ** 63 + 0x1234_5678_9ABC]  # the second above 2^61 (and above 2^63: unsigned arithmetic)
DROP_PS = [0.0, 0.1, 0.5, 0.999]


def drop_thresh(p):
    """floor(p 2^24) of the f32 value of p (the C ABI takes p as a float)"""
    return int(np.floor(np.float64(np.float32(p)) * 2.0 ** 24))


def keep_ref(seed, idx, p):
    """include/lthm.h: element i is kept iff the top 24 bits of
    splitmix64(seed + i * 0x9E3779B97F4A7C15) are >= floor(p 2^24); numpy uint64, wrapping"""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + idx * np.uint64(GOLDEN64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)) >= np.uint64(drop_thresh(p))


def keep_py(seed, i, p):
    """the same in Python integers"""
    m = (1 << 64) - 1
    z = (seed + i * GOLDEN64) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return (z >> 40) >= drop_thresh(p)


def drop_scale(p):
    """s = float32(1) / (float32(1) - float32(p)) as a 0-dim f32 tensor"""
    one = torch.ones((), dtype=torch.float32)
    return one / (one - torch.tensor(p, dtype=torch.float32))


def ref_dropout(x, p, seed, res1=None, res2=None, out_dtype=torch.float32):
    """((keep ? x * s : 0) + res1) + res2 in f32, in that order, rounded once to out_dtype"""
    keep = torch.from_numpy(keep_ref(seed, np.arange(x.numel()), p)).view(x.shape)
    v = torch.where(keep, x.float() * drop_scale(p), torch.zeros((), dtype=torch.float32))
    if res1 is not None:
        v = v + res1
    if res2 is not None:
        v = v + res2
    return v.to(out_dtype)


def ref_dropout_rows(x, groups, p, seed):
    """x [rows, groups * cols]: element (r, g, c) = x * (keep(g * rows + r) ? s : 0), rounded once"""
    rows = x.shape[0]
    cols = x.shape[1] // groups
    idx = np.arange(groups)[None, :] * rows + np.arange(rows)[:, None]            # [rows, groups]
    keep = torch.from_numpy(keep_ref(seed, idx, p))
    f = torch.where(keep, drop_scale(p), torch.zeros((), dtype=torch.float32))    # [rows, groups]
    return (x.float().view(rows, groups, cols) * f[:, :, None]).view(rows, groups * cols).to(x.dtype)


KEEP_RATE = {"n": 2 ** 20, "p": 0.3, "seed": SEEDS[0]}


def keep_rate_window(n, p):
    """the kept fraction lies within 5 sqrt(p (1 - p) / n) of 1 - p"""
    return 1.0 - p, 5.0 * float(np.sqrt(p * (1.0 - p) / n))
