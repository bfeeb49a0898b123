"""The shared pad prefix (recommendations_amd/pad_prefix.py, include/lthm.h lthm_pad_prefix_*,
lthm_rows_move, the packed-row mode of the long-T' attention kernels) against references that
share nothing with the kernels.

One restatement serves every test: ``ref_maps`` builds the index maps from a mask in plain
numpy as include/lthm.h documents them, and ``packed_apply`` defines the packed form of a
per-sequence operation f as the autograd composition pack . f . unpack (two index_selects).
Backpropagating a packed gradient through that composition gives the packed gradients: the
chain-row sums over the sequences and the zero dO at the pads of every sequence but the chain's
owner both come out of the adjoints of the index_selects, none of the kernels' bookkeeping is
restated.  The helpers are pinned on the CPU (test_ref_helpers_cpu) against brute-force loops.

Integer maps and row moves are compared exactly; the chain sum elementwise against a derived
f32 bound; attention and the block per slice (the chain rows, each sequence's valid rows), so
that one wrong row is not averaged away by a whole-tensor norm.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from parity import check, relerr
from oracle import ref

gpu = pytest.mark.gpu


def bf(x):
    return x.to(torch.bfloat16)


# ------------------------------------------------------------------ the CPU restatement
def mask_from_npad(npad, T):
    """[B, T] uint8, 1 = pad: row b has its first npad[b] positions set."""
    return (np.arange(T)[None, :] < np.asarray(npad)[:, None]).astype(np.uint8)


class RefMaps:
    """include/lthm.h (lthm_pad_prefix_*) restated from a mask [B, T] (1 = pad).  Tp = T + 1
    positions per sequence; position 0 is always a chain row, position p <= npad[b] is the chain
    row p, the valid positions follow the chain in sequence order."""

    def __init__(self, mask):
        mask = np.asarray(mask) != 0
        B, T = mask.shape
        Tp = T + 1
        npad = np.zeros(B, dtype=np.int64)
        ok = True
        for b in range(B):
            n = 0
            while n < T and mask[b, n]:
                n += 1
            npad[b] = n
            ok = ok and not mask[b, n:].any()
        P = int(npad.max())
        owner = int(np.nonzero(npad == P)[0][0])
        valid = int((T - npad).sum())
        M = P + 1 + valid
        pof = np.full(B * Tp, -7, dtype=np.int64)
        pof_x = np.full(B * Tp, -7, dtype=np.int64)
        fop = np.full(M, -7, dtype=np.int64)
        first = np.zeros(B, dtype=np.int64)  # packed row of b's first valid position
        r = P + 1
        for b in range(B):
            first[b] = r
            for p in range(Tp):
                f = b * Tp + p
                if p <= npad[b]:
                    pof[f] = p
                    pof_x[f] = p if b == owner else -1
                    if b == owner:
                        fop[p] = f
                else:
                    pof[f] = pof_x[f] = r
                    fop[r] = f
                    r += 1
        assert r == M
        self.B, self.T, self.Tp, self.P, self.owner, self.M = B, T, Tp, P, owner, M
        self.ok, self.valid, self.npad, self.first = ok, valid, npad, first
        self.pof, self.pof_x, self.fop = pof, pof_x, fop

    def stats(self):
        return [int(self.ok), self.valid, self.P, self.owner]

    def valid_rows(self, b):
        """packed rows of sequence b's valid positions"""
        return slice(int(self.first[b]), int(self.first[b] + self.T - self.npad[b]))

    def chain_rows(self):
        return slice(0, self.P + 1)

    def first_live_tile(self, b, tile=32):
        """the first `tile`-row query tile that holds a row sequence b owns (Tp / tile rounded up
        when it owns none)"""
        own = np.nonzero(self.pof_x[b * self.Tp:(b + 1) * self.Tp] >= 0)[0]
        return int(own[0]) // tile if own.size else (self.Tp + tile - 1) // tile


def check_map_invariants(m):
    """What makes the maps a packing, whatever produced them."""
    assert (m.pof[m.fop] == np.arange(m.M)).all()                       # fop is a right inverse of pof
    assert ((m.pof_x == m.pof) | (m.pof_x == -1)).all()
    owned = np.sort(m.pof_x[m.pof_x >= 0])
    assert owned.size == m.M and (owned == np.arange(m.M)).all()         # every packed row owned once
    assert ((m.pof >= 0) & (m.pof < m.M)).all()


def packed_apply(f, packed, m):
    """pack . f . unpack: packed [M, W] -> f on [B, Tp, W] -> packed [M, W'] (autograd through
    both index_selects)."""
    pof = torch.from_numpy(m.pof)
    fop = torch.from_numpy(m.fop)
    full = packed.index_select(0, pof).view(m.B, m.Tp, -1)
    out = f(full)
    return out.reshape(m.B * m.Tp, -1).index_select(0, fop)


def attn_full(full_qkv, H, table, causal=True):
    """oracle/ref.sdpa on [B, Tp, 3 H E] rows laid out as the c_attn output -> [B, Tp, H E]"""
    B, Tp, C3 = full_qkv.shape
    E = C3 // (3 * H)
    q, k, v = full_qkv.view(B, Tp, 3, H, E).permute(2, 0, 3, 1, 4)
    mask = ref.causal_mask(Tp).to(full_qkv.dtype) if causal else None
    return ref.sdpa(q, k, v, mask, table).transpose(1, 2).reshape(B, Tp, H * E)


def lse_full(full_qkv, H, table):
    """log-sum-exp of the causal scores, [B, H, Tp]"""
    B, Tp, C3 = full_qkv.shape
    E = C3 // (3 * H)
    q, k, _ = full_qkv.view(B, Tp, 3, H, E).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) / math.sqrt(E)
    if table is not None:
        s = ref.rel_pos_bias(s, table)
    # not ref.causal_mask: the reference's mask is 1 (not 0) at the live keys, which a softmax
    # does not see and a log-sum-exp does
    return torch.logsumexp(s + torch.full((Tp, Tp), -float("inf"), dtype=s.dtype).triu(1), dim=-1)


# ------------------------------------------------------------------ CPU: the helpers themselves
MASKS = {
    "all_valid": ([0, 0, 0, 0, 0], 12),
    "all_padded": ([12, 12, 12], 12),
    "full_row_owner": ([3, 12, 5], 12),
    "full_row_not_owner": ([12, 2, 12], 12),
    "tie_lowest_b": ([2, 7, 7, 1], 12),
    "tile_edges": ([0, 1, 30, 31, 32, 33, 63, 64, 69], 70),
    "one_sequence": ([5], 12),
}


def _mask_300():
    rng = np.random.default_rng(300)
    npad = rng.integers(0, 15, size=300)
    npad[270] = npad[290] = 17  # the longest prefix only past the first 256-thread block, twice
    return npad.tolist(), 20


MASKS["b300_two_blocks"] = _mask_300()


@pytest.mark.parametrize("name", sorted(MASKS))
def test_ref_maps_invariants_cpu(name):
    npad, T = MASKS[name]
    m = RefMaps(mask_from_npad(npad, T))
    check_map_invariants(m)
    assert m.ok and m.npad.tolist() == list(npad) and m.P == max(npad) and m.owner == npad.index(max(npad))
    assert m.M == m.P + 1 + sum(T - n for n in npad)
    # the chain first, then the valid rows in sequence order: fop ascending past the chain
    assert (np.diff(m.fop[m.P + 1:]) > 0).all()
    assert (m.fop[:m.P + 1] == m.owner * m.Tp + np.arange(m.P + 1)).all()
    for b in range(m.B):
        rows = m.valid_rows(b)
        assert (m.fop[rows] == b * m.Tp + np.arange(npad[b] + 1, m.Tp)).all()


def test_ref_helpers_cpu():
    """pack . f . unpack at T' = 9 against brute-force fp64 attention over the full sequences:
    a softmax written as loops for the forward, and for the gradients an explicit adjoint (dO
    scattered to the rows the packed output read, the full gradients added into the packed row
    each full row was read from)."""
    npad, T, H, E = [0, 3, 8, 2, 8, 7], 8, 2, 4
    m = RefMaps(mask_from_npad(npad, T))
    check_map_invariants(m)
    C = H * E
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(m.M, 3 * C, generator=g, dtype=torch.float64)
    table = 0.5 * torch.randn(2 * m.Tp + 1, H, generator=g, dtype=torch.float64)
    dout = torch.randn(m.M, C, generator=g, dtype=torch.float64)
    qp = qkv.clone().requires_grad_(True)
    tp = table.clone().requires_grad_(True)
    got = packed_apply(lambda x: attn_full(x, H, tp), qp, m)
    got.backward(dout)
    # brute force on the full sequences
    full = qkv[torch.from_numpy(m.pof)].view(m.B, m.Tp, 3, H, E).numpy()
    out = np.zeros((m.B, m.Tp, H, E))
    lse = np.zeros((m.B, H, m.Tp))
    for b in range(m.B):
        for h in range(H):
            for q in range(m.Tp):
                s = np.array([full[b, q, 0, h] @ full[b, k, 1, h] / math.sqrt(E) + table[q - k + m.Tp, h].item()
                              for k in range(q + 1)])
                w = np.exp(s - s.max())
                lse[b, h, q] = math.log(w.sum()) + s.max()
                out[b, q, h] = (w / w.sum()) @ full[b, :q + 1, 2, h]
    out = out.reshape(m.B * m.Tp, C)
    assert np.abs(got.detach().numpy() - out[m.fop]).max() < 1e-12
    assert np.abs(lse_full(qkv[torch.from_numpy(m.pof)].view(m.B, m.Tp, -1), H, table).numpy() - lse).max() < 1e-12
    # the premise of the packing: a pad position's output depends on its position alone
    for b in range(m.B):
        for p in range(npad[b] + 1):
            assert np.abs(out[b * m.Tp + p] - out[m.owner * m.Tp + p]).max() < 1e-12
    # gradients: autograd on an independent full leaf, then the explicit adjoint
    fl = qkv[torch.from_numpy(m.pof)].clone().view(m.B, m.Tp, 3 * C).requires_grad_(True)
    tf = table.clone().requires_grad_(True)
    dfull = torch.zeros(m.B * m.Tp, C, dtype=torch.float64)
    dfull[torch.from_numpy(m.fop)] = dout
    attn_full(fl, H, tf).backward(dfull.view(m.B, m.Tp, C))
    want = np.zeros((m.M, 3 * C))
    np.add.at(want, m.pof, fl.grad.view(-1, 3 * C).numpy())
    assert np.abs(qp.grad.numpy() - want).max() < 1e-12
    assert np.abs(tp.grad.numpy() - tf.grad.numpy()).max() < 1e-12
    # dO reaches the pads of the chain's owner only
    assert (dfull.view(m.B, m.Tp, C)[torch.from_numpy(m.pof_x.reshape(m.B, m.Tp) < 0)] == 0).all()
    assert m.first_live_tile(m.owner, 4) == 0 and m.first_live_tile(1, 4) == 1 and m.first_live_tile(4, 4) == 3


# ------------------------------------------------------------------ 1. maps and stats, exact
def _stats(dev, mask_d):
    from recommendations_amd._lib import call, ptr, stream
    B, T = mask_d.shape
    npad = torch.full((B,), -3, dtype=torch.int32, device=dev)
    stats = torch.full((4,), -3, dtype=torch.int32, device=dev)
    call("lthm_pad_prefix_stats", ptr(mask_d), mask_d.stride(0), B, T, ptr(npad), ptr(stats), stream())
    return npad.cpu().numpy(), stats.tolist()


def _assert_maps_equal(pp, m):
    assert (pp.B, pp.T, pp.Tp, pp.P, pp.owner, pp.M) == (m.B, m.T, m.Tp, m.P, m.owner, m.M)
    for name in ("npad", "pof", "pof_x", "fop"):
        got = getattr(pp, name)
        assert got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy().astype(np.int64), getattr(m, name)), name


@gpu
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("name", sorted(MASKS))
def test_maps_and_stats_exact(dev, name, strided):
    """lthm_pad_prefix_stats / _maps through PadPrefix.build and the raw ABI against the numpy
    restatement, integer for integer; ``strided``: the mask as a column-offset view (row stride >
    T, as the trimmed wrapper passes it), the columns around it set so that a read outside
    the view changes npad."""
    from recommendations_amd.pad_prefix import PadPrefix
    npad, T = MASKS[name]
    mask = mask_from_npad(npad, T)
    m = RefMaps(mask)
    if strided:
        big = torch.ones(len(npad), T + 7, dtype=torch.uint8)
        big[:, 3:3 + T] = torch.from_numpy(mask)
        mask_d = big.to(dev)[:, 3:3 + T]
        assert mask_d.stride(0) > T
    else:
        mask_d = torch.from_numpy(mask).to(dev)
    got_npad, got_stats = _stats(dev, mask_d)
    assert np.array_equal(got_npad, m.npad)
    assert got_stats == m.stats()
    pp = PadPrefix.build(mask_d, min_gain=0.0)
    assert pp is not None
    _assert_maps_equal(pp, m)
    # the invariants on the kernel's own maps
    check_map_invariants(SimpleNamespace(M=pp.M, **{n: getattr(pp, n).cpu().numpy().astype(np.int64)
                                                    for n in ("pof", "pof_x", "fop")}))


@gpu
@pytest.mark.parametrize("row", [[1, 1, 0, 1, 0, 0], [0, 0, 1, 0, 0, 0], [1, 1, 1, 1, 0, 1]])
def test_not_a_prefix_mask(dev, row):
    """A hole after the pads, a pad after a valid position: stats[0] = 0 and no packing."""
    from recommendations_amd.pad_prefix import PadPrefix
    mask = mask_from_npad([2, 6, 0, 4], 6)
    mask[2] = row
    m = RefMaps(mask)
    assert not m.ok
    mask_d = torch.from_numpy(mask).to(dev)
    got_npad, got_stats = _stats(dev, mask_d)
    assert np.array_equal(got_npad, m.npad)
    assert got_stats[0] == 0 and got_stats == m.stats()
    assert PadPrefix.build(mask_d, min_gain=0.0) is None


@gpu
def test_build_min_gain(dev):
    """build returns None where the packed set is larger than (1 - min_gain) of the full one."""
    from recommendations_amd.pad_prefix import PadPrefix
    for npad, T in (([0, 0, 0, 0], 10), ([1, 0, 2, 0], 10), ([9, 8, 10, 7], 10), ([5, 5, 5, 5], 10)):
        mask = mask_from_npad(npad, T)
        m = RefMaps(mask)
        mask_d = torch.from_numpy(mask).to(dev)
        for gain in (0.1, 0.5):
            pp = PadPrefix.build(mask_d) if gain == 0.1 else PadPrefix.build(mask_d, min_gain=gain)
            if m.M > (1.0 - gain) * m.B * m.Tp:
                assert pp is None, (npad, gain)
            else:
                _assert_maps_equal(pp, m)
    assert PadPrefix.build(torch.from_numpy(mask_from_npad([0, 0, 0, 0], 10)).to(dev)) is None
    assert PadPrefix.build(torch.from_numpy(mask_from_npad([9, 8, 10, 7], 10)).to(dev)) is not None


# ------------------------------------------------------------------ 2. lthm_rows_move, exact
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def _bits(n, cols, dtype, g):
    """random bit patterns (NaNs and denormals included) as integers [n, cols] of dtype's width"""
    it = _INT[dtype]
    info = torch.iinfo(it)
    return torch.randint(info.min, info.max, (n, cols), generator=g, dtype=torch.int64).to(it)


def _rows_move(dev, src, sld, idx, dst, dld, rb, scatter):
    from recommendations_amd._lib import call, ptr, stream
    call("lthm_rows_move", ptr(src), sld, ptr(idx), idx.numel(), ptr(dst), dld, rb, scatter, stream())


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("row_bytes", [16, 48, 4112])
def test_rows_gather_exact(dev, row_bytes, dtype):
    """Gather through kernels.rows_gather (contiguous rows) and through the ABI with both
    leading dimensions wider than the row: bytewise against numpy indexing, zero rows at the
    negative indices, the destination's bytes past row_bytes untouched."""
    from recommendations_amd import kernels as K
    es = 2 if dtype == torch.bfloat16 else 4
    W, n, c = row_bytes // es, 37, 53
    g = torch.Generator().manual_seed(row_bytes + es)
    src = _bits(n, W, dtype, g)
    idx = torch.randint(0, n, (c,), generator=g, dtype=torch.int64)
    idx[torch.randperm(c, generator=g)[:9]] = -1
    idx[0], idx[1], idx[2] = n - 1, 0, -5
    want = src[idx.clamp(min=0)].clone()
    want[idx < 0] = 0
    idx_d = idx.to(torch.int32).to(dev)
    got = K.rows_gather(src.to(dev).view(dtype), idx_d)
    assert got.dtype == dtype and torch.equal(got.view(_INT[dtype]).cpu(), want)
    # wider leading dimensions: 16 B more per source row, 32 B more per destination row
    ps, pd = 16 // es, 32 // es
    src_w = _bits(n, W + ps, dtype, g)
    src_w[:, :W] = src
    dst_w = _bits(c, W + pd, dtype, g)
    want_w = dst_w.clone()
    want_w[:, :W] = want
    dst_d = dst_w.to(dev)
    _rows_move(dev, src_w.to(dev), (W + ps) * es, idx_d, dst_d, (W + pd) * es, row_bytes, 0)
    assert torch.equal(dst_d.cpu(), want_w)


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("row_bytes", [16, 48, 4112])
def test_rows_scatter_exact(dev, row_bytes, dtype):
    """Scatter (dst row idx[i] = src row i) through the ABI into a sentinel-filled destination
    with a leading dimension wider than the row: the negative indices are skipped, the rows no
    index names and the bytes past row_bytes keep the sentinel."""
    es = 2 if dtype == torch.bfloat16 else 4
    W, n, nd = row_bytes // es, 41, 60
    g = torch.Generator().manual_seed(2 * row_bytes + es)
    ps, pd = 32 // es, 16 // es
    src = _bits(n, W + ps, dtype, g)
    idx = torch.randperm(nd, generator=g)[:n]
    idx[torch.randperm(n, generator=g)[:11]] = -1
    idx[0] = -9
    dst = torch.full((nd, W + pd), 0x5A5A, dtype=_INT[dtype])
    want = dst.clone()
    sel = idx >= 0
    want[idx[sel], :W] = src[sel, :W]
    dst_d = dst.to(dev)
    _rows_move(dev, src.to(dev), (W + ps) * es, idx.to(torch.int32).to(dev), dst_d, (W + pd) * es, row_bytes, 1)
    assert torch.equal(dst_d.cpu(), want)


@gpu
def test_rows_move_in_place_empty_and_large(dev):
    """The documented in-place zeroing (out is src, idx[i] in {i, -1}); count = 0; and an index
    set of more 16-byte chunks than one pass of the capped grid covers (4096 blocks x 256
    threads: 70 000 rows of 256 B are 1 120 000 chunks), gathered and scattered."""
    from recommendations_amd import kernels as K
    g = torch.Generator().manual_seed(5)
    for dtype, W in ((torch.bfloat16, 24), (torch.float32, 1028)):
        n = 45
        src = _bits(n, W, dtype, g)
        keep = torch.rand(n, generator=g) < 0.6
        keep[0], keep[n - 1] = False, True
        idx = torch.where(keep, torch.arange(n), torch.full((n,), -1))
        want = src.clone()
        want[~keep] = 0
        buf = src.to(dev).view(dtype)
        out = K.rows_gather(buf, idx.to(torch.int32).to(dev), out=buf)
        assert out.data_ptr() == buf.data_ptr() and torch.equal(buf.view(_INT[dtype]).cpu(), want)
    # count = 0
    src = _bits(8, 8, torch.bfloat16, g).to(dev)
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    assert tuple(K.rows_gather(src.view(torch.bfloat16), empty).shape) == (0, 8)
    dst = torch.full((8, 8), 0x5A5A, dtype=torch.int16, device=dev)
    _rows_move(dev, src, 16, empty, dst, 16, 16, 1)
    _rows_move(dev, src, 16, empty, dst, 16, 16, 0)
    assert bool((dst == 0x5A5A).all())
    # more chunks than the grid's threads
    n, W = 70000, 128
    assert n * (W * 2 // 16) > 4096 * 256
    src = _bits(n, W, torch.bfloat16, g)
    idx = torch.randperm(n, generator=g)
    idx[torch.randperm(n, generator=g)[:1000]] = -1
    want = src[idx.clamp(min=0)].clone()
    want[idx < 0] = 0
    idx_d = idx.to(torch.int32).to(dev)
    got = K.rows_gather(src.to(dev).view(torch.bfloat16), idx_d)
    assert torch.equal(got.view(torch.int16).cpu(), want)
    dst = torch.full((n, W), 0x5A5A, dtype=torch.int16)
    want = dst.clone()
    want[idx[idx >= 0]] = src[idx >= 0]
    dst_d = dst.to(dev)
    _rows_move(dev, src.to(dev), W * 2, idx_d, dst_d, W * 2, W * 2, 1)
    assert torch.equal(dst_d.cpu(), want)


# ------------------------------------------------------------------ 3. lthm_pad_prefix_sum
def _pp_from_ref(dev, m):
    """PadPrefix over the restatement's maps: a test of the sum or of attention does not
    depend on the map kernels."""
    from recommendations_amd.pad_prefix import PadPrefix
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)  # noqa: E731
    return PadPrefix(m.B, m.T, m.P, m.owner, i32(m.npad), i32(m.pof), i32(m.pof_x), i32(m.fop))


def _npad_pattern(kind, B, T, rng):
    if kind == "P0":
        return [0] * B
    npad = rng.integers(0, T + 1, size=B)
    if kind == "Pfull":
        npad[rng.integers(0, B)] = T  # P = Tp - 1
    elif B > 1:
        npad[npad == T] = T - 1      # mixed: P < Tp - 1
    else:
        npad[0] = T - 2
    return npad.tolist()


def _sum_bound(terms, abs_terms, B, dtype):
    """|got - ref| per element: f32 summation of at most B terms in any order is within
    B 2^-23 sum |x_b| of the exact sum; a bf16 result adds half a bf16 ulp of the f32 sum s
    (round to nearest, 8 significant bits): 2^(e - 8) for 2^e <= |s| < 2^(e + 1), which is
    2^-9 |s| only at the top of a binade and 2^-8 |s| at its bottom."""
    e32 = B * 2.0 ** -23 * abs_terms
    if dtype == torch.bfloat16:
        s = (terms.abs() + e32).clamp(min=2.0 ** -126)
        return e32 + torch.exp2(torch.floor(torch.log2(s)) - 8)
    return e32


def _assert_within(got, want, bound, what):
    err = (got.double() - want).abs()
    assert bool(torch.isfinite(got).all()), what
    over = err > bound
    assert not bool(over.any()), (what, int(over.sum()), float((err - bound).max()))
    # recorded as the largest error in units of its bound
    check(what, float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0, 1.0 + 1e-12)


@gpu
@pytest.mark.parametrize("kind", ["mixed", "P0", "Pfull"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("W", [8, 136, 2056])
@pytest.mark.parametrize("B", [1, 32, 33, 70])
def test_chain_sum_vs_fp64(dev, B, W, dtype, kind):
    """PadPrefix.chain_sum as the attention backward calls it (src [B, P + 1, ld] with ld > W,
    dst a column-offset view with a wider row stride) and PadPrefix.reduce, every element
    against the fp64 sum of the definition.  The source rows of sequences with npad[b] < p and
    the source columns past W are NaN, the destination is sentinel-filled: rows past P and
    columns outside the view must keep it."""
    T = 6
    rng = np.random.default_rng(B * 1000 + W + (dtype == torch.bfloat16))
    m = RefMaps(mask_from_npad(_npad_pattern(kind, B, T, rng), T))
    assert {"P0": m.P == 0, "Pfull": m.P == m.Tp - 1, "mixed": m.P < m.Tp - 1}[kind]
    pp = _pp_from_ref(dev, m)
    g = torch.Generator().manual_seed(B + W)
    R = m.P + 1
    live = torch.from_numpy(np.arange(R)[None, :] <= m.npad[:, None])         # [B, R]: b contributes to row p
    src = torch.randn(B, R, W + 8, generator=g).to(dtype)
    src[:, :, W:] = float("nan")
    src[~live] = float("nan")
    x = torch.where(live[:, :, None], src[:, :, :W].double(), torch.zeros((), dtype=torch.float64))
    want, wabs = x.sum(0), x.abs().sum(0)
    sent = -1024.0  # exact in bf16
    dst = torch.full((m.M, W + 16), sent, dtype=dtype)
    dst_d = dst.to(dev)
    pp.chain_sum(src.view(B * R, W + 8).to(dev)[:, :W], W, R, dst_d[:, 8:8 + W])
    got = dst_d.cpu()
    assert bool((got[:, :8] == sent).all()) and bool((got[:, 8 + W:] == sent).all()) and bool((got[R:] == sent).all())
    _assert_within(got[:R, 8:8 + W], want, _sum_bound(want, wabs, B, dtype), f"chain_sum / bound {dtype}")
    # reduce: the adjoint of unpack on full rows [B Tp, W]
    full = torch.randn(B * m.Tp, W, generator=g).to(dtype)
    red = pp.reduce(full.to(dev)).cpu()
    assert tuple(red.shape) == (m.M, W)
    assert torch.equal(red[R:].view(_INT[dtype]), full[torch.from_numpy(m.fop[R:])].view(_INT[dtype]))
    fx = full.view(B, m.Tp, W)[:, :R].double() * live[:, :, None]
    _assert_within(red[:R], fx.sum(0), _sum_bound(fx.sum(0), fx.abs().sum(0), B, dtype), f"reduce / bound {dtype}")


@gpu
def test_chain_sum_backward_call_form(dev):
    """The call attn_bwd_qkv makes: W = 2C columns of a contiguous [B (P + 1), 2C] bf16 chain
    buffer into dqkv[:, C:] (row stride 3C): dq's columns and the rows past the chain keep
    their values."""
    T, C = 40, 64
    m = RefMaps(mask_from_npad([0, 33, 40, 7, 40, 32, 1], T))
    pp = _pp_from_ref(dev, m)
    R = m.P + 1
    g = torch.Generator().manual_seed(4)
    live = torch.from_numpy(np.arange(R)[None, :] <= m.npad[:, None])
    chain = bf(torch.randn(m.B, R, 2 * C, generator=g))
    chain[~live] = float("nan")
    dqkv = bf(torch.randn(m.M, 3 * C, generator=g))
    dqkv_d = dqkv.to(dev)
    pp.chain_sum(chain.view(m.B * R, 2 * C).to(dev), 2 * C, R, dqkv_d[:, C:])
    got = dqkv_d.cpu()
    assert torch.equal(got[:, :C].view(torch.int16), dqkv[:, :C].view(torch.int16))
    assert torch.equal(got[R:].view(torch.int16), dqkv[R:].view(torch.int16))
    x = chain.double() * live[:, :, None]
    x[~live] = 0.0
    _assert_within(got[:R, C:], x.sum(0), _sum_bound(x.sum(0), x.abs().sum(0), m.B, torch.bfloat16),
                   "chain_sum into dqkv[:, C:] / bound")


# ------------------------------------------------------------------ 4. packed attention
def _edge_npad(T):
    """Pad counts just before, on and after the two first 32-row tile edges (position p is a
    chain row for p <= npad, so npad = 31 makes tile 0 all pads), one valid row, and none: the
    fully padded row once as the chain's owner and once not."""
    return [0, 30, T, 31, 32, 63, 64, T - 1, T]


_LIMIT = {}


def _packed_limit():
    """the largest T' the packed-row attention kernels take at E = 64 (host-only probe)"""
    if not _LIMIT:
        from recommendations_amd._lib import load
        lib = load()
        ok = [t for t in range(257, 1025) if lib.lthm_attn_packed_ok(t, 64)]
        assert ok and ok == list(range(257, ok[-1] + 1)) and ok[-1] > 300
        _LIMIT["T"] = ok[-1]
    return _LIMIT["T"]


# bounds: ~2x the largest error measured over the slices of the cases below on an MI355X (out
# 1.6e-4, dq 3.0e-3, dk 3.1e-3, dv 3.0e-3, the largest on one-row slices where nothing averages
# the bf16 rounding of the stored gradient; dtable 7.6e-4; lse 1.2e-6 absolute; dtable against
# the unpacked run 1.3e-7, held to 1e-6 because the order of the LDS float atomics behind it
# is not fixed from run to run), inside the kernels' own 1e-3 (forward) / 1e-2 (gradients)
ATTN_BOUND = {"out": 3.5e-4, "dq": 6e-3, "dk": 6.5e-3, "dv": 6e-3, "dtable": 1.6e-3, "lse": 4e-6,
              "dtable_unpacked": 1e-6}


def _slice_check(what, got, want, bound):
    if want.numel() == 0:
        return
    if float(want.norm()) == 0.0:  # softmax over one key: exactly zero gradients
        assert float(got.abs().max()) < 1e-4, what
    else:
        check(what, relerr(got, want), bound)


@gpu
@pytest.mark.parametrize("Tp,H,table,p0", [(257, 1, True, False), (288, 2, True, False), (300, 1, True, False),
                                           (300, 2, True, False), ("max", 1, True, False), ("max", 2, True, False),
                                           (300, 1, False, False), (257, 2, True, True)])
def test_packed_attention_vs_oracle(dev, Tp, H, table, p0):
    """attn_fwd_qkv / attn_bwd_qkv on packed rows (attn_fwd32_k and attn_bwd32l_k reading
    through row_map / live_map, dK / dV of chain keys through the chain buffer and
    lthm_pad_prefix_sum) against oracle/ref.sdpa under pack . f . unpack in fp64, per slice: the
    chain rows, and each sequence's valid rows on their own.  ``max``: the largest T' the packed
    kernels take.  Then against the same kernels with no maps on the unpacked rows: the packed
    mode changes addressing and skips tiles whose contribution is an exact zero, so the owned
    rows of out / lse / dq and the non-chain rows of dk / dv are equal bit for bit."""
    from recommendations_amd import kernels as K
    E = 64
    if Tp == "max":
        Tp = _packed_limit()
    assert K.attn_packed_ok(Tp, E)
    T, C = Tp - 1, H * E
    npad = [0, 0, 0] if p0 else _edge_npad(T)
    m = RefMaps(mask_from_npad(npad, T))
    check_map_invariants(m)
    pp = _pp_from_ref(dev, m)
    B, M, R = m.B, m.M, m.P + 1
    g = torch.Generator().manual_seed(Tp * 7 + H)
    qkv = bf(torch.randn(M, 3 * C, generator=g))
    tab = 0.5 * torch.randn(2 * Tp + 5, H, generator=g) if table else None
    dout = bf(torch.randn(M, C, generator=g))
    tab_d = None if tab is None else tab.to(dev)
    qkv_d, dout_d = qkv.to(dev), dout.to(dev)
    out, lse = K.attn_fwd_qkv(qkv_d, B, Tp, H, E, tab_d, True, pack=pp)
    dqkv, dtab = K.attn_bwd_qkv(qkv_d, out, dout_d, lse, B, Tp, H, E, tab_d, True, pack=pp)
    # the same kernels, no maps, on the unpacked rows
    qkv_f = K.rows_gather(qkv_d, pp.pof)
    out_f, lse_f = K.attn_fwd_qkv(qkv_f, B, Tp, H, E, tab_d, True)
    dqkv_f, dtab_f = K.attn_bwd_qkv(qkv_f, out_f, K.rows_gather(dout_d, pp.pof_x), lse_f, B, Tp, H, E, tab_d, True)
    torch.cuda.synchronize()
    out, lse, dqkv, out_f, lse_f, dqkv_f = (t.cpu() for t in (out, lse, dqkv, out_f, lse_f, dqkv_f))

    # ---- fp64 oracle
    qp = qkv.double().requires_grad_(True)
    tp = None if tab is None else tab.double().requires_grad_(True)
    exp = packed_apply(lambda x: attn_full(x, H, tp), qp, m)
    exp.backward(dout.double())
    exp = exp.detach()
    want = {"out": bf(exp).double(), "dq": qp.grad[:, :C], "dk": qp.grad[:, C:2 * C], "dv": qp.grad[:, 2 * C:]}
    got = {"out": out.double(), "dq": dqkv[:, :C].double(), "dk": dqkv[:, C:2 * C].double(),
           "dv": dqkv[:, 2 * C:].double()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    tag = f"T'={Tp} H={H}"
    for name in ("out", "dq", "dk", "dv"):
        _slice_check(f"packed attn {name} chain rows {tag}", got[name][m.chain_rows()], want[name][m.chain_rows()],
                     ATTN_BOUND[name])
        for b in range(B):
            rows = m.valid_rows(b)
            _slice_check(f"packed attn {name} seq {b} (npad {npad[b]}) {tag}", got[name][rows], want[name][rows],
                         ATTN_BOUND[name])
    if tab is not None:
        _slice_check(f"packed attn dtable {tag}", dtab.cpu().double(), tp.grad[: 2 * Tp + 1], ATTN_BOUND["dtable"])
    else:
        assert dtab is None
    # lse of every row in a tile the kernel runs (the backward reads them)
    lse_ref = lse_full(qkv.double()[torch.from_numpy(m.pof)].view(B, Tp, 3 * C), H, None if tab is None else tab.double())
    for b in range(B):
        q0 = 32 * m.first_live_tile(b)
        assert bool(torch.isfinite(lse[b]).all())
        if q0 < Tp:
            err = float((lse[b, :, q0:].double() - lse_ref[b, :, q0:]).abs().max())
            check(f"packed attn lse seq {b} (npad {npad[b]}) {tag}", err, ATTN_BOUND["lse"])

    # ---- bit equality with the unpacked run
    fop = torch.from_numpy(m.fop)
    i16 = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    assert torch.equal(i16(out), i16(out_f[fop])), "out: packed vs unpacked"
    assert torch.equal(i16(dqkv[:, :C]), i16(dqkv_f[fop, :C])), "dq: packed vs unpacked"
    assert torch.equal(i16(dqkv[R:, C:]), i16(dqkv_f[fop[R:], C:])), "dk / dv past the chain: packed vs unpacked"
    own = torch.from_numpy(m.pof_x.reshape(B, Tp) >= 0)[:, None, :].expand(B, H, Tp)
    assert torch.equal(lse[own].view(torch.int32), lse_f[own].view(torch.int32)), "lse: packed vs unpacked"
    if tab is not None:  # LDS float atomics: summation order only
        check(f"packed attn dtable vs unpacked {tag}", relerr(dtab, dtab_f), ATTN_BOUND["dtable_unpacked"])


# ------------------------------------------------------------------ 5. the block, both branches
def _packed_block_oracle(sd, xp, dyp, H, m):
    """oracle/ref.transformer_block with the HIP path's bf16 rounding points (as
    test_gpu_encoder._block_oracle), double residual, under pack . f . unpack."""
    p = {k: v.detach().cpu().float().clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    xr = xp.detach().cpu().float().clone().requires_grad_(True)
    y = packed_apply(lambda full: ref.transformer_block(full, p, H, True, bf16=True) + full, xr, m)
    y.backward(dyp.detach().cpu().float())
    return y.detach(), xr.grad, {k: v.grad for k, v in p.items()}


@gpu
@pytest.mark.parametrize("case", ["unpack_49", "packed_300", "unpack_past_limit"])
def test_block_packed_branches_vs_bf16_oracle(dev, case):
    """TransformerBlock.forward_double_residual(xp, pack=pp) (d = 128, H = 2, E = 64) against
    the bf16-mirrored oracle under pack . f . unpack, at T' = 49 (attn_packed_ok false: the
    unpack / unpack_owner / reduce fallback), T' = 300 (the packed kernels) and the first T'
    past the packed kernels' limit (the fallback again, with the windowed backward).  The
    block's own bounds, the output and dx over the chain rows and the valid rows separately."""
    from test_gpu_encoder import _rand_block
    from recommendations_amd import kernels as K
    d, H = 128, 2
    if case == "unpack_49":
        Tp, packed = 49, False
        npad = [0, 30, 48, 31, 32, 47, 48, 5]
    elif case == "packed_300":
        Tp, packed = 300, True
        npad = _edge_npad(Tp - 1)
    else:
        Tp, packed = _packed_limit() + 1, False
        npad = [31, Tp - 1, 64, Tp - 1]
    assert K.attn_packed_ok(Tp, d // H) == packed
    m = RefMaps(mask_from_npad(npad, Tp - 1))
    pp = _pp_from_ref(dev, m)
    blk, sd, _, _ = _rand_block(dev, 1, Tp, d, H, seed=Tp)
    g = torch.Generator().manual_seed(Tp)
    xp = torch.randn(m.M, d, generator=g)
    dyp = torch.randn(m.M, d, generator=g) / math.sqrt(m.M * d)
    xd = xp.to(dev).requires_grad_(True)
    y = blk.forward_double_residual(xd, pack=pp)
    assert tuple(y.shape) == (m.M, d)
    yr, dxr, gr = _packed_block_oracle(sd, xp, dyp, H, m)
    y.backward(dyp.to(dev))
    yc, dx = y.detach().cpu(), xd.grad.cpu()
    for name, rows in (("chain rows", m.chain_rows()), ("valid rows", slice(m.P + 1, m.M))):
        check(f"{case} block fwd {name}", relerr(yc[rows] - 2 * xp[rows], yr[rows] - 2 * xp[rows]), 1e-3)
        check(f"{case} block dx {name}", relerr(dx[rows], dxr[rows]), 1e-2)
    for n, p in blk.named_parameters():
        check(f"{case} block d{n}", relerr(p.grad, gr[n]), 1e-2)
