"""The checker of the retrieval-cursor tests (test_retrieval_after_host.py pins it on the CPU,
test_gpu_retrieval_after.py holds the kernels to it): tags_checker of retrieval_tags_case.py plus
the eligibility rule of a cursor (after_score f32, after_row int32) per query or user,

    row j is eligible  iff  s_j < after_score  or  (s_j == after_score and j > after_row),

applied in f32: the cursor is an f32 and the scores are rounded to f32 first, so that equality
means what the kernel means by it (and -0 == +0, NaN compares false with everything).  A row that
is not eligible is -inf like an excluded or filtered row: it takes no slot and does not count in
the rank; the target's own score stays the plain (best-over-heads) dot."""
import numpy as np

from retrieval_exclude_case import valid_rows
from retrieval_tags_case import eligible


def after_eligible(s, after_score, after_row):
    """s [U, N] scores, after_score [U], after_row [U] -> bool [U, N], the rule above in f32."""
    s32 = np.asarray(s).astype(np.float32)
    cs = np.asarray(after_score, dtype=np.float32)[:, None]
    cr = np.asarray(after_row).astype(np.int64)[:, None]
    j = np.arange(s32.shape[1], dtype=np.int64)[None, :]
    with np.errstate(invalid="ignore"):
        return (s32 < cs) | ((s32 == cs) & (j > cr))


def after_checker(q_bf, items_bf, k, after_score=None, after_row=None, tags=None, filt=None, excl=None, trow=None):
    """q_bf [Q, 128] or [U, G, 128] and items_bf [N, 128]: the bf16 operands; after_score [U] and
    after_row [U], or both None (no cursor); tags [N] and filt [U, 3], or both None; excl [U, X] or
    None; trow [U] or None.  Returns the fp64 best-over-heads scores s [U, N], the same with -inf
    at every row that is ineligible for any reason, the expected (scores f32 [U, k], rows int32
    [U, k]), rank int32 [U] and target_score f32 [U] (or None).  k may be any positive number: the
    expected list is the first k rows of the full order."""
    if q_bf.dim() == 2:
        q_bf = q_bf[:, None, :]
    U, G, D = q_bf.shape
    sg = (q_bf.double().reshape(U * G, D) @ items_bf.double().T).numpy().reshape(U, G, -1)
    s = sg.max(axis=1)
    N = s.shape[1]
    masked = s.copy()
    if after_score is not None:
        masked[~after_eligible(s, after_score, after_row)] = -np.inf
    if tags is not None:
        masked[~eligible(tags, filt)] = -np.inf
    if excl is not None:
        for u in range(U):
            masked[u, valid_rows(excl[u], N)] = -np.inf
    rows = np.full((U, k), -1, dtype=np.int32)
    sc = np.full((U, k), -np.inf, dtype=np.float32)
    ar = np.arange(N)
    for u in range(U):
        order = np.lexsort((ar, -masked[u]))
        order = order[masked[u, order] > -np.inf][:k]
        rows[u, :len(order)] = order
        sc[u, :len(order)] = s[u, order].astype(np.float32)
    rank = tscore = None
    if trow is not None:
        rank = np.full(U, -1, dtype=np.int32)
        tscore = np.full(U, -np.inf, dtype=np.float32)
        for u in range(U):
            t = int(trow[u])
            if 0 <= t < N:  # strict: the target never counts itself, nor does a row at -inf
                rank[u] = int((np.delete(masked[u], t) > s[u, t]).sum())
                tscore[u] = np.float32(s[u, t])
    return s, masked, sc, rows, rank, tscore
