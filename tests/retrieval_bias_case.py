"""The checker of the score-prior retrieval tests (test_retrieval_bias_host.py pins it on the CPU,
test_gpu_retrieval_bias.py holds the kernels to it).  With bf16 operands q and items, an f32 bias
per catalogue row and an f32 weight per query (user),

    s[u, j] = max_g (q[u, g] . items[j]) + w[u] * bias[j]          in fp64,

the value the kernel's f32 fma(w, bias, dot) rounds.  Everything downstream sees s and only s:
the order (score descending, row ascending), the cursor rule of retrieval_after_case.py (applied
to s rounded to f32), the rank, and the target's own score, which is biased like every other row
and never excluded or filtered as a target.  A row that is excluded, filtered or not behind the
cursor is -inf: it takes no slot and does not count."""
import numpy as np

from retrieval_after_case import after_eligible
from retrieval_exclude_case import valid_rows
from retrieval_tags_case import eligible


def bias_scores(q_bf, items_bf, bias=None, w=None):
    """fp64 [U, N]: the best-over-heads dot plus w[u] * bias[j] (w None: 1; bias None: no prior)."""
    if q_bf.dim() == 2:
        q_bf = q_bf[:, None, :]
    U, G, D = q_bf.shape
    sg = (q_bf.double().reshape(U * G, D) @ items_bf.double().T).numpy().reshape(U, G, -1)
    s = sg.max(axis=1)
    if bias is not None:
        wv = np.ones(U) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64).reshape(U)
        s = s + wv[:, None] * np.asarray(bias, dtype=np.float32).astype(np.float64)[None, :]
    return s


def bias_checker(q_bf, items_bf, k, bias=None, w=None, after_score=None, after_row=None, tags=None, filt=None,
                 excl=None, trow=None, eps=0.0):
    """q_bf [Q, 128] or [U, G, 128] and items_bf [N, 128]: the bf16 operands; bias f32 [N] or None;
    w f32 [U] or None (1); after_score / after_row [U] or both None; tags [N] and filt [U, 3] or both
    None; excl [U, X] or None; trow [U] or None.  Returns a dict:
      s       fp64 [U, N] biased scores          masked  the same, -inf at every ineligible row
      scores  f32 [U, k], rows int32 [U, k]      the first k of the order, -inf / -1 behind it
      rank    int32 [U], tscore f32 [U]          (None without trow): the hit position, the number
              of eligible rows other than the target scoring strictly above the target's biased score
      near    near[u][i]: the rows whose masked score is within eps of the i-th expected score
              (with eps = 0 the tie run of that rank)."""
    s = bias_scores(q_bf, items_bf, bias, w)
    U, N = s.shape
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
    near = []
    ar = np.arange(N)
    for u in range(U):
        order = np.lexsort((ar, -masked[u]))
        order = order[masked[u, order] > -np.inf][:k]
        rows[u, :len(order)] = order
        sc[u, :len(order)] = s[u, order].astype(np.float32)
        near.append([set(np.nonzero(np.abs(masked[u] - s[u, j]) <= eps)[0].tolist()) for j in order])
    rank = tscore = None
    if trow is not None:
        rank = np.full(U, -1, dtype=np.int32)
        tscore = np.full(U, -np.inf, dtype=np.float32)
        for u in range(U):
            t = int(trow[u])
            if 0 <= t < N:  # strict: the target never counts itself, nor does a row at -inf
                rank[u] = int((np.delete(masked[u], t) > s[u, t]).sum())
                tscore[u] = np.float32(s[u, t])
    return dict(s=s, masked=masked, scores=sc, rows=rows, rank=rank, tscore=tscore, near=near)
