"""LTHMModelWrapper — drop-in for models/lthm/sequence/wrapper.py:16-275.

Same BaseModelWrapper surface: ``forward(batch) -> dict``, ``train_step``,
``val_step``, ``optim_group``, ``optimizers_for_param_groups``.  The loss of
``_mini_batch_mapper`` + ``_train_or_val_step_helper`` (wrapper.py:78-245) is
one fused op over all mini-batches (``ContrastiveLossFn``, csrc/loss.hip):
identical math per 32-sequence mini-batch and lookahead head, with the
lookahead offsets drawn per mini-batch exactly as wrapper.py:147-153 does
(from a seeded ``random.Random`` instead of the global ``random``).

Bug resolutions: #11 ``self._model_config`` -> ``self.model_config``;
#12 ``current_token_id`` -> ``current_token_ids``; #13 ``sparse`` /
``log_q_config`` / ``loss_type`` declared in the config.  The logQ streaming
estimates are trained on every helper call whatever beta is, as in the reference
(wrapper.py:131-136); the correction enters the loss kernels only when
``log_q_config.beta != 0`` (the shipped YAML has beta = 0, where it is exactly zero).
``train_step`` / ``val_step`` return ``(loss, metrics)`` with the reference's metric
dict (``StepMetrics``: materialised from the device statistics on first read).
"""
from __future__ import annotations

import ctypes
import os
import random
from collections.abc import MutableMapping
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from .... import kernels as K
from ...._lib import STRUCTS, TIMER_RECORDS, call, dcode, load, ptr, stream, sub_events, timer_on
from ....commons.base_model_wrapper import BaseModelWrapper
from ....commons.layers import CascadedStreamingLogQCorrectionModule
from ....optim import FusedAdamW, SparseRowAdamW
from .encoder import Encoder

NSTAT_BASE = 8  # csrc/loss.hip CL_NSTAT: stats before hits@k
LOSS_DE = 128  # operand width the loss kernels are compiled for (csrc/loss.hip DE)
_KS_DEV: Dict[tuple, torch.Tensor] = {}  # (metric ks, device) -> int32 device copy


class ContrastiveLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, target, mask, offsets_dev, cfg, logq=None):
        """y [B, T+1, NH, De] (next_token_emb), target [B, T, De] (current_token_emb),
        mask [B, T] uint8 (row stride = mask.stride(0)), offsets_dev int32 [n_mb, NH];
        logq: None or f32 [B, T], the additive logit correction -beta * logQ of each input token."""
        B, Tp, NH, De = y.shape
        T = Tp - 1
        mbs, tau, ks = cfg["mb"], cfg["tau"], cfg["ks"]
        n_mb = (B + mbs - 1) // mbs
        n_max = ((mbs * T + 63) // 64) * 64
        dev = y.device
        yc = y.contiguous()
        tc = target.contiguous()
        rows = (ctx.needs_input_grad[0] and not _OLD_BWD and not _NO_FUSED_ROWS and logq is None
                and 2.0 / tau <= 80.0 and mbs <= 4096 and yc.dtype in (torch.bfloat16, torch.float32))
        if rows and not _NO_VC:
            # the compact path's gather normalises the `out` rows it reads (their norms into ynorm)
            yn, ynorm = None, torch.empty(B * Tp * NH, dtype=torch.float32, device=y.device)
        else:
            yn, ynorm = K.rownorm(yc.view(-1, De))
        # pad positions of `in` are zero rows: every logit against them is excluded
        # anyway, and the loss kernels then need no per-element pad test
        tn, tnorm = K.rownorm(tc.view(-1, De), row_mask=mask)
        f32 = dict(dtype=torch.float32, device=dev)
        lse = torch.empty((NH, n_mb, n_max), **f32)
        pos = torch.empty((NH, n_mb, n_max), **f32)
        diag = torch.empty((NH, n_mb, n_max), **f32)
        w = torch.empty((NH, n_mb, n_max), **f32)
        cnt = torch.empty((NH, n_mb, n_max), dtype=torch.int32, device=dev)
        rank = torch.empty((NH, n_mb, n_max), dtype=torch.int32, device=dev)
        nstat = NSTAT_BASE + len(ks)
        stats = torch.empty((NH, n_mb, nstat), **f32)
        ks_dev = _KS_DEV.get((tuple(ks), dev))  # uploaded once per (ks, device), not per step
        if ks_dev is None:
            ks_dev = _KS_DEV[(tuple(ks), dev)] = torch.tensor(ks, dtype=torch.int32).to(dev)
        lqc = torch.empty((NH, n_mb, n_max), **f32) if logq is not None else None
        # every head in one set of launches (head h's buffers at h * n_mb * n_max)
        d = ContrastiveLossFn._desc(yn, tn, mask, B, T, NH, 0, De, mbs, n_mb, n_max, tau, offsets_dev,
                                    lse[0], pos[0], cnt[0], rank[0], diag[0], w[0], logq,
                                    None if lqc is None else lqc[0])
        d.heads_run, d.head_stride = NH, n_mb * n_max
        wsb = load().lthm_contrastive_ws_bytes(n_mb, n_max, NH)
        ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev)
        d.stats_ws, d.stats_ws_bytes = ptr(ws), ws.numel() * 8
        # training at the fixed shift: the forward also runs the row side of the backward and
        # writes dy (unit upstream gradient) -- one S pass instead of the forward's plus ROWS'
        dy = None
        vc = None
        if rows:
            dy = torch.empty_like(yc)
            d.y_raw, d.y_norm, d.dy, d.y_dtype = ptr(yc), ptr(ynorm), ptr(dy), dcode(yc)
            if not _NO_VC:
                # valid-row compaction: the S passes run over the non-pad indices only (the
                # workspace is shared with this forward's backward)
                vc = torch.empty(load().lthm_contrastive_vc_ws_bytes(B, T, NH, mbs, n_mb, n_max),
                                 dtype=torch.uint8, device=dev)
                d.vc_ws, d.vc_ws_bytes = ptr(vc), vc.numel()
        # algorithmic work: 2 n^2 De per head (S); with the row side also dS . in (2 n^2 De); with
        # the compaction n is the valid count m of each (mini-batch, head), read after the step
        work = (2.0 if rows else 1.0) * float(sum(cfg["flops"]))
        ev = sub_events("cl_fr32_k" if rows else "cl_fwd_main", work, "flop")
        if ev is not None:  # the fused pass alone, timed inside the call (bench.py's roofline kernel)
            d.main_ev0, d.main_ev1 = ev[0].cuda_event, ev[1].cuda_event
        call("lthm_contrastive_fwd", ctypes.addressof(d), ptr(stats), nstat, ptr(ks_dev), len(ks),
             1.0 / n_mb, stream(), _key="cl_fwd_k", _work=work, _unit="flop")
        if vc is not None and timer_on():
            # the timer's work of both compact passes: 2 x 2 m^2 De per (mini-batch, head); kept
            # for the backward's record also when this forward's passes are not timed
            mv = vc[:NH * n_mb * 4].view(torch.int32).clone()
            vwork = lambda: 4.0 * De * float((mv.double() ** 2).sum())  # noqa: E731
            want = {"cl_fr32_k", "cl_fwd_k"}  # this call's two records, the latest of their keys
            for rec in reversed(TIMER_RECORDS()):
                if rec[0] in want:
                    rec[3] = vwork
                    want.discard(rec[0])
                    if not want:
                        break
            cfg["vc_work"] = vwork
        # loss = sum_mb sum_heads mean-CE / n_mb  (wrapper.py:109-111)
        loss = torch.empty(1, **f32)
        call("lthm_colsum", ptr(stats), 0, NH * n_mb, 1, nstat, ptr(loss), 0, stream())
        loss = loss / n_mb
        ctx.save_for_backward(yc, tc, yn, tn, ynorm, tnorm, lse, w, diag, mask, offsets_dev, logq, lqc, dy)
        ctx.vc = vc
        ctx.vc_work = cfg.get("vc_work")
        ctx.meta = (B, T, NH, De, mbs, n_mb, n_max, tau)
        ctx.stats = stats
        cfg.get("stats_out", []).append(stats)
        cfg.get("rows_out", []).append((lse, pos, cnt, rank))  # the per-row outputs, for the tests
        ctx.flops = cfg["flops"]
        return loss

    @staticmethod
    def _desc(yn, tn, mask, B, T, NH, h, De, mbs, n_mb, n_max, tau, offsets_dev, lse, pos, cnt, rank, diag, w,
              logq=None, lqc=None):
        d = STRUCTS["lthm_contrastive_desc"]()
        if logq is not None:
            d.logq, d.logq_stride, d.logq_col = ptr(logq), logq.stride(0), ptr(lqc)
        d.out_n, d.in_n, d.mask, d.mask_stride = ptr(yn), ptr(tn), ptr(mask), mask.stride(0)
        d.B, d.T, d.n_heads, d.head, d.De = B, T, NH, h, De
        d.mb_size, d.n_mb, d.n_max, d.tau = mbs, n_mb, n_max, tau
        d.offsets = ptr(offsets_dev)
        d.lse, d.pos, d.cnt, d.rank, d.diag, d.w = ptr(lse), ptr(pos), ptr(cnt), ptr(rank), ptr(diag), ptr(w)
        return d

    @staticmethod
    def backward(ctx, dloss):
        yc, tc, yn, tn, ynorm, tnorm, lse, w, diag, mask, offsets_dev, logq, lqc, dy_f = ctx.saved_tensors
        B, T, NH, De, mbs, n_mb, n_max, tau = ctx.meta
        g = dloss.contiguous().float()
        if _OLD_BWD:
            return ContrastiveLossFn._backward_per_head(ctx, g)
        # every head in one call: the ROWS kernel writes dy per head through F.normalize (or the
        # forward already did: rows_done, dy scaled by g here), the COLS kernel sums dIn over the
        # six heads on chip and writes dt once through F.normalize
        if dy_f is not None and getattr(ctx, "dy_consumed", False):
            # a second backward through this graph (retain_graph): the first one scaled the
            # forward's dy in place and returned it, so run the ROWS side again into a fresh dy
            dy_f = None
        if yn is None and dy_f is None:  # the full passes read every normalised `out` row
            yn, ynorm = K.rownorm(yc.view(-1, De))
        if dy_f is not None:
            ctx.dy_consumed = True
        dy = dy_f if dy_f is not None else torch.empty_like(yc)
        dt = torch.empty_like(tc)
        d = ContrastiveLossFn._desc(yn, tn, mask, B, T, NH, 0, De, mbs, n_mb, n_max, tau, offsets_dev,
                                    lse[0], None, None, None, diag[0], w[0],  # diag: shift scratch
                                    logq, None if lqc is None else lqc[0])
        d.heads_run, d.head_stride = NH, n_mb * n_max
        d.gscale = ptr(g)
        d.y_raw, d.y_norm, d.dy, d.y_dtype = ptr(yc), ptr(ynorm), ptr(dy), dcode(yc)
        d.t_raw, d.t_norm, d.dt, d.t_dtype = ptr(tc), ptr(tnorm), ptr(dt), dcode(tc)
        d.rows_done = 1 if dy_f is not None else 0
        vw = None
        if dy_f is not None and ctx.vc is not None:  # the forward's compact index lists and images
            d.vc_ws, d.vc_ws_bytes = ptr(ctx.vc), ctx.vc.numel()
            vw = ctx.vc_work
        if dy_f is not None:  # the columns pass alone: S recompute + dS^T . out, 4 n^2 De per head
            ev = sub_events("cl_bwd32_k", vw or 2.0 * float(sum(ctx.flops)), "flop")
            if ev is not None:
                d.main_ev0, d.main_ev1 = ev[0].cuda_event, ev[1].cuda_event
        # algorithmic work per head: one S recompute + dS^T . out (2 x 2 n^2 De) with the row side
        # done in the forward; else also dS . in (3 x; the ROWS and COLS kernels each recompute S)
        call("lthm_contrastive_bwd", ctypes.addressof(d), stream(), _key="cl_bwd_k",
             _work=vw or (2.0 if dy_f is not None else 3.0) * float(sum(ctx.flops)), _unit="flop")
        return dy, dt, None, None, None, None

    @staticmethod
    def _backward_per_head(ctx, g):
        """The round-2 backward (16x16x32 kernels, one call per head, f32 d_in read-modify-written
        per head); kept behind LTHM_CL_BWD_OLD=1 for A/B measurements."""
        yc, tc, yn, tn, ynorm, tnorm, lse, w, diag, mask, offsets_dev, logq, lqc, _ = ctx.saved_tensors
        B, T, NH, De, mbs, n_mb, n_max, tau = ctx.meta
        dev = yc.device
        fuse = yc.dtype == torch.bfloat16
        dy = torch.empty_like(yc) if fuse else None
        d_out = None if fuse else torch.empty((B, T + 1, NH, De), dtype=torch.float32, device=dev)
        d_in = K.zeros((B, T, De), torch.float32, dev)
        for h in range(NH):
            d = ContrastiveLossFn._desc(yn, tn, mask, B, T, NH, h, De, mbs, n_mb, n_max, tau, offsets_dev,
                                        lse[h], None, None, None, diag[h], w[h], logq, None if lqc is None else lqc[h])
            d.gscale, d.d_out, d.d_in = ptr(g), ptr(d_out), ptr(d_in)
            if fuse:
                d.y_raw, d.y_norm, d.dy, d.y_dtype = ptr(yc), ptr(ynorm), ptr(dy), dcode(yc)
            call("lthm_contrastive_bwd", ctypes.addressof(d), stream(), _key="cl_bwd_k",
                 _work=3.0 * ctx.flops[h], _unit="flop")
        if not fuse:
            dy, _ = K.rownorm_bwd(yc.view(-1, De), ynorm, d_out.view(-1, De))
        dt, _ = K.rownorm_bwd(tc.view(-1, De), tnorm, d_in.view(-1, De))
        return dy.view(yc.shape), dt.view(tc.shape), None, None, None, None


_OLD_BWD = os.environ.get("LTHM_CL_BWD_OLD") == "1"
_NO_FUSED_ROWS = os.environ.get("LTHM_CL_NO_FUSED_ROWS") == "1"  # A/B: separate forward and ROWS passes
_NO_VC = os.environ.get("LTHM_CL_VC") == "0"  # A/B: the full n x n passes (no valid-row compaction)


def contrastive_step(y, tgt, mask, offs: np.ndarray, mbs: int, tau: float, ks: List[int], logq=None):
    """All helper calls of one train / val step (wrapper.py:78-245) on the fused kernels.

    y [B, T+1, NH, De] next_token_emb, tgt [B, T, De] current_token_emb, mask [B, T] pad
    mask, offs [n_mb, NH] the lookahead offsets drawn per helper call, mbs sequences per
    helper call (B: the whole batch).  Returns the loss (mean over helper calls of the
    per-call sum over heads) and the device statistics [NH, n_mb, 8 + len(ks)]."""
    B, T = y.shape[0], y.shape[1] - 1
    n_mb = (B + mbs - 1) // mbs
    assert offs.shape[0] == n_mb, (offs.shape, n_mb)
    offsets_dev = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int32)).pin_memory().to(
        y.device, non_blocking=True)
    flops = []  # algorithmic logits flops per head: sum over mini-batches of 2 n^2 De
    for h in range(offs.shape[1]):
        tot = 0.0
        for mb in range(n_mb):
            n = min(mbs, B - mb * mbs) * max(T - int(offs[mb, h]), 0)
            tot += 2.0 * n * n * y.shape[-1]
        flops.append(tot)
    holder = []
    cfg = dict(mb=mbs, tau=tau, ks=list(ks), flops=flops, stats_out=holder)
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    loss = ContrastiveLossFn.apply(y, tgt, mask, offsets_dev, cfg, logq)
    return loss, holder[0]


class LTHMModelWrapper(BaseModelWrapper):
    def __init__(self, model_config, stats=None):
        super().__init__(dummy_params=model_config.sparse, sparse=model_config.sparse)
        self.model_config = model_config
        de = model_config.product_tower.product_emb_dim
        if de != LOSS_DE:
            # the fused loss kernels are compiled for one operand width (csrc/loss.hip DE); refuse at
            # construction instead of at the first train_step (query_tower.py:54-55, product_tower.py:37-39)
            raise ValueError(f"product_emb_dim={de} is not supported by the fused contrastive loss kernels "
                             f"(built for product_emb_dim={LOSS_DE}, model/lthm.yaml:22)")
        self._sparse = model_config.sparse
        self._softmax_temperature = model_config.softmax_temperature
        self._export_span = model_config.export_span
        self._export_tokens = model_config.export_tokens
        self._loss_type = model_config.loss_type
        self._metrics_k_all = list(model_config.metrics_k_all)
        self._lookahead = list(model_config.lookahead)
        self._model = Encoder(model_config)
        # wrapper.py:34-42 (built whatever beta is, so the state_dict carries its a / b buffers)
        lq = model_config.log_q_config
        self._log_q_beta = float(lq.beta)
        self._log_q_calc = CascadedStreamingLogQCorrectionModule(
            num_buckets=lq.num_buckets, hash_offsets=lq.hash_offsets, alpha=lq.alpha, p_init=lq.p_init)
        self.batch_idx = 0
        self._rng = random.Random(model_config.seed)
        self.last_stats = None

    # wrapper.py:48-64
    def format_inputs(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        for k in ("product_ids", "labels", "timestamp"):
            assert batch[k].dtype == torch.int64, f"{k} was expected to be of type long but was {batch[k].dtype}"
        return batch

    def forward(self, batch: Dict[str, torch.Tensor]):
        return self._model(self.format_inputs(batch))

    def prefetch(self, batch: Dict[str, torch.Tensor], ready=None) -> None:
        """Run the frozen item-table lookup of a later ``forward(batch)`` now, on a side
        stream (``Encoder.prefetch``; build-defined, the reference has no pipelining).
        ``ready``: an event recorded when ``batch``'s ids became valid."""
        self._model.prefetch(self.format_inputs(batch), ready)

    def draw_offsets(self, n_mb: int) -> np.ndarray:
        """wrapper.py:147-153, once per mini-batch: head 0 uses lookahead[0], head i
        draws randint(previous + 1, lookahead[i])."""
        out = np.zeros((n_mb, len(self._lookahead)), dtype=np.int32)
        for mb in range(n_mb):
            prev = 0
            for i, mx in enumerate(self._lookahead):
                if i == 0:
                    off = mx
                else:
                    off = self._rng.randint(prev + 1, mx)
                prev = off
                out[mb, i] = off
        return out

    def train_step(self, batch, output):
        return self._loss_and_metrics(output, training=True)

    def val_step(self, batch, output):
        return self._loss_and_metrics(output, training=False)

    def _loss_and_metrics(self, output, training: bool):
        """_mini_batch_mapper (wrapper.py:78-112): training splits the batch into
        train_mini_batch_size sequences per helper call; val_step and a negative
        train_mini_batch_size run the helper (wrapper.py:114-245) once over the whole
        batch.  Every helper call of the step runs in one fused launch set."""
        y = output["next_token_emb"]
        tgt = output["current_token_emb"]
        mask = output["current_token_mask"]
        B, Tp = y.shape[0], y.shape[1]
        T = Tp - 1
        step_type = "train" if training else "val"
        mbs = self.model_config.train_mini_batch_size
        whole = (not training) or mbs < 0
        mbs = B if whole else min(mbs, B)
        n_mb = (B + mbs - 1) // mbs
        offs = self.draw_offsets(n_mb)  # a head whose offset reaches past T has no rows (wrapper.py:157-159)
        # wrapper.py:126-130 per helper call in order, train and val alike: logQ train_step on its
        # non-pad ids, then the correction -beta * logQ of its ids (zeroed on the positive
        # in-kernel).  The streaming estimates advance whatever beta is, as the reference's do;
        # the correction enters the loss only when beta != 0 (with beta = 0 it is exactly zero)
        want = self._log_q_beta != 0.0
        logq = self._log_q_calc.stream_correction(output["current_token_ids"], mask, mbs, self.batch_idx,
                                                  self._log_q_beta, want_out=want)
        loss, stats = contrastive_step(y, tgt, mask, offs, mbs, self._softmax_temperature, self._metrics_k_all, logq)
        self.batch_idx += n_mb  # the reference counts helper calls, one per mini-batch
        self.last_stats = (stats, offs, step_type, B, T, mbs, whole)
        return loss, StepMetrics(stats, offs, step_type, self._metrics_k_all, B, T, mbs, whole)

    def metrics(self) -> Dict[str, float]:
        """Metric dict of the last train_step / val_step as a plain dict (the same values
        train_step / val_step return)."""
        if self.last_stats is None:
            return {}
        stats, offs, step_type, B, T, mbs, whole = self.last_stats
        return lthm_metrics(stats.cpu().numpy(), offs, step_type, self._metrics_k_all, B, T, mbs, whole)

    @torch.no_grad()
    def retrieve(self, batch: Dict[str, torch.Tensor], catalogue, k: int, head: int = 0,
                 exclude_history: bool = False, heads: Optional[Sequence[int]] = None,
                 tag_all=None, tag_any=None, tag_none=None, after=None,
                 bias_weight=None, nprobe: Optional[int] = None, diversity: Optional[float] = None,
                 pool: Optional[int] = None, group_cap: Optional[int] = None,
                 shortlist: Optional[int] = None, exclude_seen: bool = False) -> Dict[str, torch.Tensor]:
        """The k best catalogue items for each sequence's next event (build-defined; see
        retrieval.py): the query is ``next_token_emb[:, -1, head]``, the prediction after the
        most recent token.  Returns ``item_ids`` int64 [B, k] (0 in empty slots) and ``scores``
        f32 [B, k], sorted by (score descending, catalogue row ascending).  With
        ``exclude_history`` sequence b never gets an item of its own ``current_token_ids[b, :]``
        back (T <= 1024): the k best items it has not interacted with.  With ``heads`` (1 to 8
        distinct head indices; ``head`` is then ignored) the queries are
        ``next_token_emb[:, -1, heads]`` and an item is scored by its best match over them: the k
        items the sequence is most likely to touch at any of those lookahead offsets.  With
        ``tag_all`` / ``tag_any`` / ``tag_none`` (each an int or an int tensor [B] of 32-bit masks;
        the catalogue must carry tags) sequence b gets only items whose tag word has every
        ``tag_all`` bit, some ``tag_any`` bit and no ``tag_none`` bit: the k best items that may
        be shown.  The filter composes with ``exclude_history`` and ``heads``.  ``after`` asks for
        the next page: the dict a previous ``retrieve`` returned (its last column is the cursor)
        or ``(scores [B], item_ids [B])``; sequence b then gets the k best items strictly behind
        that position of its list, with every other argument as in the call before.  ``k`` may
        reach ``K.RETRIEVE_MAX_DEEP`` = 1024; above 128 the list still comes from a single scan
        of the catalogue.  A catalogue that carries a bias scores item j as fma(w, bias[j], q . e_j);
        ``bias_weight`` is w, None for 1, a number or f32 [B], one weight per sequence (a
        catalogue without a bias refuses it).  The scores returned are the biased ones, so
        ``after`` pages a biased list with nothing added: pass the same ``bias_weight`` again.
        A ``ClusteredItemCatalogue`` takes ``nprobe`` (1..min(L, 64)): sequence b gets the k best
        items (k <= 128) of the ``nprobe`` lists nearest to its query, by id ascending among equal
        scores; ``exclude_history`` composes, every other argument above is refused by name.  Its
        ``with_filters()`` view also takes ``tag_all`` / ``tag_any`` / ``tag_none``, ``after`` and
        ``bias_weight``, with the meaning they have on a flat catalogue, on the probed lists (pass the
        same ``nprobe`` with ``after``); it still refuses ``heads`` and k > 128.  Its ``with_deep(groups)``
        view takes k up to 1024 and ``diversity`` / ``pool`` / ``group_cap`` as a flat catalogue does, below:
        the pool is the deep list of the probed lists and the view's own ``diversify`` selects from it;
        ``heads`` it still refuses.  Its ``with_heads()`` view takes everything the ``with_filters()`` view
        takes and ``heads``: the queries are ``next_token_emb[:, -1, heads]``, sequence b probes the
        ``nprobe`` lists whose centroids score best for any of them and gets the k best items (k <= 128)
        of those lists by the best match over the heads, every item once; ``exclude_history``,
        ``tag_*``, ``bias_weight`` and ``after`` compose as on a flat catalogue, and with ``nprobe`` = L
        the result is the flat catalogue's for the same arguments.  It refuses ``diversity`` / ``pool`` /
        ``group_cap`` and k > 128: deep lists with heads take ``to_flat()``.
        ``diversity`` = lambda in [0, 1] and / or ``group_cap`` = m (alone it means lambda = 1; the
        catalogue must carry groups) ask a flat ``ItemCatalogue`` for a diversified list: the call
        retrieves ``pool`` items (default min(8 k, 1024); k <= ``pool`` <= 1024, k <= 128; above 128
        by the deep scan) exactly as above, with ``exclude_history``, ``heads``, ``tag_*`` and
        ``bias_weight`` in force, and returns the k that ``ItemCatalogue.diversify`` selects from
        them, in selection order: ``scores`` are the pool's own and ``objective`` f32 [B, k] is the
        value each item was selected at.  ``after`` is refused with them: a cursor has no meaning in
        a re-ordered list.  Sharded and clustered catalogues refuse them, but for a ``with_deep()`` view.
        A ``QuantizedItemCatalogue`` (``ItemCatalogue.quantize``) takes ``shortlist`` (None for
        min(max(4 k, 128), 1024); k..1024): the e4m3 scan's ``shortlist`` best rows are re-scored with the
        exact rows and the k best returned (k <= 1024), the flat list wherever the shortlist holds it;
        ``exclude_history`` composes, every other argument above is refused by name.  Any other
        catalogue refuses ``shortlist``.
        A ``QuantizedClusteredItemCatalogue`` (``ClusteredItemCatalogue.quantize``) takes ``nprobe`` together
        with ``shortlist``, and ``tag_all`` / ``tag_any`` / ``tag_none``, ``bias_weight`` and ``exclude_history``
        with the meaning they have on a ``with_filters()`` view: the e4m3 scan of the probed lists gives the
        ``shortlist`` best eligible rows, which are re-scored with the exact rows and the prior (k <= 1024), the
        ``with_deep()`` list wherever the shortlist holds it.  ``heads``, ``after`` and ``diversity`` / ``pool`` /
        ``group_cap`` are refused by name.
        A ``ShardedClusteredItemCatalogue`` takes ``nprobe`` per shard (every shard probes its own
        min(nprobe, nlist) nearest lists) and the arguments a clustered catalogue of its shards' kind takes,
        but ``heads`` and ``diversity`` / ``pool`` / ``group_cap``, which it refuses.  ``exclude_seen`` is ``catalogue_metrics``' name for
        ``exclude_history`` and means the same here, for every catalogue."""
        from .retrieval import make_tag_filter
        exclude_history = bool(exclude_history) or bool(exclude_seen)
        # the catalogue refuses the keywords its kind does not take and checks k / nprobe / shortlist (retrieval.py)
        catalogue._check_retrieve(k, {"heads": heads, "tag_all": tag_all, "tag_any": tag_any, "tag_none": tag_none,
                                      "after": after, "bias_weight": bias_weight, "nprobe": nprobe, "diversity": diversity,
                                      "pool": pool, "group_cap": group_cap, "shortlist": shortlist})
        diversify = diversity is not None or group_cap is not None
        if diversify:
            if "diversity" not in catalogue.retrieve_takes:
                raise ValueError("diversity / group_cap take a flat ItemCatalogue: a sharded or clustered list is "
                                 "diversified with ItemCatalogue.diversify on a flat catalogue over the same items")
            if after is not None:
                raise ValueError("after given with diversity / group_cap: a cursor has no meaning in a re-ordered list")
            if diversity is not None and (isinstance(diversity, bool) or not isinstance(diversity, (int, float))
                                          or not 0.0 <= float(diversity) <= 1.0):
                raise ValueError(f"diversity takes lambda in [0, 1] (got {diversity!r})")
            if group_cap is not None and not catalogue.has_groups:
                raise ValueError("group_cap given, but this catalogue carries no groups")
            if group_cap is not None and (isinstance(group_cap, bool) or not isinstance(group_cap, int) or group_cap < 1):
                raise ValueError(f"group_cap takes an int >= 1 (got {group_cap!r})")
            if not 1 <= int(k) <= K.RETRIEVE_MAX_K:
                raise ValueError(f"a diversified list takes k in 1..{K.RETRIEVE_MAX_K} (got {k})")
            if pool is None:
                pool = min(8 * int(k), K.RETRIEVE_MAX_POOL)
            if isinstance(pool, bool) or not isinstance(pool, int) or not int(k) <= pool <= K.RETRIEVE_MAX_POOL:
                raise ValueError(f"pool takes k..{K.RETRIEVE_MAX_POOL} candidates (got pool={pool!r}, k={k})")
        elif pool is not None:
            raise ValueError("pool given without diversity or group_cap")
        after_scores = after_ids = None
        if after is not None:
            if isinstance(after, dict):
                after_scores, after_ids = after["scores"][:, -1], after["item_ids"][:, -1]
            else:
                after_scores, after_ids = after
            if after_scores.dim() != 1 or after_ids.dim() != 1 or after_ids.dtype != torch.int64:
                raise ValueError("after takes a retrieve() result or (scores f32 [B], item_ids int64 [B])")
        if heads is not None:
            heads = [int(h) for h in heads]
            n_heads = len(self._lookahead)
            if not 1 <= len(heads) <= K.RETRIEVE_MAX_GROUP or len(set(heads)) != len(heads) \
                    or any(h < 0 or h >= n_heads for h in heads):
                raise ValueError(f"heads takes 1..{K.RETRIEVE_MAX_GROUP} distinct indices in 0..{n_heads - 1} "
                                 f"(got {heads})")
        out = self.forward(batch)
        if heads is None:
            q = out["next_token_emb"][:, -1, head].contiguous()
        else:
            q = out["next_token_emb"][:, -1, heads].contiguous()  # [B, G, 128]
        if q.dtype not in (torch.float32, torch.bfloat16):
            q = q.float()
        seen = None
        if exclude_history:
            seen = out["current_token_ids"]
            if seen.shape[1] > K.RETRIEVE_MAX_EXCLUDE:
                raise ValueError(f"exclude_history takes histories of at most {K.RETRIEVE_MAX_EXCLUDE} tokens "
                                 f"(T = {seen.shape[1]})")
        filt = None
        if tag_all is not None or tag_any is not None or tag_none is not None:
            if not catalogue.has_tags:
                raise ValueError("tag_all / tag_any / tag_none given, but this catalogue carries no tags")
            filt = make_tag_filter(q.shape[0], 0 if tag_all is None else tag_all, 0 if tag_any is None else tag_any,
                                   0 if tag_none is None else tag_none, device=q.device)
        if after_scores is not None:
            after_scores = after_scores.to(device=q.device, dtype=torch.float32).contiguous()
            after_ids = after_ids.to(q.device).contiguous()
        if isinstance(bias_weight, torch.Tensor):
            bias_weight = bias_weight.to(device=q.device, dtype=torch.float32).contiguous()
        item_ids, scores = catalogue._retrieve(q, pool if diversify else k, nprobe, shortlist, seen, filt, after_scores,
                                               after_ids, bias_weight)
        if diversify:
            item_ids, scores, obj = catalogue.diversify(item_ids, scores, k, lam=1.0 if diversity is None else float(diversity),
                                                        group_cap=group_cap)
            return {"item_ids": item_ids, "scores": scores, "objective": obj}
        return {"item_ids": item_ids, "scores": scores}

    @torch.no_grad()
    def catalogue_metrics(self, output, catalogue, ks: Optional[List[int]] = None, head: int = 0,
                          exclude_seen: bool = False, same_tags_mask: Optional[int] = None,
                          bias_weight: Optional[float] = None, nprobe: Optional[int] = None) -> Dict[str, float]:
        """Hit rate and hit position of one forward against the whole catalogue: the in-batch
        metrics of wrapper.py:228-238 with every catalogue item as a negative.  Queries are the
        positions t whose target ``current_token_ids[:, t + lookahead[head]]`` is a non-pad
        token (wrapper.py:155-163) the catalogue holds; the hit position is the number of items
        scoring strictly above the target.

        With ``exclude_seen`` the query at (b, t) ranks its target among the items sequence b has
        not seen up to t: the rows of ``current_token_ids[b, :t + 1]`` do not count (a target
        that is itself among them is still ranked, over the remaining rows).  The keys then end
        in ``_unseen``.  T <= 1024; the lists are built for at most 16,384 queries at a time.

        With ``same_tags_mask`` (an int, a 32-bit mask; the catalogue must carry tags) every query
        ranks its target among the items that agree with the target on the masked tag bits, say
        the items of the target's own category: whether the model finds the item once it has the
        category.  The keys then take the suffix ``_tagged``, after ``_unseen`` when both are on.

        With ``bias_weight`` (a float; the catalogue must carry a bias) every score, the target's
        included, is fma(bias_weight, bias[j], q . e_j): the hit position under the prior.  The
        keys then take the suffix ``_biased``, after ``_unseen`` / ``_tagged``.  Without it the
        metrics are those of the plain dot, whether or not the catalogue carries a bias.

        A ``ShardedClusteredItemCatalogue`` takes ``nprobe`` (per shard): the hit position is then the
        number of items of the probed lists scoring strictly above the target, the flat catalogue's once
        every list is probed and a lower bound of it before (the target's own list need not be probed)."""
        takes_nprobe = catalogue._RANKS_TAKE_NPROBE  # a sharded clustered catalogue: per shard
        if takes_nprobe:
            if nprobe is None:
                raise ValueError("catalogue_metrics with a sharded clustered catalogue takes nprobe, the lists each "
                                 "query scans in every shard")
            catalogue._check_call(1, nprobe)
            if not catalogue.scans_filters and (same_tags_mask is not None or bias_weight is not None):
                raise ValueError("same_tags_mask / bias_weight take with_filters() or with_deep() shards")
        elif nprobe is not None:
            raise ValueError("nprobe given, but this catalogue is not a sharded clustered one")
        if catalogue._NO_RANKS is not None:  # a clustered catalogue on one device scans some lists only
            raise ValueError(catalogue._NO_RANKS)
        ks = list(self._metrics_k_all if ks is None else ks)
        y, ids, mask = output["next_token_emb"], output["current_token_ids"], output["current_token_mask"]
        off = int(self._lookahead[head])
        L = ids.shape[1] - off
        sfx = ("_unseen" if exclude_seen else "") + ("_tagged" if same_tags_mask is not None else "") \
            + ("_biased" if bias_weight is not None else "")
        if same_tags_mask is not None and not catalogue.has_tags:
            raise ValueError("same_tags_mask given, but this catalogue carries no tags")
        if bias_weight is not None:
            if isinstance(bias_weight, bool) or not isinstance(bias_weight, (int, float)):
                raise ValueError(f"bias_weight takes a float (got {type(bias_weight).__name__})")
            if not catalogue.has_bias:
                raise ValueError("bias_weight given, but this catalogue carries no bias")
            bias_weight = float(bias_weight)
        res: Dict[str, float] = {"catalogue_queries" + sfx: 0}
        if L <= 0:
            return res
        tids = ids[:, off:]
        keep = (mask[:, off:] == 0) & catalogue.holds(tids)
        n = int(keep.sum())
        if n == 0:
            return res
        q = y[:, :L, head][keep].contiguous()
        if q.dtype not in (torch.float32, torch.bfloat16):
            q = q.float()
        tid = tids[keep].contiguous()
        filt = None
        if same_tags_mask is not None:
            filt = catalogue.filter_like(tid, same_tags_mask)
        # the scans are the catalogue's (target_ranks): one K.retrieve_topk with k = 1 per call for an
        # ItemCatalogue, one per shard and a merge for a ShardedItemCatalogue
        kw = {"nprobe": nprobe} if takes_nprobe else {}
        if not exclude_seen:
            rank = catalogue.target_ranks(q, tid, tag_filter=filt, bias_weight=bias_weight, **kw)
        else:
            T = ids.shape[1]
            if T > K.RETRIEVE_MAX_EXCLUDE:
                raise ValueError(f"exclude_seen takes histories of at most {K.RETRIEVE_MAX_EXCLUDE} tokens (T = {T})")
            bi, ti = keep.nonzero(as_tuple=True)  # the order of q's rows
            col = torch.arange(T, device=ids.device)
            ranks = []
            for lo in range(0, n, 16384):  # an [n, T] list matrix at a time; the pad id 0 and unknown ids exclude nothing
                b, t = bi[lo:lo + 16384], ti[lo:lo + 16384]
                xi = torch.where(col[None, :] <= t[:, None], ids[b], torch.zeros_like(ids[b])).contiguous()
                ranks.append(catalogue.target_ranks(q[lo:lo + 16384], tid[lo:lo + 16384], exclude_ids=xi,
                                                    tag_filter=None if filt is None else filt[lo:lo + 16384],
                                                    bias_weight=bias_weight, **kw))
            rank = torch.cat(ranks)
        pos = rank.float()
        res["catalogue_queries" + sfx] = n
        for k in ks:
            res[f"hit_rate_at_{k}_catalogue{sfx}"] = float((rank < k).float().mean())
        res["average_hit_position_catalogue" + sfx] = float(pos.mean())
        res["median_hit_position_catalogue" + sfx] = float(pos.quantile(q=0.5))
        return res

    def is_sparse(self, param_name: str):
        return super().is_sparse(param_name) or "user_context.tables" in param_name

    def optim_group(self, parent_module: nn.Module, full_param_name: str, numel: int) -> Optional[str]:
        return "SPARSE_ROWS" if "user_context.tables" in full_param_name else "USE_OPTIM"

    def optimizers_for_param_groups(self, param_groups: Dict[str, List[torch.nn.Parameter]]):
        result = []
        dense = [p for p in param_groups.get("USE_OPTIM", []) if p.requires_grad]
        if dense:
            result.append(FusedAdamW(dense, lr=self.model_config.lr, weight_decay=self.model_config.weight_decay,
                                     betas=self.model_config.betas))
        if param_groups.get("SPARSE_ROWS") and self._model.user_context is not None:
            result.append(SparseRowAdamW([self._model.user_context.tables], lr=self.model_config.lr,
                                         betas=self.model_config.betas, weight_decay=self.model_config.weight_decay))
        return result

    def param_groups(self) -> Dict[str, List[torch.nn.Parameter]]:
        groups: Dict[str, List[torch.nn.Parameter]] = {}
        for name, p in self.named_parameters():
            groups.setdefault(self.optim_group(self, name, p.numel()), []).append(p)
        return groups


class StepMetrics(MutableMapping):
    """The metric dict ``train_step`` / ``val_step`` return (wrapper.py:71-112, 139-142,
    221-245: same keys, same values), built lazily from the loss kernels' device statistics.

    Construction issues one non-blocking device->host copy of the [NH, n_mb, 8 + len(ks)]
    statistics into pinned memory on the current stream and records an event; nothing
    waits for the GPU until a key, the length or the repr is first read, so a training
    loop that never reads the dict pays no synchronisation.  After that it behaves as a
    plain mutable dict (the reference trainer adds into the first step's dict in place,
    accelerate_training_strategy.py:405-409)."""

    __slots__ = ("_pending", "_d")

    def __init__(self, stats: torch.Tensor, offs: np.ndarray, step_type: str, ks: List[int], B: int, T: int,
                 mbs: int, whole: bool):
        host = torch.empty(stats.shape, dtype=stats.dtype, pin_memory=True)
        host.copy_(stats, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending = (host, ev, offs, step_type, list(ks), B, T, mbs, whole)
        self._d: Optional[Dict[str, float]] = None

    def _dict(self) -> Dict[str, float]:
        if self._d is None:
            host, ev, offs, step_type, ks, B, T, mbs, whole = self._pending
            ev.synchronize()
            self._d = lthm_metrics(host.numpy(), offs, step_type, ks, B, T, mbs, whole)
            self._pending = None
        return self._d

    def __getitem__(self, k):
        return self._dict()[k]

    def __setitem__(self, k, v):
        self._dict()[k] = v

    def __delitem__(self, k):
        del self._dict()[k]

    def __iter__(self):
        return iter(self._dict())

    def __len__(self):
        return len(self._dict())

    def __repr__(self):
        return repr(self._dict())

    def copy(self) -> Dict[str, float]:
        return dict(self._dict())


def lthm_metrics(stats: np.ndarray, offs: np.ndarray, step_type: str, ks: List[int], B: int, T: int, mbs: int,
                 whole: bool) -> Dict[str, float]:
    """The reference's metric dict from the per-(head, mini-batch) kernel statistics.

    Per helper call (wrapper.py:139-142, 221-242): batch size, sequence length, and per head
    with a usable row the offset-keyed effective batch size, mean negatives, used tokens,
    mean CE, mean / median hit position and hits@k, then the summed loss.  A head none of whose
    used rows has a finite CE records nothing (wrapper.py:210-214: ``used_tokens == 0``);
    effective batch size and used tokens differ only when some CE is NaN.  With mini-batches
    (wrapper.py:95-111) each key is averaged over the helper calls that produced it and
    ``{step}_overall_batch_size`` is added; a whole-batch call returns its dict as is."""
    NH, n_mb, _ = stats.shape
    per = []
    for mb in range(n_mb):
        m = {f"{step_type}_batch_size": min(mbs, B - mb * mbs), f"{step_type}_seq_len": T}
        loss_mb = 0.0
        for h in range(NH):
            st = stats[h, mb]
            off = int(offs[mb, h])
            used, used_tokens = int(st[1]), int(st[7])
            if used == 0 or used_tokens == 0:
                continue
            loss_mb += float(st[0])
            m[f"{step_type}_effective_batch_size_offset_{off}"] = used
            m[f"{step_type}_average_negatives_per_token_offset_{off}"] = float(st[2])
            m[f"{step_type}_used_tokens_offset_{off}"] = used_tokens
            m[f"{step_type}_loss_all_tokens_offset_{off}"] = float(st[0])
            m[f"{step_type}_average_hit_position_offset_{off}"] = float(st[4])
            m[f"{step_type}_median_hit_position_offset_{off}"] = float(st[5])
            for q, k in enumerate(ks):
                m[f"{step_type}_hit_rate_at_{k}_offset_{off}"] = float(st[NSTAT_BASE + q])
        m[f"{step_type}_loss"] = loss_mb
        per.append(m)
    if whole:
        return per[0]
    acc: Dict[str, float] = {}
    cnt: Dict[str, int] = {}
    for m in per:
        for k, v in m.items():
            acc[k] = acc.get(k, 0.0) + v
            cnt[k] = cnt.get(k, 0) + 1
    out = {k: acc[k] / cnt[k] for k in acc}
    out[f"{step_type}_overall_batch_size"] = B
    return out
