"""The ranking stage: score and sort retrieved candidate lists with the ranker.

    ids = lthm.retrieve(batch, catalogue.with_deep(), 1024, nprobe=32)["item_ids"]   # int64 [Q, 1024], pads 0
    top, logits, src = ranker.rank(users, ids, store, k=100)                         # best first

``RankerModelConfig.n_user_dense`` / ``n_user_categorical`` split the ranker's input columns into a user
side (the first columns) and an item side (the rest).  ``ItemFeatureStore`` holds the item side of every
item the ranker may meet, by id; ``rank`` (``RankerModelWrapper.rank``) takes one user row per query and a
list of candidate ids per query, and per chunk of queries runs

    store.rows_of  ->  K.rank_assemble  ->  the model's own forward  ->  K.rank_sort

on the device, without a host synchronisation in between (csrc/rank.hip).  The logits are the forward's
own: the assembled batch holds the bits an explicit ``expand`` / index / ``cat`` would, so the stage adds
no arithmetic of its own.  The order of a list is (logit descending, store row ascending, list position
ascending); store rows ascend with the ids, so equal logits come id-ascending and a repeated id keeps
both copies in input order.  Pads (id 0), ids the store does not hold and NaN logits are no candidates;
empty slots hold (0, -inf, -1).
"""
from __future__ import annotations

import json
from typing import Dict, Optional, Tuple

import torch

from ... import kernels as K

FORMAT = "lthm-ranker-item-features-v1"


class ItemFeatureStore:
    """``ids`` int64 [N], strictly ascending (so unique) and without the pad id 0, the rules of
    ``ItemCatalogue``; ``dense`` f32 [N, n_item_dense] and ``categorical`` int64 [N, n_item_cat], row i the
    item-side ranker features of ``ids[i]``.  Either width may be 0."""

    def __init__(self, ids: torch.Tensor, dense: torch.Tensor, categorical: torch.Tensor):
        if ids.dtype != torch.int64 or ids.dim() != 1:
            raise ValueError(f"store ids must be int64 [N] (got {ids.dtype} {tuple(ids.shape)})")
        if dense.dtype != torch.float32 or dense.dim() != 2:
            raise ValueError(f"store dense features must be f32 [N, n_item_dense] (got {dense.dtype} {tuple(dense.shape)})")
        if categorical.dtype != torch.int64 or categorical.dim() != 2:
            raise ValueError(f"store categorical features must be int64 [N, n_item_cat] "
                             f"(got {categorical.dtype} {tuple(categorical.shape)})")
        if dense.shape[0] != ids.shape[0] or categorical.shape[0] != ids.shape[0] or ids.shape[0] < 1:
            raise ValueError(f"store needs one dense and one categorical row per id and at least one id "
                             f"({ids.shape[0]} ids, {dense.shape[0]} dense rows, {categorical.shape[0]} categorical rows)")
        if ids.device != dense.device or ids.device != categorical.device:
            raise ValueError("store ids, dense and categorical features must live on one device")
        if bool((ids == 0).any()):
            raise ValueError("store ids must not hold 0, the pad id")
        if ids.shape[0] > 1 and not bool((ids[1:] > ids[:-1]).all()):
            raise ValueError("store ids must be strictly ascending (sorted, no duplicates)")
        self.ids = ids.contiguous()
        self.dense = dense.contiguous()
        self.categorical = categorical.contiguous()

    def __len__(self) -> int:
        return self.ids.shape[0]

    @property
    def n_item_dense(self) -> int:
        return self.dense.shape[1]

    @property
    def n_item_categorical(self) -> int:
        return self.categorical.shape[1]

    @property
    def device(self) -> torch.device:
        return self.ids.device

    def to(self, device) -> "ItemFeatureStore":
        return ItemFeatureStore(self.ids.to(device), self.dense.to(device), self.categorical.to(device))

    def rows_of(self, ids: torch.Tensor) -> torch.Tensor:
        """Store row of every id (int32, same shape), -1 for ids the store does not hold and for 0."""
        flat = ids.reshape(-1).to(self.ids.device)
        at = torch.searchsorted(self.ids, flat).clamp_(max=len(self) - 1)
        rows = torch.where(self.ids[at] == flat, at, torch.full_like(at, -1))
        return rows.to(torch.int32).view(ids.shape)

    def save(self, path: str) -> None:
        from safetensors.torch import save_file
        tensors = {"ids": self.ids.detach().cpu().contiguous(), "dense": self.dense.detach().cpu().contiguous(),
                   "categorical": self.categorical.detach().cpu().contiguous()}
        save_file(tensors, path, metadata={"format": FORMAT})

    @classmethod
    def load(cls, path: str, *, device=None) -> "ItemFeatureStore":
        from safetensors import safe_open
        with safe_open(path, framework="pt") as f:
            meta = f.metadata() or {}
            if meta.get("format") != FORMAT:
                raise ValueError(f"{path}: not an item feature store (metadata {json.dumps(meta)})")
            store = cls(f.get_tensor("ids"), f.get_tensor("dense"), f.get_tensor("categorical"))
        return store.to(device) if device is not None else store


def check_rank_call(cfg, user_batch: Dict[str, torch.Tensor], item_ids: torch.Tensor, store: ItemFeatureStore,
                    k: Optional[int], max_rows: int) -> Tuple[int, int, int, int]:
    """Every refusal of ``rank``, before anything runs; returns (Q, M, k, queries per chunk)."""
    if cfg.n_user_dense is None or cfg.n_user_categorical is None:
        raise ValueError("rank needs a config with a feature split: set n_user_dense and n_user_categorical "
                         f"(got n_user_dense={cfg.n_user_dense}, n_user_categorical={cfg.n_user_categorical})")
    du, fu = cfg.n_user_dense, cfg.n_user_categorical
    di, fi = cfg.n_dense - du, cfg.n_categorical - fu
    if item_ids.dtype != torch.int64 or item_ids.dim() != 2:
        raise ValueError(f"item_ids must be int64 [Q, M] (got {item_ids.dtype} {tuple(item_ids.shape)})")
    Q, M = item_ids.shape
    if Q < 1 or not 1 <= M <= K.RANK_MAX_LIST:
        raise ValueError(f"item_ids takes Q >= 1 lists of 1..{K.RANK_MAX_LIST} candidates (got Q={Q}, M={M})")
    if not isinstance(user_batch, dict) or "dense" not in user_batch or "categorical" not in user_batch:
        raise ValueError('user_batch must be a dict with "dense" and "categorical"')
    ud, uc = user_batch["dense"], user_batch["categorical"]
    if ud.dtype != torch.float32 or tuple(ud.shape) != (Q, du):
        raise ValueError(f'user_batch["dense"] must be f32 [Q, n_user_dense] = [{Q}, {du}] (got {ud.dtype} {tuple(ud.shape)})')
    if uc.dtype != torch.int64 or tuple(uc.shape) != (Q, fu):
        raise ValueError(f'user_batch["categorical"] must be int64 [Q, n_user_categorical] = [{Q}, {fu}] '
                         f"(got {uc.dtype} {tuple(uc.shape)})")
    if not isinstance(store, ItemFeatureStore):
        raise ValueError(f"store must be an ItemFeatureStore (got {type(store).__name__})")
    if store.n_item_dense != di or store.n_item_categorical != fi:
        raise ValueError(f"store must hold the item side of the split, {di} dense and {fi} categorical columns "
                         f"(got {store.n_item_dense} and {store.n_item_categorical})")
    k = M if k is None else k
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= M:
        raise ValueError(f"k takes an int in 1..M = 1..{M} (got {k!r})")
    if isinstance(max_rows, bool) or not isinstance(max_rows, int) or max_rows < 1:
        raise ValueError(f"max_rows takes an int >= 1 (got {max_rows!r})")
    return Q, M, k, max(1, max_rows // M)


@torch.no_grad()
def rank(wrapper, user_batch: Dict[str, torch.Tensor], item_ids: torch.Tensor, store: ItemFeatureStore,
         k: Optional[int] = None, *, max_rows: int = 65536, probabilities: bool = False):
    """``RankerModelWrapper.rank`` (see there)."""
    Q, M, k, step = check_rank_call(wrapper.model_config, user_batch, item_ids, store, k, max_rows)
    dev = store.device
    ud, uc = user_batch["dense"].to(dev).contiguous(), user_batch["categorical"].to(dev).contiguous()
    item_ids = item_ids.to(dev).contiguous()
    out_ids = torch.empty((Q, k), dtype=torch.int64, device=dev)
    out_scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_src = torch.empty((Q, k), dtype=torch.int32, device=dev)
    for q0 in range(0, Q, step):
        q1 = min(Q, q0 + step)
        rows = store.rows_of(item_ids[q0:q1]).contiguous()
        dense, cat = K.rank_assemble(ud[q0:q1], uc[q0:q1], store.dense, store.categorical, rows)
        logits = wrapper.forward({"dense": dense, "categorical": cat})["logits"]
        scores, top, src = K.rank_sort(logits.reshape(q1 - q0, M).float().contiguous(), rows, k)
        out_ids[q0:q1] = torch.where(top >= 0, store.ids[top.clamp(min=0).long()], torch.zeros_like(top, dtype=torch.int64))
        out_scores[q0:q1] = scores
        out_src[q0:q1] = src
    if probabilities:
        out_scores = torch.sigmoid(out_scores)  # an empty slot's -inf gives 0.0
    return out_ids, out_scores, out_src
