"""Item catalogue and full-catalogue retrieval for the LTHM two-tower model (build-defined:
the reference trains the towers, wrapper.py:114-245, but ships no retrieval code).

``next_token_emb[:, t, head]`` is a query and the product tower's ``prod_emb`` a candidate;
the loss normalises both (wrapper.py:118-119) and ranks by their dot product.  An
``ItemCatalogue`` holds the normalised candidate of every item id once, so that a query is
scored against all of them (``K.retrieve_topk``, csrc/retrieve.hip) instead of against the
in-batch negatives only.

File format: safetensors with the two tensors ``ids`` / ``emb`` and a ``format`` metadata
string, in the style of item_artifact.py.  Loading executes nothing from the file.
"""
from __future__ import annotations

import json
from typing import Optional

import torch

from .... import kernels as K
from ....distributed import world_size

FORMAT = "lthm-item-catalogue-v1"
WIDTH = K.RETRIEVE_WIDTH


class ItemCatalogue:
    """``ids`` int64 [N], strictly ascending (so unique) and without the pad id 0; ``emb`` bf16
    [N, 128], row i the normalised candidate vector of ``ids[i]``."""

    def __init__(self, ids: torch.Tensor, emb: torch.Tensor):
        if ids.dtype != torch.int64 or ids.dim() != 1:
            raise ValueError(f"catalogue ids must be int64 [N] (got {ids.dtype} {tuple(ids.shape)})")
        if emb.dtype != torch.bfloat16 or emb.dim() != 2 or emb.shape[1] != WIDTH:
            raise ValueError(f"catalogue embeddings must be bf16 [N, {WIDTH}] (got {emb.dtype} {tuple(emb.shape)})")
        if emb.shape[0] != ids.shape[0] or ids.shape[0] < 1:
            raise ValueError(f"catalogue needs one embedding row per id and at least one id "
                             f"({ids.shape[0]} ids, {emb.shape[0]} rows)")
        if ids.device != emb.device:
            raise ValueError("catalogue ids and embeddings must live on one device")
        if bool((ids == 0).any()):
            raise ValueError("catalogue ids must not hold 0, the pad id")
        if ids.shape[0] > 1 and not bool((ids[1:] > ids[:-1]).all()):
            raise ValueError("catalogue ids must be strictly ascending (sorted, no duplicates); "
                             "ItemCatalogue.from_embeddings sorts")
        self.ids = ids.contiguous()
        self.emb = emb.contiguous()

    def __len__(self) -> int:
        return self.ids.shape[0]

    @classmethod
    def from_embeddings(cls, ids: torch.Tensor, emb: torch.Tensor) -> "ItemCatalogue":
        """From ids in any order and their (already normalised, bf16) vectors: rows are sorted
        by id.  Duplicate ids are refused, as is id 0."""
        if ids.dim() != 1 or emb.dim() != 2 or ids.shape[0] != emb.shape[0]:
            raise ValueError("from_embeddings takes ids [N] and emb [N, 128]")
        order = torch.argsort(ids, stable=True)
        return cls(ids[order], emb[order.to(emb.device)])

    def to(self, device) -> "ItemCatalogue":
        return ItemCatalogue(self.ids.to(device), self.emb.to(device))

    def rows_of(self, ids: torch.Tensor) -> torch.Tensor:
        """Catalogue row of every id (int32, same shape), -1 for ids the catalogue does not hold."""
        flat = ids.reshape(-1).to(self.ids.device)
        at = torch.searchsorted(self.ids, flat).clamp_(max=len(self) - 1)
        rows = torch.where(self.ids[at] == flat, at, torch.full_like(at, -1))
        return rows.to(torch.int32).view(ids.shape)

    def topk(self, q: torch.Tensor, k: int, *, normalize_q: bool = True, target_ids: Optional[torch.Tensor] = None,
             slab_rows: int = 0, exclude_ids: Optional[torch.Tensor] = None):
        """The k best items per query: (item_ids int64 [Q, k], scores f32 [Q, k], rank, target_score).
        Empty slots (N < k) hold id 0 and score -inf.  With ``target_ids`` [Q], ``rank`` is each
        query's count of items scoring strictly above its target (-1 where the catalogue does
        not hold the target) and ``target_score`` the target's score; else both are None.
        ``exclude_ids`` int64 [Q, X] (X <= 1024) names items query q must not return, in any
        order: they take no slot and do not count in ``rank`` (``K.retrieve_topk``'s
        ``exclude_rows``).  Ids the catalogue does not hold, and the pad id 0, exclude nothing.
        A 3-D ``q`` [U, G, 128] (G <= 8) holds G queries per user: an item's score is its best
        over them (``K.retrieve_topk_group``), and the outputs, ``target_ids`` [U] and
        ``exclude_ids`` [U, X] are per user."""
        tr = self.rows_of(target_ids).contiguous() if target_ids is not None else None
        xr = None
        if exclude_ids is not None:
            if exclude_ids.dtype != torch.int64 or exclude_ids.dim() != 2:
                raise ValueError(f"exclude_ids must be int64 [Q, X] (got {exclude_ids.dtype} {tuple(exclude_ids.shape)})")
            xr = self.rows_of(exclude_ids).contiguous()  # -1 for unknown ids and for 0, which no catalogue holds
        call = K.retrieve_topk_group if q.dim() == 3 else K.retrieve_topk
        scores, rows, rank, tscore = call(q, self.emb, k, normalize_q=normalize_q, target_rows=tr,
                                          slab_rows=slab_rows, exclude_rows=xr)
        item_ids = torch.where(rows >= 0, self.ids[rows.clamp(min=0).long()], torch.zeros_like(rows, dtype=torch.int64))
        return item_ids, scores, rank, tscore

    def save(self, path: str) -> None:
        from safetensors.torch import save_file
        save_file({"ids": self.ids.detach().cpu().contiguous(), "emb": self.emb.detach().cpu().contiguous()}, path,
                  metadata={"format": FORMAT})

    @classmethod
    def load(cls, path: str, *, device=None) -> "ItemCatalogue":
        from safetensors import safe_open
        with safe_open(path, framework="pt") as f:
            meta = f.metadata() or {}
            if meta.get("format") != FORMAT:
                raise ValueError(f"{path}: not an item catalogue (metadata {json.dumps(meta)})")
            ids, emb = f.get_tensor("ids"), f.get_tensor("emb")
        cat = cls(ids, emb)
        return cat.to(device) if device is not None else cat


@torch.no_grad()
def build_catalogue(wrapper, ids: torch.Tensor, chunk: int = 65536) -> ItemCatalogue:
    """The catalogue of ``ids`` under ``wrapper``'s current weights: per chunk, the item
    embedding module and the product tower on a [1, n] id row (the training kernels), then
    F.normalize to bf16 as the loss does (``K.rownorm``).  A row therefore equals the
    normalised ``current_token_emb`` row a forward produces for that id."""
    from ....commons.layers import RowShardedKShiftEmbedding
    enc = wrapper._model
    if isinstance(enc.product_emb_module, RowShardedKShiftEmbedding) and world_size() > 1:
        raise RuntimeError("build_catalogue does not take a row-sharded item table at world size > 1")
    if ids.dtype != torch.int64 or ids.dim() != 1 or ids.numel() < 1:
        raise ValueError("build_catalogue takes int64 ids [N], N >= 1")
    if chunk < 1:
        raise ValueError("chunk must be positive")
    dev = next(wrapper.parameters()).device
    ids = torch.unique(ids.to(dev))  # sorted ascending
    if bool((ids == 0).any()):
        raise ValueError("catalogue ids must not hold 0, the pad id")
    out = torch.empty((ids.numel(), WIDTH), dtype=torch.bfloat16, device=dev)
    for lo in range(0, ids.numel(), chunk):
        row = ids[lo:lo + chunk].view(1, -1).contiguous()
        _, prod, _ = enc.product_tower(row, enc.product_emb_module(row))
        out[lo:lo + row.numel()] = K.rownorm(prod.reshape(-1, WIDTH).contiguous())[0]
    return ItemCatalogue(ids, out)
