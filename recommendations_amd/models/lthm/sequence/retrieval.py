"""Item catalogue and full-catalogue retrieval for the LTHM two-tower model (build-defined:
the reference trains the towers, wrapper.py:114-245, but ships no retrieval code).

``next_token_emb[:, t, head]`` is a query and the product tower's ``prod_emb`` a candidate;
the loss normalises both (wrapper.py:118-119) and ranks by their dot product.  An
``ItemCatalogue`` holds the normalised candidate of every item id once, so that a query is
scored against all of them (``K.retrieve_topk``, csrc/retrieve.hip) instead of against the
in-batch negatives only.

File format: safetensors with the two tensors ``ids`` / ``emb``, the optional ``tags``,
``bias`` and ``groups``, and a ``format`` metadata string, in the style of item_artifact.py.  Loading executes
nothing from the file.

Tags: a catalogue may carry one int32 word per item, read as 32 independent attribute bits (in
stock, category, market, ...).  A query's filter (all, any, none) then restricts its top-K and
its rank to the items whose word has every ``all`` bit, some ``any`` bit (if any is non-zero) and
no ``none`` bit, inside the kernel (``K.retrieve_topk``'s ``tags`` / ``tag_filter``).

Bias: a catalogue may carry one finite f32 per item, a score prior (popularity, freshness, a
sponsored lift, a demotion).  A query's score for item j is then fma(w, bias[j], q . e_j) with a
weight w per query (1 unless told otherwise), inside the kernel (``K.retrieve_topk``'s ``bias`` /
``bias_weight``): the order, the cursors and the ranks are those of the biased scores.

Groups: a catalogue may carry one int32 key per item (brand, seller, parent product; 0 = none).
``ItemCatalogue.diversify`` re-ranks a list any ``topk`` returned: greedy maximal-marginal-relevance
selection against the items already chosen, with at most ``group_cap`` chosen items per non-zero key
(``K.retrieve_diversify``, one block per query on the device).

Shards: a ``ShardedItemCatalogue`` holds the items as several ``ItemCatalogue``s with disjoint ids,
on this process's devices and, with a process group, on the other ranks' (the row-sharded item
table of C3: ``build_catalogue(..., shard=(rank, world))``).  Its ``topk`` returns, bit for bit, what
one catalogue over the union returns: every shard is scanned on its own against the target's score
(``K.retrieve_target_score``, ``K.retrieve_topk(target_scores=)``) and the lists are merged on the
device (``K.retrieve_merge_shards``).

Clusters: a ``ClusteredItemCatalogue`` (``ItemCatalogue.cluster`` or ``from_assignment``) holds the
rows grouped into lists around centroids, and its ``topk`` scans only the ``nprobe`` lists nearest
to each query (``K.retrieve_ivf_topk``): the exact top-k of the probed lists, with the flat scan's
score bits, and with ``nprobe`` = L the flat scan's result.  Its ``with_filters()`` view scans the same
lists with the catalogue's tags and bias and behind a (score, id) cursor, under ``ItemCatalogue.topk``'s
conventions.  Its ``with_heads()`` view is that view for users with several queries each (``q``
[U, G, 128], ``K.retrieve_ivf_topk_group``): one probe row per user, an item scored by its best match
over the user's queries inside the scan, one slot per item.

Clustered shards: a ``ShardedClusteredItemCatalogue`` holds clustered catalogues (plain, ``with_filters()``
or ``with_deep()``) with disjoint ids as the shards of one catalogue: every shard probes its own ``nprobe``
nearest lists, one call scans the probed lists of all shards of a device and merges them
(``K.retrieve_ivf_topk_shards``), and with every list probed the result is the flat catalogue's bit for bit.

Clustered e4m3: ``ClusteredItemCatalogue.quantize`` gives a ``QuantizedClusteredItemCatalogue``, the same lists
as e4m3 codes with the catalogue's tags and bias: its ``topk`` scans the probed lists' codes for a shortlist of
the eligible rows (``K.retrieve_ivf_q8_topk``) and re-scores it with the exact rows and the prior
(``K.retrieve_rescore_bias``), which is the ``with_filters()`` / ``with_deep()`` list restricted to the shortlist.

Updates: ``ItemCatalogue.update`` and ``ClusteredItemCatalogue.update`` return a new catalogue without some ids
and with the rows of an ``upsert`` catalogue replacing or joining the old ones, an upserted row in the list of
its nearest centroid: per list one merge of two ascending id sequences (``K.catalogue_update``,
csrc/catalogue_update.hip), bit for bit ``from_assignment`` of the rebuilt flat catalogue.  The quantised and
the sharded catalogues refuse ``update`` and say what to do instead.

Shared by the kinds, once each: the id lookup of the single-device catalogues (``_IdIndex``: ``rows_of``, ``holds``,
``_ids_of``, ``filter_like`` where the kind scans tags; flat rows are in id order, clustered ones go through ``_ids`` / ``_order``), the
argument checks every ``topk`` calls (``_check_exclude``, ``_check_tag_filter``, ``_check_bias_weight``,
``_check_cursor``, ``_check_shortlist``, ``_check_probe_call``), ``_hit_fraction`` behind every ``recall``, ``_save`` /
``_opened`` behind every ``save`` / ``load``, ``_sharded_target_score`` in both sharded scans, and what
``LTHMModelWrapper.retrieve`` asks of a catalogue (``_Catalogue``: the keywords it takes, the sentence for the
others, its checks ahead of the forward and the one ``topk`` call that answers with (item_ids, scores)).
"""
from __future__ import annotations

import contextlib
import json
from typing import List, Optional, Sequence, Tuple, Union

import torch

from .... import kernels as K
from ....distributed import all_gather_stack, all_reduce_max, world_size

FORMAT = "lthm-item-catalogue-v1"
WIDTH = K.RETRIEVE_WIDTH


def _bits32(v, n: int, name: str, device) -> torch.Tensor:
    """An int or an integer tensor [n] (or scalar) of values in -2^31 .. 2^32 - 1 as int64 [n]
    holding the int32 value with the same low 32 bits."""
    if isinstance(v, torch.Tensor):
        if v.dtype not in (torch.int32, torch.int64, torch.uint8, torch.int16, torch.int8) or v.dim() > 1:
            raise ValueError(f"{name} must be an int or an integer tensor [{n}] (got {v.dtype} {tuple(v.shape)})")
        t = v.to(device=device, dtype=torch.int64).reshape(-1)
        if t.numel() == 1:
            t = t.expand(n)
        if t.numel() != n:
            raise ValueError(f"{name} must hold one value or {n} (got {t.numel()})")
    else:
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an int or an integer tensor (got {type(v).__name__})")
        t = torch.full((n,), v, dtype=torch.int64, device=device)
    if bool(((t < -(1 << 31)) | (t > (1 << 32) - 1)).any()):
        raise ValueError(f"{name} must lie in 0..2^32-1 (or be an int32 bit pattern)")
    t = t & 0xFFFFFFFF
    return torch.where(t >= (1 << 31), t - (1 << 32), t)


def make_tag_filter(n: int, tag_all: Union[int, torch.Tensor] = 0, tag_any: Union[int, torch.Tensor] = 0,
                    tag_none: Union[int, torch.Tensor] = 0, device=None) -> torch.Tensor:
    """The int32 [n, 3] filter (all, any, none) of n queries from Python ints or integer tensors
    [n] (one value serves every query).  Values are 32-bit masks in 0..2^32-1 and wrap to the
    int32 with the same bits, so bit 31 is ``1 << 31``."""
    if n < 1:
        raise ValueError("make_tag_filter takes n >= 1")
    cols = [_bits32(v, n, name, device) for v, name in ((tag_all, "tag_all"), (tag_any, "tag_any"), (tag_none, "tag_none"))]
    return torch.stack(cols, dim=1).to(torch.int32).contiguous()


def _opt(t: Optional[torch.Tensor], f) -> Optional[torch.Tensor]:
    """``f(t)``, or None for a column the catalogue does not carry."""
    return None if t is None else f(t)


def _filter_row(t: torch.Tensor, found: torch.Tensor, mask, device) -> torch.Tensor:
    """``filter_like``'s int32 [Q, 3] rows (t & mask, 0, ~t & mask) from the targets' tag words ``t`` (int64 [Q],
    the int32 values) and ``found`` (bool [Q]): (0, 0, 0) where no target was found."""
    m = _bits32(mask, t.numel(), "mask", device)
    m = torch.where(found, m, torch.zeros_like(m))
    return torch.stack([t & m, torch.zeros_like(t), ~t & m], dim=1).to(torch.int32).contiguous()


# The argument checks of every ``topk`` / ``_scan``.  With ``Q`` they also check the shape against the queries;
# without it they leave that to the kernel's wrapper (the flat scans, whose per-user arguments it knows).

def _check_exclude(exclude_ids) -> None:
    if exclude_ids is not None and (exclude_ids.dtype != torch.int64 or exclude_ids.dim() != 2):
        raise ValueError(f"exclude_ids must be int64 [Q, X] (got {exclude_ids.dtype} {tuple(exclude_ids.shape)})")


def _check_tag_filter(cat, tag_filter, Q: Optional[int] = None) -> None:
    if tag_filter is None:
        return
    if not cat.has_tags:
        raise ValueError("tag_filter given, but this catalogue carries no tags")
    if Q is not None and (tag_filter.dtype != torch.int32 or tuple(tag_filter.shape) != (Q, 3)):
        raise ValueError(f"tag_filter must be int32 [Q, 3] = (all, any, none) "
                         f"(got {tag_filter.dtype} {tuple(tag_filter.shape)}, Q={Q})")


def _check_bias_weight(cat, bias_weight, Q: Optional[int] = None) -> None:
    if bias_weight is None:
        return
    if not cat.has_bias:
        raise ValueError("bias_weight given, but this catalogue carries no bias")
    if Q is None:
        return
    if isinstance(bias_weight, torch.Tensor):
        if bias_weight.dtype != torch.float32 or tuple(bias_weight.shape) != (Q,):
            raise ValueError(f"bias_weight must be None, a number or f32 [Q] "
                             f"(got {bias_weight.dtype} {tuple(bias_weight.shape)}, Q={Q})")
    elif isinstance(bias_weight, bool) or not isinstance(bias_weight, (int, float)):
        raise ValueError(f"bias_weight must be None, a number or f32 [Q] (got {type(bias_weight).__name__})")


def _check_cursor(after_scores, after_ids, Q: Optional[int] = None) -> None:
    if (after_scores is None) != (after_ids is None):
        raise ValueError("after_scores and after_ids are given together or neither")
    if after_ids is None:
        return
    if after_ids.dtype != torch.int64 or (after_ids.dim() != 1 if Q is None else tuple(after_ids.shape) != (Q,)):
        raise ValueError(f"after_ids must be int64 [Q] (got {after_ids.dtype} {tuple(after_ids.shape)})")
    if Q is not None and (after_scores.dtype != torch.float32 or tuple(after_scores.shape) != (Q,)):
        raise ValueError(f"after_scores must be f32 [Q] (got {after_scores.dtype} {tuple(after_scores.shape)})")


def _check_shortlist(k: int, shortlist, keyword: bool = False) -> int:
    """The rows of the e4m3 scan's shortlist: ``shortlist``, or min(max(4 k, 128), 1024) for None; in k..1024.
    ``keyword``: ``retrieve``'s argument, an int, refused in ``retrieve``'s words."""
    if keyword and shortlist is not None and (isinstance(shortlist, bool) or not isinstance(shortlist, int)
                                              or not int(k) <= shortlist <= K.RETRIEVE_Q8_MAX_POOL):
        raise ValueError(f"shortlist takes k..{K.RETRIEVE_Q8_MAX_POOL} rows (got shortlist={shortlist!r}, k={k})")
    M = QuantizedItemCatalogue.default_shortlist(k) if shortlist is None else int(shortlist)
    if not keyword and not k <= M <= K.RETRIEVE_Q8_MAX_POOL:
        raise ValueError(f"shortlist must lie in k..{K.RETRIEVE_Q8_MAX_POOL} (got shortlist={M}, k={k})")
    return M


def _check_probe_call(k: int, nprobe, max_k: int, nlist: Optional[int] = None) -> Tuple[int, int]:
    """(k, nprobe) of a clustered scan: ``nprobe`` an int in 1..64 and, for one catalogue, at most its ``nlist``
    (sharded: every shard probes min(nprobe, its nlist)); ``k`` in 1..``max_k``."""
    if nprobe is None or isinstance(nprobe, bool) or not isinstance(nprobe, int):
        raise ValueError(f"a clustered catalogue takes nprobe, an int (got {nprobe!r})")
    if nprobe > K.RETRIEVE_MAX_PROBE:
        raise ValueError(f"nprobe takes at most {K.RETRIEVE_MAX_PROBE} lists per query (got {nprobe})")
    if nlist is not None and nprobe > nlist:
        raise ValueError(f"nprobe takes at most the {nlist} lists there are (got {nprobe})")
    if nprobe < 1:
        raise ValueError(f"nprobe takes at least one list (got {nprobe})")
    k = int(k)
    if not 1 <= k <= max_k:
        raise ValueError(f"a clustered catalogue takes k in 1..{max_k} (got {k})")
    return k, nprobe


def _hit_fraction(want_ids: torch.Tensor, got_ids: torch.Tensor, k: int) -> float:
    """Every ``recall``: the mean, over the queries whose reference list ``want_ids`` [Q, k] holds an id at all, of
    the fraction of its ids (0 = an empty slot) that ``got_ids`` [Q, k] holds; 1.0 where no reference list does.
    The comparison runs over at most 16 Mi (want, got) pairs at a time.

    Two of the five callers (``QuantizedItemCatalogue``, ``ClusteredItemCatalogue``) used to write hits /
    max(ids, 1) averaged over all queries, in one piece.  Their reference is the unfiltered flat list of a
    catalogue that is never empty, so no list is empty: no query is left out, the hit and id counts are the
    same integers, and the divisions and the mean are the same f64 operations on them.  The floats agree."""
    real = want_ids != 0
    rows = max(1, (1 << 24) // (int(k) * int(k)))  # queries per comparison
    hit = torch.cat([((want_ids[i:i + rows, :, None] == got_ids[i:i + rows, None, :]).any(dim=2) & real[i:i + rows]).sum(dim=1)
                     for i in range(0, want_ids.shape[0], rows)]).double()
    n = real.sum(dim=1)
    if not bool((n > 0).any()):
        return 1.0
    return float((hit[n > 0] / n[n > 0].double()).mean())


def _save(path: str, tensors: dict, index: Optional[str] = None) -> None:
    """The named tensors (None: a column not carried) as safetensors with the format tag and the kind's ``index`` tag."""
    from safetensors.torch import save_file
    meta = {"format": FORMAT} if index is None else {"format": FORMAT, "index": index}
    save_file({n: t.detach().cpu().contiguous() for n, t in tensors.items() if t is not None}, path, metadata=meta)


@contextlib.contextmanager
def _opened(path: str, index: Optional[str], what: str):
    """A catalogue file of the kind ``index`` (None: any item catalogue), checked: yields ``get(name)``, which reads
    one tensor, and with ``optional=True`` gives None for one the file does not hold."""
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        meta = f.metadata() or {}
        if meta.get("format") != FORMAT or (index is not None and meta.get("index") != index):
            raise ValueError(f"{path}: not {what} (metadata {json.dumps(meta)})")
        names = set(f.keys())
        yield lambda name, optional=False: f.get_tensor(name) if not optional or name in names else None


# retrieve()'s optional keywords that a catalogue which does not take them refuses by name, in the message's order
_NAMED = ("heads", "tag_all", "tag_any", "tag_none", "after", "bias_weight", "nprobe", "diversity", "pool", "group_cap")
_TAGS = ("tag_all", "tag_any", "tag_none")


def _refuse_named(cat, given: dict, order=_NAMED) -> None:
    bad = [name for name in order if given[name] is not None and name not in cat.retrieve_takes]
    if bad:
        raise ValueError(cat._REFUSAL.format(", ".join(bad)))


def _refuse_shortlist(given: dict) -> None:
    if given["shortlist"] is not None:
        raise ValueError("shortlist given, but this catalogue is not quantised (ItemCatalogue.quantize builds one)")


def _need_nprobe(given: dict) -> None:
    if given["nprobe"] is None:
        raise ValueError("retrieve with a clustered catalogue takes nprobe, the lists each query scans")


class _Catalogue:
    """What ``LTHMModelWrapper.retrieve`` and ``catalogue_metrics`` ask of every catalogue kind:

    ``retrieve_takes``  the optional keywords of ``retrieve`` this catalogue takes (a property where views differ)
    ``_REFUSAL``        the sentence for the others, with a slot for their names
    ``_check_retrieve(k, given)``  refuses the keywords not taken and checks ``k`` / ``nprobe`` / ``shortlist``
                        ahead of the forward, in this kind's order; ``given`` maps every keyword to its value
    ``_retrieve(q, k, nprobe, shortlist, exclude_ids, tag_filter, after_scores, after_ids, bias_weight)``
                        the one ``topk`` call behind ``retrieve``: (item_ids, scores)
    ``_NO_RANKS``       why ``catalogue_metrics`` does not take this kind (None: it does, by ``target_ranks``)
    ``_RANKS_TAKE_NPROBE``  whether its ``target_ranks`` takes ``nprobe``"""
    _NO_RANKS = None
    _RANKS_TAKE_NPROBE = False
    tags = bias = None

    @property
    def has_tags(self) -> bool:
        return self.tags is not None

    @property
    def has_bias(self) -> bool:
        return self.bias is not None


class _IdIndex(_Catalogue):
    """The id lookup of a single-device catalogue.  ``_ids`` are its ids ascending.  A flat catalogue's rows are in
    that order: ``_order`` is None and row i holds ``_ids[i]``.  A clustered one's are list-major: ``_order[i]`` is
    the row of ``_ids[i]`` and ``row_ids`` the id of every row."""
    _order = None

    def rows_of(self, ids: torch.Tensor) -> torch.Tensor:
        """The catalogue row of every id (int32, same shape), -1 for ids the catalogue does not hold."""
        flat = ids.reshape(-1).to(self._ids.device)
        at = torch.searchsorted(self._ids, flat).clamp_(max=len(self) - 1)
        rows = torch.where(self._ids[at] == flat, at if self._order is None else self._order[at], torch.full_like(at, -1))
        return rows.to(torch.int32).view(ids.shape)

    def holds(self, ids: torch.Tensor) -> torch.Tensor:
        """bool, the shape of ``ids``: the catalogue holds this id."""
        return self.rows_of(ids) >= 0

    def _ids_of(self, rows: torch.Tensor) -> torch.Tensor:
        """The id of every row (int64, same shape), 0 for a row < 0: ``rows_of``'s inverse."""
        ids = self._ids if self._order is None else self.row_ids
        return torch.where(rows >= 0, ids[rows.clamp(min=0).long()], torch.zeros_like(rows, dtype=torch.int64))

    def _filter_like(self, target_ids: torch.Tensor, mask: int) -> torch.Tensor:
        """The filter "the same value as the target in the masked bit field": per target t the
        row (tags[t] & mask, 0, ~tags[t] & mask) of an int32 [Q, 3] filter.  ``mask`` is a 32-bit
        mask in 0..2^32-1.  A target the catalogue does not hold gets (0, 0, 0)."""
        if self.tags is None:
            raise ValueError("filter_like needs a catalogue with tags")
        if target_ids.dim() != 1:
            raise ValueError("filter_like takes target ids [Q]")
        rows = self.rows_of(target_ids).long()
        t = torch.where(rows >= 0, self.tags[rows.clamp(min=0)].long(), torch.zeros_like(rows))
        return _filter_row(t, rows >= 0, mask, self.tags.device)


def _sharded_target_score(shards, q, target_ids, normalize_q: bool, bias_weight, use_bias: bool, reduce_max):
    """The target's score over the shards of a catalogue, from the one shard that holds the target
    (``K.retrieve_target_score`` per shard, NaN where it does not hold it, to -inf; the maximum over the shards and,
    with ``reduce_max``, over the ranks: a real score is finite).  Returns (the score with NaN where no shard holds
    the target, as ``target_scores`` of the scans; the same with -inf there, what one catalogue returns; the
    target's row in every shard)."""
    home = q.device
    on = lambda t, dev: None if t is None else t.to(dev).contiguous()
    parts, trows = [], []
    for s in shards:
        dev = s.emb.device
        trows.append(s.rows_of(target_ids).contiguous())
        with torch.cuda.device(dev):
            parts.append(K.retrieve_target_score(on(q, dev), s.emb, trows[-1], normalize_q=normalize_q,
                                                 bias=s.bias if use_bias else None,
                                                 bias_weight=on(bias_weight, dev) if use_bias else None).to(home))
    ts = torch.stack(parts)
    ts = reduce_max(torch.where(torch.isnan(ts), torch.full_like(ts, float("-inf")), ts).amax(dim=0))
    return torch.where(ts == float("-inf"), torch.full_like(ts, float("nan")), ts).contiguous(), ts, trows


_UPDATE_COLUMNS = (("tags", torch.int32), ("bias", torch.float32), ("groups", torch.int32))


def _update_dead(cat, upsert, remove_ids, missing_ok: bool, who: str) -> Tuple[torch.Tensor, int]:
    """The argument checks of ``update`` on ``cat`` (flat or clustered) and (dead, N'): the uint8 [N] flag
    of the old rows that are removed or replaced, found with ``cat.rows_of``, and the row count of the
    result.  The count and the three verdicts that only the device knows (an absent, a repeated, a doubly
    named id) come to the host in one read."""
    N, dev = len(cat), cat.emb.device
    if upsert is not None:
        if not isinstance(upsert, ItemCatalogue):
            raise ValueError(f"{who} takes an ItemCatalogue as upsert (got {type(upsert).__name__})")
        if upsert.ids.device != dev:
            raise ValueError(f"{who} takes an upsert on the catalogue's device ({dev}; got {upsert.ids.device})")
        for name, _ in _UPDATE_COLUMNS:
            has, gets = getattr(cat, name) is not None, getattr(upsert, name) is not None
            if has != gets:
                raise ValueError(f"{who}: upsert must carry {name} exactly when the catalogue does "
                                 f"(the catalogue {'has' if has else 'has no'} {name}, upsert {'has' if gets else 'has none'})")
    if remove_ids is not None:
        if not isinstance(remove_ids, torch.Tensor) or remove_ids.dtype != torch.int64 or remove_ids.dim() != 1:
            raise ValueError(f"{who} takes remove_ids int64 [R] (got {getattr(remove_ids, 'dtype', type(remove_ids).__name__)} "
                             f"{tuple(getattr(remove_ids, 'shape', ()))})")
        if remove_ids.device != dev:
            raise ValueError(f"{who} takes remove_ids on the catalogue's device ({dev}; got {remove_ids.device})")
        if remove_ids.numel() == 0:
            remove_ids = None
    hit = torch.zeros(N + 1, dtype=torch.uint8, device=dev)  # slot N takes the ids the catalogue does not hold
    flags = torch.zeros(3, dtype=torch.int64, device=dev)    # absent, repeated, in both arguments
    if remove_ids is not None:
        rows = cat.rows_of(remove_ids).long()
        hit[torch.where(rows >= 0, rows, torch.full_like(rows, N))] = 1
        srt = torch.sort(remove_ids)[0]
        flags[0] = (rows < 0).sum()
        flags[1] = (srt[1:] == srt[:-1]).sum()
        if upsert is not None:
            flags[2] = upsert.holds(remove_ids).sum()
    if upsert is not None:
        rows = cat.rows_of(upsert.ids).long()
        hit[torch.where(rows >= 0, rows, torch.full_like(rows, N))] = 1
    dead = hit[:N]
    live, absent, repeated, both = torch.cat([(N - dead.sum(dtype=torch.int64)).reshape(1), flags]).tolist()  # the one read
    if repeated:
        raise ValueError(f"{who}: remove_ids must be distinct ({repeated} repeated)")
    if both:
        raise ValueError(f"{who}: {both} ids are in both upsert and remove_ids; an id is replaced or removed, not both")
    if absent and not missing_ok:
        raise ValueError(f"{who}: {absent} of the remove_ids are not in the catalogue (missing_ok=True ignores them)")
    n_out = live + (0 if upsert is None else len(upsert))
    if n_out < 1:
        raise ValueError(f"{who}: no row remains, and a catalogue is never empty")
    return dead, n_out


def _update_delta(cat, upsert: Optional["ItemCatalogue"], order: Optional[torch.Tensor]) -> dict:
    """The delta arguments of ``K.catalogue_update``: the upsert's rows in ``order`` (None: as they are), or
    no rows with the columns ``cat`` carries."""
    dev = cat.emb.device
    if upsert is None:
        kw = {"delta_ids": torch.empty(0, dtype=torch.int64, device=dev),
              "delta_emb": torch.empty((0, WIDTH), dtype=torch.bfloat16, device=dev)}
        for name, dt in _UPDATE_COLUMNS:
            kw["delta_" + name] = None if getattr(cat, name) is None else torch.empty(0, dtype=dt, device=dev)
        return kw
    pick = (lambda t: t) if order is None else (lambda t: t[order])
    kw = {"delta_ids": pick(upsert.ids), "delta_emb": pick(upsert.emb)}
    for name, _ in _UPDATE_COLUMNS:
        kw["delta_" + name] = None if getattr(upsert, name) is None else pick(getattr(upsert, name))
    return kw


def _no_update(what: str, instead: str):
    raise ValueError(f"{what} has no update: {instead}")


class ItemCatalogue(_IdIndex):
    """``ids`` int64 [N], strictly ascending (so unique) and without the pad id 0; ``emb`` bf16
    [N, 128], row i the normalised candidate vector of ``ids[i]``; ``tags`` int32 [N] or None,
    row i the 32 attribute bits of ``ids[i]``; ``bias`` f32 [N] or None, row i the score prior of
    ``ids[i]``, every value finite (checked here, with one sync); ``groups`` int32 [N] or None, row i
    the group key of ``ids[i]`` (brand, seller, parent product), 0 for an item of no group."""

    def __init__(self, ids: torch.Tensor, emb: torch.Tensor, tags: Optional[torch.Tensor] = None,
                 bias: Optional[torch.Tensor] = None, groups: Optional[torch.Tensor] = None):
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
        if tags is not None:
            if tags.dtype != torch.int32 or tags.dim() != 1 or tags.shape[0] != ids.shape[0]:
                raise ValueError(f"catalogue tags must be int32 [N], one word per id "
                                 f"(got {tags.dtype} {tuple(tags.shape)}, N={ids.shape[0]})")
            if tags.device != ids.device:
                raise ValueError("catalogue tags must live on the device of ids and embeddings")
            tags = tags.contiguous()
        if bias is not None:
            if bias.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] != ids.shape[0]:
                raise ValueError(f"catalogue bias must be f32 [N], one word per id "
                                 f"(got {bias.dtype} {tuple(bias.shape)}, N={ids.shape[0]})")
            if bias.device != ids.device:
                raise ValueError("catalogue bias must live on the device of ids and embeddings")
            if not bool(torch.isfinite(bias).all()):
                raise ValueError("catalogue bias must be finite (it holds NaN or +-inf)")
            bias = bias.contiguous()
        if groups is not None:
            if groups.dtype != torch.int32 or groups.dim() != 1 or groups.shape[0] != ids.shape[0]:
                raise ValueError(f"catalogue groups must be int32 [N], one key per id "
                                 f"(got {groups.dtype} {tuple(groups.shape)}, N={ids.shape[0]})")
            if groups.device != ids.device:
                raise ValueError("catalogue groups must live on the device of ids and embeddings")
            groups = groups.contiguous()
        self.ids = ids.contiguous()
        self.emb = emb.contiguous()
        self.tags = tags
        self.bias = bias
        self.groups = groups

    _ids = property(lambda self: self.ids)
    filter_like = _IdIndex._filter_like

    def __len__(self) -> int:
        return self.ids.shape[0]

    @property
    def has_groups(self) -> bool:
        return self.groups is not None

    def take(self, rows: torch.Tensor) -> "ItemCatalogue":
        """The catalogue of some of the rows: a bool mask [N] or an integer index tensor (any order,
        no row twice).  Tags, bias and groups move with the rows; at least one row must remain."""
        if rows.dtype == torch.bool:
            if rows.shape != self.ids.shape:
                raise ValueError(f"take: a mask must be bool [N] (got {tuple(rows.shape)}, N={len(self)})")
            idx = rows.to(self.ids.device).nonzero(as_tuple=True)[0]
        else:
            if rows.dim() != 1 or rows.is_floating_point():
                raise ValueError(f"take: an index must be an integer tensor [n] (got {rows.dtype} {tuple(rows.shape)})")
            idx = torch.sort(rows.to(device=self.ids.device, dtype=torch.int64))[0]
            if idx.numel() and (int(idx[0]) < 0 or int(idx[-1]) >= len(self)):
                raise ValueError(f"take: rows must lie in 0..{len(self) - 1}")
            if idx.numel() > 1 and bool((idx[1:] == idx[:-1]).any()):
                raise ValueError("take: a row is named twice")
        if idx.numel() < 1:
            raise ValueError("take: no row remains, and a catalogue is never empty")
        pick = lambda t: t[idx]
        return ItemCatalogue(self.ids[idx], self.emb[idx], _opt(self.tags, pick), _opt(self.bias, pick), _opt(self.groups, pick))

    def split(self, n: int) -> List["ItemCatalogue"]:
        """n shards of contiguous id ranges: shard i holds rows [i N // n, (i + 1) N // n), so none
        is empty.  n > N is refused."""
        N = len(self)
        if not 1 <= int(n) <= N:
            raise ValueError(f"split takes 1..N shards (got n={n}, N={N}): a shard is never empty")
        n = int(n)
        dev = self.ids.device
        return [self.take(torch.arange(i * N // n, (i + 1) * N // n, device=dev)) for i in range(n)]

    def target_ranks(self, q: torch.Tensor, target_ids: torch.Tensor, *, exclude_ids: Optional[torch.Tensor] = None,
                     tag_filter: Optional[torch.Tensor] = None, bias_weight: Optional[float] = None) -> torch.Tensor:
        """The hit position of every query's target (``catalogue_metrics``): the number of eligible
        items scoring strictly above it, -1 where the catalogue does not hold the target; one
        ``K.retrieve_topk`` with k = 1.  The prior counts only where ``bias_weight`` is given: without
        it the scores are the plain dots, whether or not the catalogue carries a bias."""
        xr = None if exclude_ids is None else self.rows_of(exclude_ids).contiguous()
        return K.retrieve_topk(q, self.emb, 1, normalize_q=True, target_rows=self.rows_of(target_ids).contiguous(),
                               exclude_rows=xr, tags=self.tags if tag_filter is not None else None, tag_filter=tag_filter,
                               bias=self.bias if bias_weight is not None else None, bias_weight=bias_weight)[2]

    @classmethod
    def from_embeddings(cls, ids: torch.Tensor, emb: torch.Tensor, tags: Optional[torch.Tensor] = None,
                        bias: Optional[torch.Tensor] = None, groups: Optional[torch.Tensor] = None) -> "ItemCatalogue":
        """From ids in any order and their (already normalised, bf16) vectors: rows are sorted
        by id, and ``tags`` (int32 [N]), ``bias`` (f32 [N]) and ``groups`` (int32 [N]), given in the
        order of ``ids``, move with them.  Duplicate ids are refused, as is id 0."""
        if ids.dim() != 1 or emb.dim() != 2 or ids.shape[0] != emb.shape[0]:
            raise ValueError("from_embeddings takes ids [N] and emb [N, 128]")
        if tags is not None and (tags.dim() != 1 or tags.shape[0] != ids.shape[0]):
            raise ValueError("from_embeddings takes tags [N], one word per id")
        if bias is not None and (bias.dim() != 1 or bias.shape[0] != ids.shape[0]):
            raise ValueError("from_embeddings takes bias [N], one word per id")
        if groups is not None and (groups.dim() != 1 or groups.shape[0] != ids.shape[0]):
            raise ValueError("from_embeddings takes groups [N], one key per id")
        order = torch.argsort(ids, stable=True)
        pick = lambda t: t[order.to(t.device)]
        return cls(ids[order], pick(emb), _opt(tags, pick), _opt(bias, pick), _opt(groups, pick))

    def to(self, device) -> "ItemCatalogue":
        on = lambda t: t.to(device)
        return ItemCatalogue(on(self.ids), on(self.emb), _opt(self.tags, on), _opt(self.bias, on), _opt(self.groups, on))

    def cursor_rows(self, after_ids: torch.Tensor) -> torch.Tensor:
        """The row cursor of an id cursor (int32, same shape): (number of catalogue ids <=
        after_id) - 1, so that "row > cursor row" means "id > after_id" whether or not the
        catalogue holds after_id.  An id below the first gives -1, one above the last N - 1."""
        flat = after_ids.reshape(-1).to(self.ids.device).contiguous()
        return (torch.searchsorted(self.ids, flat, right=True) - 1).to(torch.int32).view(after_ids.shape)

    def topk(self, q: torch.Tensor, k: int, *, normalize_q: bool = True, target_ids: Optional[torch.Tensor] = None,
             slab_rows: int = 0, exclude_ids: Optional[torch.Tensor] = None,
             tag_filter: Optional[torch.Tensor] = None, after_scores: Optional[torch.Tensor] = None,
             after_ids: Optional[torch.Tensor] = None,
             bias_weight: Union[None, float, torch.Tensor] = None):
        """The k best items per query: (item_ids int64 [Q, k], scores f32 [Q, k], rank, target_score).
        Empty slots (N < k) hold id 0 and score -inf.  With ``target_ids`` [Q], ``rank`` is each
        query's count of items scoring strictly above its target (-1 where the catalogue does
        not hold the target) and ``target_score`` the target's score; else both are None.
        ``exclude_ids`` int64 [Q, X] (X <= 1024) names items query q must not return, in any
        order: they take no slot and do not count in ``rank`` (``K.retrieve_topk``'s
        ``exclude_rows``).  Ids the catalogue does not hold, and the pad id 0, exclude nothing.
        A 3-D ``q`` [U, G, 128] (G <= 8) holds G queries per user: an item's score is its best
        over them (``K.retrieve_topk_group``), and the outputs, ``target_ids`` [U] and
        ``exclude_ids`` [U, X] are per user.
        ``tag_filter`` int32 [Q, 3] ([U, 3] with a 3-D ``q``) = (all, any, none) restricts query q
        to the items whose tag word passes it (see ``make_tag_filter`` and ``filter_like``): the others
        take no slot and do not count in ``rank``, exactly like excluded items.  The catalogue
        must carry tags.
        ``after_scores`` f32 [Q] and ``after_ids`` int64 [Q] ([U] with a 3-D ``q``), together or
        neither, start every list strictly behind (score, id) in the order (score descending, id
        ascending): the last column of one page is the cursor of the next, and it stays valid
        after its item has left the catalogue (``cursor_rows``).  The empty slot (-inf, 0) of an
        exhausted page gives an empty page.  ``k`` may reach ``K.RETRIEVE_MAX_DEEP`` = 1024; above
        128 the list still comes from a single scan of the catalogue (the deep selection kernel).
        A catalogue that carries a ``bias`` scores item j as fma(w, bias[j], q . e_j): ``scores``,
        the order, ``target_score``, ``rank`` and the cursors are those of the biased scores.
        ``bias_weight`` is w: None for 1, a number, or f32 [Q] ([U] with a 3-D ``q``), one weight
        per query.  A catalogue without a bias refuses a weight."""
        _check_tag_filter(self, tag_filter)
        _check_bias_weight(self, bias_weight)
        _check_cursor(after_scores, after_ids)
        ar = None
        if after_ids is not None:
            ar = self.cursor_rows(after_ids).contiguous()
            after_scores = after_scores.contiguous()
        tr = self.rows_of(target_ids).contiguous() if target_ids is not None else None
        _check_exclude(exclude_ids)
        xr = _opt(exclude_ids, lambda x: self.rows_of(x).contiguous())  # -1 for unknown ids and for 0, which no catalogue holds
        call = K.retrieve_topk_group if q.dim() == 3 else K.retrieve_topk
        scores, rows, rank, tscore = call(q, self.emb, k, normalize_q=normalize_q, target_rows=tr,
                                          slab_rows=slab_rows, exclude_rows=xr,
                                          tags=self.tags if tag_filter is not None else None, tag_filter=tag_filter,
                                          after_scores=after_scores, after_rows=ar, deep=int(k) > K.RETRIEVE_MAX_K,
                                          bias=self.bias, bias_weight=bias_weight)
        return self._ids_of(rows), scores, rank, tscore

    retrieve_takes = frozenset(_NAMED) - {"nprobe"}

    def _check_retrieve(self, k, given: dict) -> None:
        _refuse_shortlist(given)
        if given["nprobe"] is not None:
            raise ValueError("nprobe given, but this catalogue is not clustered (ItemCatalogue.cluster builds one)")

    def _retrieve(self, q, k, nprobe, shortlist, exclude_ids, tag_filter, after_scores, after_ids, bias_weight):
        return self.topk(q, k, normalize_q=True, exclude_ids=exclude_ids, tag_filter=tag_filter, after_scores=after_scores,
                         after_ids=after_ids, bias_weight=bias_weight)[:2]

    def diversify(self, item_ids: torch.Tensor, scores: torch.Tensor, k: int, *,
                  lam: Union[float, torch.Tensor] = 1.0, group_cap: Optional[int] = None):
        """A diversified list of k out of a pool per query: (item_ids int64 [Q, k], scores f32 [Q, k],
        objective f32 [Q, k]) in selection order (``K.retrieve_diversify``).  ``item_ids`` int64 [Q, M]
        and ``scores`` f32 [Q, M], M <= ``K.RETRIEVE_MAX_POOL`` = 1024, are a list any catalogue over
        these items returned (flat, sharded or clustered: all give ids), in any order; an id this
        catalogue does not hold, the pad id 0 and a score of -inf or NaN are no candidates.  k times
        the item with the largest ``lam`` * score - (1 - ``lam``) * (its largest dot with an item
        chosen so far) is chosen, ties to the lower id; ``lam`` is a number or f32 [Q], in [0, 1]:
        1 keeps the order by score, 0 looks at similarity only.  ``group_cap`` = m keeps at most m
        chosen items of one non-zero group key and needs a catalogue with groups.  ``scores`` of
        the result are the pool's own; empty slots hold (0, -inf, -inf)."""
        if item_ids.dtype != torch.int64 or item_ids.dim() != 2:
            raise ValueError(f"diversify takes int64 item_ids [Q, M] (got {item_ids.dtype} {tuple(item_ids.shape)})")
        if scores.dtype != torch.float32 or scores.shape != item_ids.shape:
            raise ValueError(f"diversify takes f32 scores of the ids' shape (got {scores.dtype} {tuple(scores.shape)})")
        Q, M = item_ids.shape
        if not 1 <= M <= K.RETRIEVE_MAX_POOL:
            raise ValueError(f"diversify takes a pool of 1..{K.RETRIEVE_MAX_POOL} candidates (got M={M})")
        if not 1 <= int(k) <= K.RETRIEVE_MAX_K:
            raise ValueError(f"diversify takes k in 1..{K.RETRIEVE_MAX_K} (got {k})")
        if group_cap is not None:
            if self.groups is None:
                raise ValueError("group_cap given, but this catalogue carries no groups")
            if isinstance(group_cap, bool) or not isinstance(group_cap, int) or group_cap < 1:
                raise ValueError(f"group_cap takes an int >= 1 (got {group_cap!r})")
        dev = self.emb.device
        if isinstance(lam, torch.Tensor):
            if lam.dim() != 1 or lam.shape[0] != Q or not lam.is_floating_point():
                raise ValueError(f"lam must be a number or a float tensor [Q] (got {lam.dtype} {tuple(lam.shape)}, Q={Q})")
            lam_t = lam.detach().to(torch.float32).cpu()
            if not bool(((lam_t >= 0) & (lam_t <= 1)).all()):  # NaN fails as well
                raise ValueError("lam must lie in [0, 1] for every query")
            lam_t = lam_t.to(dev).contiguous()
        else:
            if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= float(lam) <= 1.0:
                raise ValueError(f"lam must lie in [0, 1] (got {lam!r})")
            lam_t = None if float(lam) == 1.0 else torch.full((Q,), float(lam), dtype=torch.float32, device=dev)
        rows, sc, obj = K.retrieve_diversify(self.emb, self.rows_of(item_ids).contiguous(), scores.to(dev).contiguous(),
                                             int(k), lam=lam_t, groups=self.groups if group_cap is not None else None,
                                             cap=group_cap if group_cap is not None else 1)
        return self._ids_of(rows), sc, obj

    def save(self, path: str) -> None:
        _save(path, {"ids": self.ids, "emb": self.emb, "tags": self.tags, "bias": self.bias, "groups": self.groups})

    @classmethod
    def load(cls, path: str, *, device=None) -> "ItemCatalogue":
        with _opened(path, None, "an item catalogue") as get:
            cat = cls(get("ids"), get("emb"), get("tags", True), get("bias", True), get("groups", True))
        return cat.to(device) if device is not None else cat

    def quantize(self, keep_exact: bool = True) -> "QuantizedItemCatalogue":
        """This catalogue as e4m3 codes with one power-of-two scale per row
        (``K.quantize_catalogue_q8``, on the catalogue's device), and with ``keep_exact`` the bf16 rows
        beside them for re-scoring.  Tags, bias and groups are not carried in this version: a quantised
        catalogue scores plain dots over all rows, and ``quantize()`` drops them."""
        codes, scale = K.quantize_catalogue_q8(self.emb)
        return QuantizedItemCatalogue(self.ids, codes, scale, self.emb if keep_exact else None)

    @torch.no_grad()
    def cluster(self, nlist: int, iters: int = 10, seed: int = 0, sample: Optional[int] = None) -> "ClusteredItemCatalogue":
        """This catalogue as ``nlist`` lists around centroids found by spherical k-means, on the
        catalogue's device (the assignments are ``K.retrieve_topk`` calls).  The centroids start as
        ``nlist`` rows picked by a permutation seeded with ``seed``; with ``sample`` the iterations
        see only the first ``sample`` rows of that permutation (``nlist <= sample <= N``).  An
        iteration assigns every row to its best centroid (``K.retrieve_topk`` with k = 1, the rows as
        queries: ties go to the lower list) and replaces every centroid by the normalised f32 sum of
        its rows, taken in (list, id) order by a segmented sum, so two builds give the same bits; a
        list left without rows keeps its centroid.  A last assignment of all rows against the stored
        centroids fixes the lists."""
        N = len(self)
        nlist, iters = int(nlist), int(iters)
        if not 1 <= nlist <= N:
            raise ValueError(f"cluster takes 1..N lists (got nlist={nlist}, N={N})")
        if iters < 0:
            raise ValueError(f"cluster takes iters >= 0 (got {iters})")
        if sample is not None and not nlist <= int(sample) <= N:
            raise ValueError(f"cluster takes nlist <= sample <= N (got sample={sample}, nlist={nlist}, N={N})")
        dev = self.emb.device
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))  # on the host: one order everywhere
        centroids = self.emb[perm[:nlist].to(dev)].contiguous()
        train = self.emb
        if sample is not None and int(sample) < N:
            train = self.emb[torch.sort(perm[:int(sample)])[0].to(dev)].contiguous()  # id-ascending, as the catalogue is
        for _ in range(iters):
            assign = K.retrieve_topk(train, centroids, 1, normalize_q=False)[1][:, 0].long()
            order = torch.argsort(assign, stable=True)  # (list, id)
            counts = torch.bincount(assign, minlength=nlist)
            sums = torch.segment_reduce(train[order].float(), "sum", lengths=counts, axis=0, unsafe=True)
            norm = sums.norm(dim=1, keepdim=True)
            keep = (counts == 0)[:, None] | (norm == 0)
            centroids = torch.where(keep, centroids, (sums / norm.clamp_min(1e-12)).to(torch.bfloat16)).contiguous()
        assign = K.retrieve_topk(self.emb, centroids, 1, normalize_q=False)[1][:, 0].long()
        return ClusteredItemCatalogue.from_assignment(self, centroids, assign)

    @classmethod
    def _trusted(cls, ids, emb, tags, bias, groups) -> "ItemCatalogue":
        """A catalogue of tensors that ``update`` produced from checked catalogues: what the constructor
        checks holds by construction, so nothing is read back from the device."""
        cat = object.__new__(cls)
        cat.ids, cat.emb, cat.tags, cat.bias, cat.groups = ids, emb, tags, bias, groups
        return cat

    @torch.no_grad()
    def update(self, upsert: Optional["ItemCatalogue"] = None, remove_ids: Optional[torch.Tensor] = None, *,
               missing_ok: bool = False) -> "ItemCatalogue":
        """A new catalogue: this one without the ``remove_ids`` (int64 [R], distinct, on this device), with
        the rows of ``upsert`` (an ``ItemCatalogue`` on this device) in place of the rows with their ids, and
        with its other rows added, ids ascending.  ``upsert`` carries exactly the optional columns (tags, bias,
        groups) this catalogue carries.  An id to remove that the catalogue does not hold is refused unless
        ``missing_ok``; so are an id in both arguments and a result without rows.  Neither argument (or an
        empty ``remove_ids`` alone) gives an equal catalogue.  This catalogue is unchanged.

        One merge of two ascending id sequences on the device (``K.catalogue_update``, the one-list case),
        with one device-to-host read, of the new row count and the verdicts on the ids."""
        who = "ItemCatalogue.update"
        dead, n_out = _update_dead(self, upsert, remove_ids, missing_ok, who)
        dev = self.ids.device
        M = 0 if upsert is None else len(upsert)
        ids, emb, _, tags, bias, groups = K.catalogue_update(
            self.ids, self.emb, torch.tensor([0, len(self)], dtype=torch.int64, device=dev), dead,
            delta_off=torch.tensor([0, M], dtype=torch.int64, device=dev), tags=self.tags, bias=self.bias,
            groups=self.groups, n_out=n_out, **_update_delta(self, upsert, None))
        return ItemCatalogue._trusted(ids, emb, tags, bias, groups)


Q8_INDEX = "lthm-q8-v1"


class QuantizedItemCatalogue(_IdIndex):
    """An ``ItemCatalogue`` stored as OCP e4m3fn codes: ``ids`` int64 [N] (strictly ascending, no 0),
    ``codes`` uint8 [N, 128] and ``scale`` f32 [N] as ``K.quantize_catalogue_q8`` writes them (row i
    stands for ``codes[i] * scale[i]``), and ``emb`` bf16 [N, 128] or None, the exact rows.  ``topk`` scans
    the codes for a shortlist (``K.retrieve_q8_topk``) and, where the exact rows are kept, re-scores the
    shortlist in bf16 (``K.retrieve_rescore``): the result is the flat list restricted to the shortlist,
    so it equals ``ItemCatalogue.topk`` whenever the shortlist holds the flat top-k.  Tags, bias and
    groups are not carried in this version."""

    def __init__(self, ids: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor, emb: Optional[torch.Tensor] = None):
        if ids.dtype != torch.int64 or ids.dim() != 1 or ids.shape[0] < 1:
            raise ValueError(f"catalogue ids must be int64 [N], N >= 1 (got {ids.dtype} {tuple(ids.shape)})")
        N = ids.shape[0]
        if codes.dtype != torch.uint8 or tuple(codes.shape) != (N, WIDTH):
            raise ValueError(f"catalogue codes must be uint8 [N, {WIDTH}] (got {codes.dtype} {tuple(codes.shape)}, N={N})")
        if scale.dtype != torch.float32 or tuple(scale.shape) != (N,):
            raise ValueError(f"catalogue scales must be f32 [N] (got {scale.dtype} {tuple(scale.shape)}, N={N})")
        if emb is not None and (emb.dtype != torch.bfloat16 or tuple(emb.shape) != (N, WIDTH)):
            raise ValueError(f"catalogue embeddings must be bf16 [N, {WIDTH}] (got {emb.dtype} {tuple(emb.shape)}, N={N})")
        if codes.device != ids.device or scale.device != ids.device or (emb is not None and emb.device != ids.device):
            raise ValueError("catalogue ids, codes, scales and embeddings must live on one device")
        if bool((ids == 0).any()):
            raise ValueError("catalogue ids must not hold 0, the pad id")
        if N > 1 and not bool((ids[1:] > ids[:-1]).all()):
            raise ValueError("catalogue ids must be strictly ascending (sorted, no duplicates)")
        self.ids = ids.contiguous()
        self.codes = codes.contiguous()
        self.scale = scale.contiguous()
        self.emb = None if emb is None else emb.contiguous()

    _ids = property(lambda self: self.ids)

    def __len__(self) -> int:
        return self.ids.shape[0]

    @property
    def keep_exact(self) -> bool:
        return self.emb is not None

    def update(self, *args, **kwargs):
        """Refused: the codes and scales are made per catalogue by ``quantize()``."""
        _no_update("a QuantizedItemCatalogue", "update the bf16 ItemCatalogue and call quantize() again")

    def to(self, device) -> "QuantizedItemCatalogue":
        return QuantizedItemCatalogue(self.ids.to(device), self.codes.to(device), self.scale.to(device),
                                      _opt(self.emb, lambda t: t.to(device)))

    def to_flat(self) -> ItemCatalogue:
        """The exact catalogue (without tags, bias or groups); needs ``keep_exact``."""
        if self.emb is None:
            raise ValueError("to_flat needs the exact rows: this catalogue was built with keep_exact=False")
        return ItemCatalogue(self.ids, self.emb)

    @staticmethod
    def default_shortlist(k: int) -> int:
        return min(max(4 * int(k), 128), K.RETRIEVE_Q8_MAX_POOL)

    def topk(self, q: torch.Tensor, k: int, *, shortlist: Optional[int] = None, rescore: bool = True,
             normalize_q: bool = True, exclude_ids: Optional[torch.Tensor] = None,
             slab_rows: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(item_ids int64 [Q, k], scores f32 [Q, k]).  The ``shortlist`` first rows under the
        approximate e4m3 scores (default min(max(4 k, 128), 1024); in k..1024) are re-scored with the
        exact bf16 rows and the k first under (score descending, id ascending) returned: every score
        has the bits ``ItemCatalogue.topk`` returns for that (query, item).  ``rescore=False`` returns
        the first k of the shortlist with the approximate scores, the only mode of a catalogue built
        with ``keep_exact=False``.  ``exclude_ids`` int64 [Q, X] (X <= 1024) as in ``ItemCatalogue.topk``.
        Empty slots hold id 0 and score -inf.  ``k`` in 1..1024, ``q`` [Q, 128]."""
        k = int(k)
        if not 1 <= k <= K.RETRIEVE_Q8_MAX_POOL:
            raise ValueError(f"a quantised catalogue takes k in 1..{K.RETRIEVE_Q8_MAX_POOL} (got {k})")
        M = _check_shortlist(k, shortlist)
        if rescore and self.emb is None:
            raise ValueError("rescore=True needs the exact rows: this catalogue was built with keep_exact=False "
                             "(pass rescore=False)")
        if q.dim() != 2:
            raise ValueError(f"a quantised catalogue takes [Q, {WIDTH}] queries, one per row (got {tuple(q.shape)})")
        _check_exclude(exclude_ids)
        xr = _opt(exclude_ids, lambda x: self.rows_of(x).contiguous())
        scores, rows = K.retrieve_q8_topk(q, self.codes, self.scale, M, normalize_q=normalize_q, exclude_rows=xr,
                                          slab_rows=slab_rows)
        if rescore:
            scores, rows = K.retrieve_rescore(q, self.emb, rows, k, normalize_q=normalize_q)
        else:
            scores, rows = scores[:, :k].contiguous(), rows[:, :k].contiguous()
        return self._ids_of(rows), scores

    retrieve_takes = frozenset()
    _REFUSAL = "retrieve with a quantised catalogue does not take {}: use catalogue.to_flat() for it"

    def _check_retrieve(self, k, given: dict) -> None:
        _refuse_named(self, given)
        _check_shortlist(k, given["shortlist"], keyword=True)
        if not 1 <= int(k) <= K.RETRIEVE_Q8_MAX_POOL:
            raise ValueError(f"a quantised catalogue takes k in 1..{K.RETRIEVE_Q8_MAX_POOL} (got {k})")

    def _retrieve(self, q, k, nprobe, shortlist, exclude_ids, tag_filter, after_scores, after_ids, bias_weight):
        return self.topk(q, k, shortlist=shortlist, rescore=self.keep_exact, normalize_q=True, exclude_ids=exclude_ids)

    def recall(self, q: torch.Tensor, k: int, shortlist: Optional[int] = None) -> float:
        """The mean over the queries of the fraction of the flat scan's top-k ids that
        ``topk(q, k, shortlist=shortlist)`` returns; needs ``keep_exact``."""
        return _hit_fraction(self.to_flat().topk(q, k)[0], self.topk(q, k, shortlist=shortlist)[0], k)

    def save(self, path: str) -> None:
        """``ItemCatalogue.save``'s container with ``codes`` and ``scale`` beside ``ids`` (and ``emb``
        where the exact rows are kept: ``ItemCatalogue.load`` then reads the flat catalogue)."""
        _save(path, {"ids": self.ids, "codes": self.codes, "scale": self.scale, "emb": self.emb}, Q8_INDEX)

    @classmethod
    def load(cls, path: str, *, device=None) -> "QuantizedItemCatalogue":
        with _opened(path, Q8_INDEX, "a quantised item catalogue") as get:
            cat = cls(get("ids"), get("codes"), get("scale"), get("emb", True))
        return cat.to(device) if device is not None else cat


IVF_INDEX = "lthm-ivf-v1"


class ClusteredItemCatalogue(_IdIndex):
    """An ``ItemCatalogue`` whose rows are grouped into L lists around centroids (an inverted-file
    index), so that a query scans the ``nprobe`` lists nearest to it instead of every row
    (``K.retrieve_ivf_topk``, csrc/retrieve.hip ``retr_ivf_topk_k``).

    ``emb`` bf16 [N, 128], list-major: list c is rows ``list_off[c] .. list_off[c + 1]``, its ids
    ascending; ``row_ids`` int64 [N], the id of every row (distinct, never 0); ``list_off`` int64
    [L + 1]; ``centroids`` bf16 [L, 128]; ``tags`` / ``bias`` in the rows' order or None.  Tags and
    bias are carried for ``to_flat()`` and for the view ``with_filters()`` returns, whose scan applies
    them and takes cursors; this catalogue's own scan scores the plain dot and filters nothing but
    ``exclude_ids``.  Groups are not carried: a clustered list is diversified against
    the flat catalogue it was built from (``ItemCatalogue.diversify`` takes its ids), or by the view
    ``with_deep(groups)`` returns, which takes them and whose lists reach k = 1,024.  Several queries per
    user (``q`` [U, G, 128], the wrapper's ``heads``) take the view ``with_heads()`` returns; this
    catalogue and the other two views take one query per row."""

    def __init__(self, row_ids: torch.Tensor, emb: torch.Tensor, list_off: torch.Tensor, centroids: torch.Tensor,
                 tags: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
        if row_ids.dtype != torch.int64 or row_ids.dim() != 1 or row_ids.shape[0] < 1:
            raise ValueError(f"clustered row_ids must be int64 [N], N >= 1 (got {row_ids.dtype} {tuple(row_ids.shape)})")
        N = row_ids.shape[0]
        if emb.dtype != torch.bfloat16 or emb.dim() != 2 or tuple(emb.shape) != (N, WIDTH):
            raise ValueError(f"clustered embeddings must be bf16 [N, {WIDTH}] (got {emb.dtype} {tuple(emb.shape)}, N={N})")
        if centroids.dim() != 2 or centroids.shape[1] != WIDTH or centroids.shape[0] < 1:
            raise ValueError(f"centroids must be [L, {WIDTH}], L >= 1 (got {tuple(centroids.shape)})")
        if centroids.dtype != torch.bfloat16:
            raise ValueError(f"centroids must be bf16, as the catalogue's rows are (got {centroids.dtype})")
        L = centroids.shape[0]
        if list_off.dtype != torch.int64 or tuple(list_off.shape) != (L + 1,):
            raise ValueError(f"list_off must be int64 [L + 1] (got {list_off.dtype} {tuple(list_off.shape)}, L={L})")
        dev = emb.device
        if any(t.device != dev for t in (row_ids, list_off, centroids)):
            raise ValueError("a clustered catalogue's tensors must live on one device")
        if int(list_off[0]) != 0 or int(list_off[-1]) != N or bool((list_off[1:] < list_off[:-1]).any()):
            raise ValueError("list_off must ascend from 0 to N")
        ids, order = torch.sort(row_ids)
        if bool((ids == 0).any()):
            raise ValueError("catalogue ids must not hold 0, the pad id")
        if N > 1 and bool((ids[1:] == ids[:-1]).any()):
            raise ValueError("catalogue ids must be distinct")
        if N > 1:
            inside = torch.ones(N - 1, dtype=torch.bool, device=dev)  # row i and row i + 1 share a list
            cut = list_off[1:-1]
            cut = cut[(cut > 0) & (cut < N)]
            inside[cut - 1] = False
            if bool((inside & (row_ids[1:] <= row_ids[:-1])).any()):
                raise ValueError("the ids of a list must ascend")
        for t, name, dt in ((tags, "tags", torch.int32), (bias, "bias", torch.float32)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != (N,) or t.device != dev):
                raise ValueError(f"clustered {name} must be {dt} [N] on the catalogue's device "
                                 f"(got {t.dtype} {tuple(t.shape)})")
        self.row_ids = row_ids.contiguous()
        self.emb = emb.contiguous()
        self.list_off = list_off.contiguous()
        self.centroids = centroids.contiguous()
        self.tags = None if tags is None else tags.contiguous()
        self.bias = None if bias is None else bias.contiguous()
        self._ids = ids.contiguous()      # ascending
        self._order = order.contiguous()  # the clustered row of every id of _ids
        self._plain = None                # the flat catalogue without tags and bias, for recall
        self.groups = None                # the with_deep() view: int32 [N] in the rows' order

    @classmethod
    def from_assignment(cls, catalogue: ItemCatalogue, centroids: torch.Tensor, assign: torch.Tensor) -> "ClusteredItemCatalogue":
        """From a flat catalogue, caller-given ``centroids`` bf16 [L, 128] and the list of every item,
        ``assign`` integer [N] in [0, L).  Nothing ties an item to its nearest centroid here: the
        contract of ``topk`` holds for any assignment."""
        if not isinstance(catalogue, ItemCatalogue):
            raise ValueError("from_assignment takes an ItemCatalogue")
        if centroids.dim() != 2 or centroids.shape[1] != WIDTH or centroids.shape[0] < 1:
            raise ValueError(f"centroids must be [L, {WIDTH}], L >= 1 (got {tuple(centroids.shape)})")
        if centroids.dtype != torch.bfloat16:
            raise ValueError(f"centroids must be bf16, as the catalogue's rows are (got {centroids.dtype})")
        N, L = len(catalogue), centroids.shape[0]
        if assign.is_floating_point() or assign.dtype == torch.bool or tuple(assign.shape) != (N,):
            raise ValueError(f"assign must be an integer tensor [N], one list per item (got {assign.dtype} "
                             f"{tuple(assign.shape)}, N={N})")
        dev = catalogue.ids.device
        assign = assign.to(device=dev, dtype=torch.int64)
        if bool(((assign < 0) | (assign >= L)).any()):
            bad = int(assign[(assign < 0) | (assign >= L)][0])
            raise ValueError(f"assign must lie in 0..{L - 1}, the lists there are (got {bad})")
        order = torch.argsort(assign, stable=True)  # list-major, id-ascending inside a list
        counts = torch.bincount(assign, minlength=L)
        list_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)])
        pick = lambda t: t[order]
        return cls(catalogue.ids[order], catalogue.emb[order], list_off, centroids.to(dev),
                   _opt(catalogue.tags, pick), _opt(catalogue.bias, pick))

    @classmethod
    def _trusted(cls, row_ids, emb, list_off, centroids, tags, bias) -> "ClusteredItemCatalogue":
        """A catalogue of tensors that ``update`` produced from a checked catalogue: what the constructor
        checks holds by construction, so nothing is read back from the device.  The id lookup is the
        constructor's sort."""
        cat = object.__new__(ClusteredItemCatalogue)
        cat.row_ids, cat.emb, cat.list_off, cat.centroids, cat.tags, cat.bias = row_ids, emb, list_off, centroids, tags, bias
        ids, order = torch.sort(row_ids)
        cat._ids, cat._order = ids.contiguous(), order.contiguous()
        cat._plain = None
        cat.groups = None
        return cat

    @torch.no_grad()
    def update(self, upsert: Optional[ItemCatalogue] = None, remove_ids: Optional[torch.Tensor] = None, *,
               missing_ok: bool = False) -> "ClusteredItemCatalogue":
        """A new clustered catalogue around the same centroids: this one without the ``remove_ids`` (int64
        [R], distinct, on this device) and with the rows of ``upsert`` (an ``ItemCatalogue`` on this device,
        carrying tags and bias exactly when this catalogue does, and groups exactly when this view does).
        An upsert row, whether its id is new or replaces a row, goes to the list of its nearest centroid
        (``K.retrieve_topk`` with k = 1, ties to the lower list: ``cluster()``'s last assignment); every
        other row keeps its list.  The result equals, in every tensor, ``from_assignment`` of the updated
        flat catalogue with that assignment, and a ``with_filters()`` / ``with_deep()`` / ``with_heads()``
        view gives a view of its kind.  An id to remove that the catalogue does not hold is refused unless
        ``missing_ok``; so are an id in both arguments and a result without rows.  This catalogue is
        unchanged, the centroids are not re-fitted.

        Per list one merge of two ascending id sequences on the device (``K.catalogue_update``) instead of
        the rebuild's assignment, argsort and gathers of all N rows, with one device-to-host read, of the new
        row count and the verdicts on the ids."""
        who = "ClusteredItemCatalogue.update"
        dead, n_out = _update_dead(self, upsert, remove_ids, missing_ok, who)
        dev, L = self.emb.device, self.nlist
        if upsert is None:
            order, delta_off = None, torch.zeros(L + 1, dtype=torch.int64, device=dev)
        else:
            assign = K.retrieve_topk(upsert.emb, self.centroids, 1, normalize_q=False)[1][:, 0].long()
            order = torch.argsort(assign, stable=True)  # (list, id): the upsert's ids ascend
            delta_off = torch.searchsorted(assign[order], torch.arange(L + 1, dtype=torch.int64, device=dev))
        row_ids, emb, list_off, tags, bias, groups = K.catalogue_update(
            self.row_ids, self.emb, self.list_off, dead, delta_off=delta_off, tags=self.tags, bias=self.bias,
            groups=self.groups, n_out=n_out, **_update_delta(self, upsert, order))
        out = ClusteredItemCatalogue._trusted(row_ids, emb, list_off, self.centroids, tags, bias)
        if self.scans_deep or self.scans_heads:
            view = out.with_deep() if self.scans_deep else out.with_heads()
            view.groups = groups
            return view
        return out.with_filters() if self.scans_filters else out

    _MAX_K = K.RETRIEVE_MAX_K  # the longest list of topk (the with_deep() view: K.RETRIEVE_MAX_DEEP)

    def __len__(self) -> int:
        return self.row_ids.shape[0]

    @property
    def nlist(self) -> int:
        return self.centroids.shape[0]

    def list_lengths(self) -> torch.Tensor:
        """int64 [L]: the rows of every list."""
        return self.list_off[1:] - self.list_off[:-1]

    def to_flat(self) -> ItemCatalogue:
        """The id-sorted ``ItemCatalogue`` of the same items, bit for bit the one this was built from."""
        pick = lambda t: t[self._order]
        return ItemCatalogue(self._ids, pick(self.emb), _opt(self.tags, pick), _opt(self.bias, pick))

    def to(self, device) -> "ClusteredItemCatalogue":
        on = lambda t: t.to(device)
        out = ClusteredItemCatalogue(on(self.row_ids), on(self.emb), on(self.list_off), on(self.centroids),
                                     _opt(self.tags, on), _opt(self.bias, on))
        if self.scans_deep or self.scans_heads:
            view = out.with_deep() if self.scans_deep else out.with_heads()
            view.groups = _opt(self.groups, on)
            return view
        return out.with_filters() if self.scans_filters else out

    @property
    def scans_filters(self) -> bool:
        """Whether ``topk`` follows the flat catalogue's conventions (tags, bias, cursors): False here,
        True on the view ``with_filters()`` returns."""
        return False

    @property
    def scans_deep(self) -> bool:
        """Whether ``topk`` takes k up to ``K.RETRIEVE_MAX_DEEP`` = 1024 and the catalogue diversifies its
        own lists: False here, True on the view ``with_deep()`` returns."""
        return False

    @property
    def scans_heads(self) -> bool:
        """Whether ``topk`` takes several queries per user, ``q`` [U, G, 128], and scores an item by its
        best match over them: False here and on the other views, True on the view ``with_heads()``
        returns."""
        return False

    def _rows_of_groups(self, groups: Optional[torch.Tensor], who: str) -> Optional[torch.Tensor]:
        """``groups`` int32 [N] in ``to_flat()``'s (id-ascending) order, permuted into the clustered row
        order (None stays None)."""
        N = len(self)
        if groups is None:
            return None
        if not isinstance(groups, torch.Tensor) or groups.dtype != torch.int32 or tuple(groups.shape) != (N,):
            raise ValueError(f"{who} takes groups int32 [N], one key per item in to_flat()'s order "
                             f"(got {getattr(groups, 'dtype', type(groups).__name__)} "
                             f"{tuple(getattr(groups, 'shape', ()))}, N={N})")
        perm = torch.empty(N, dtype=torch.int32, device=self.emb.device)
        perm[self._order] = groups.to(self.emb.device)  # _order: the clustered row of the i-th id
        return perm

    def with_heads(self, groups: Optional[torch.Tensor] = None) -> "GroupedClusteredItemCatalogue":
        """A view over the same tensors (nothing is copied) that is a ``with_filters()`` view whose
        ``topk`` takes ``q`` [U, G, 128], G <= 8 queries per user (say one per lookahead head), and
        scores an item by its best match over them, one slot per item: see
        ``GroupedClusteredItemCatalogue``.  ``groups`` int32 [N] in ``to_flat()``'s order are carried in
        the clustered row order, as ``with_deep`` carries them, for a caller who diversifies the lists
        elsewhere; this view's own scan does not read them and it refuses ``group_cap``.  This
        catalogue is unchanged; neither the flag nor the groups are stored by ``save``."""
        groups = self._rows_of_groups(groups, "with_heads")
        view = object.__new__(GroupedClusteredItemCatalogue)
        view.__dict__.update(self.__dict__)
        view._flat = None
        view.groups = groups
        return view

    def with_deep(self, groups: Optional[torch.Tensor] = None) -> "DeepClusteredItemCatalogue":
        """A view over the same tensors (nothing is copied) that is a ``with_filters()`` view whose
        ``topk`` takes k up to 1024 and that has ``diversify``: see ``DeepClusteredItemCatalogue``.
        ``groups`` int32 [N], one key per item in ``to_flat()``'s (id-ascending) order, 0 = no group:
        the ``groups`` of the flat catalogue this was built from, for ``diversify``'s ``group_cap``.
        They are permuted once into the clustered row order.  This catalogue is unchanged; neither
        the flag nor the groups are stored by ``save``."""
        groups = self._rows_of_groups(groups, "with_deep")
        view = object.__new__(DeepClusteredItemCatalogue)
        view.__dict__.update(self.__dict__)
        view._flat = None
        view.groups = groups
        return view

    def with_filters(self) -> "FilteredClusteredItemCatalogue":
        """A view over the same tensors (nothing is copied) whose scan applies the catalogue's tags and
        bias and takes cursors, as ``ItemCatalogue.topk`` does: see ``FilteredClusteredItemCatalogue``.
        This catalogue is unchanged.  The flag is not stored by ``save``."""
        view = object.__new__(FilteredClusteredItemCatalogue)
        view.__dict__.update(self.__dict__)
        view._flat = None
        return view

    def _check_call(self, k: int, nprobe) -> Tuple[int, int]:
        return _check_probe_call(k, nprobe, self._MAX_K, self.nlist)

    def probe(self, q: torch.Tensor, nprobe: int, *, normalize_q: bool = True) -> torch.Tensor:
        """int32 [Q, nprobe]: the lists of the nprobe best centroids per query, best first
        (``K.retrieve_topk`` with the centroids as the catalogue: ties go to the lower list, and the
        row at nprobe is a prefix of the row at nprobe + 1)."""
        _, nprobe = self._check_call(1, nprobe)
        return K.retrieve_topk(q, self.centroids, nprobe, normalize_q=normalize_q)[1]

    def topk(self, q: torch.Tensor, k: int, *, nprobe: int, normalize_q: bool = True,
             exclude_ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scores f32 [Q, k], ids int64 [Q, k]): per query the k first, under (score descending, id
        ascending), of the items that lie in its ``nprobe`` nearest lists and are not among its
        ``exclude_ids`` (int64 [Q, X], X <= 1024; unknown ids and 0 exclude nothing), then (-inf, 0).
        Every score has the bits ``ItemCatalogue.topk`` returns for the same (query, item), and with
        ``nprobe`` = L the whole result is that of ``to_flat().topk`` on a catalogue without a bias.
        ``nprobe`` in 1..min(L, 64), ``k`` in 1..128, ``q`` [Q, 128]."""
        k, nprobe = self._check_call(k, nprobe)
        if q.dim() != 2:
            raise ValueError(f"a clustered catalogue takes [Q, {WIDTH}] queries, one per row (got {tuple(q.shape)})")
        _check_exclude(exclude_ids)
        xr = _opt(exclude_ids, lambda x: self.rows_of(x).contiguous())
        probes = self.probe(q, nprobe, normalize_q=normalize_q)
        return K.retrieve_ivf_topk(q, self.emb, self.row_ids, self.list_off, probes, k, normalize_q=normalize_q,
                                   exclude_rows=xr)

    _REFUSAL = "retrieve with a clustered catalogue does not take {}: use catalogue.to_flat() for it"
    _NO_RANKS = "catalogue_metrics counts exact ranks, which take the flat scan: pass catalogue.to_flat()"

    @property
    def retrieve_takes(self) -> frozenset:
        """``nprobe``; a ``with_filters()`` view also the tags, the cursor and the weight it scans with, a
        ``with_heads()`` view also ``heads``, a ``with_deep()`` view also what diversifies its own lists."""
        takes = {"nprobe"}
        if self.scans_filters:
            takes |= {*_TAGS, "after", "bias_weight"}
        if self.scans_heads:
            takes |= {"heads"}
        if self.scans_deep:
            takes |= {"diversity", "pool", "group_cap"}
        return frozenset(takes)

    def _check_retrieve(self, k, given: dict) -> None:
        _refuse_shortlist(given)
        _refuse_named(self, given)
        _need_nprobe(given)
        self._check_call(k, given["nprobe"])

    def _retrieve(self, q, k, nprobe, shortlist, exclude_ids, tag_filter, after_scores, after_ids, bias_weight):
        scores, item_ids = self.topk(q, k, nprobe=nprobe, normalize_q=True, exclude_ids=exclude_ids)
        return item_ids, scores

    def recall(self, q: torch.Tensor, k: int, nprobe: int) -> float:
        """The mean over the queries of the fraction of the flat scan's top-k ids (plain dots, no
        filter) that ``topk(q, k, nprobe=nprobe)`` returns.  Never decreases in ``nprobe``; 1.0 at L."""
        if self._plain is None:
            self._plain = ItemCatalogue(self._ids, self.emb[self._order])
        return _hit_fraction(self._plain.topk(q, k)[0], self.topk(q, k, nprobe=nprobe)[1], k)

    def quantize(self, keep_exact: bool = True) -> "QuantizedClusteredItemCatalogue":
        """This catalogue as e4m3 codes with one power-of-two scale per row, in the same lists
        (``K.quantize_catalogue_q8`` of the clustered rows, on the catalogue's device), with its tags and
        bias, and with ``keep_exact`` the bf16 rows beside the codes for re-scoring: see
        ``QuantizedClusteredItemCatalogue``.  Groups are not carried."""
        codes, scale = K.quantize_catalogue_q8(self.emb)
        return QuantizedClusteredItemCatalogue(self.row_ids, codes, scale, self.list_off, self.centroids, self.tags,
                                               self.bias, self.emb if keep_exact else None)

    def save(self, path: str) -> None:
        """The flat catalogue's file (``ItemCatalogue.load`` reads it as the id-sorted catalogue) with
        ``row_ids``, ``list_off`` and ``centroids`` beside its tensors."""
        flat = self.to_flat()
        _save(path, {"ids": flat.ids, "emb": flat.emb, "row_ids": self.row_ids, "list_off": self.list_off,
                     "centroids": self.centroids, "tags": flat.tags, "bias": flat.bias}, IVF_INDEX)

    @classmethod
    def load(cls, path: str, *, device=None) -> "ClusteredItemCatalogue":
        with _opened(path, IVF_INDEX, "a clustered item catalogue") as get:
            flat = ItemCatalogue(get("ids"), get("emb"), get("tags", True), get("bias", True))
            row_ids, list_off, centroids = get("row_ids"), get("list_off"), get("centroids")
        rows = flat.rows_of(row_ids).long()
        if row_ids.shape != flat.ids.shape or bool((rows < 0).any()):
            raise ValueError(f"{path}: row_ids are not the catalogue's ids")
        pick = lambda t: t[rows]
        cat = cls(row_ids, pick(flat.emb), list_off, centroids, _opt(flat.tags, pick), _opt(flat.bias, pick))
        return cat.to(device) if device is not None else cat


class FilteredClusteredItemCatalogue(ClusteredItemCatalogue):
    """``ClusteredItemCatalogue.with_filters()``: the same tensors, scanned under the flat catalogue's
    conventions (``K.retrieve_ivf_topk`` with tags, bias and cursor; csrc/retrieve.hip
    ``retr_ivf_topk_k<true, true, TAGS, BIAS>``).  A catalogue that carries a bias scores with it, a
    ``tag_filter`` needs tags, and a cursor is a (score, id) position.  Everything else (``probe``,
    ``rows_of``, ``to_flat``, ``save``, the limits on ``nprobe`` and ``k``) is the plain catalogue's."""

    @property
    def scans_filters(self) -> bool:
        return True

    def with_filters(self) -> "FilteredClusteredItemCatalogue":
        return self

    filter_like = _IdIndex._filter_like

    def _check_filters(self, q, tag_filter, after_scores, after_ids, bias_weight) -> None:
        if q.dim() != 2:
            raise ValueError(f"a clustered catalogue takes [Q, {WIDTH}] queries, one per row (got {tuple(q.shape)})")
        _check_tag_filter(self, tag_filter, q.shape[0])
        _check_bias_weight(self, bias_weight, q.shape[0])
        _check_cursor(after_scores, after_ids, q.shape[0])

    def _scan_args(self, exclude_ids, tag_filter, after_scores, after_ids, bias_weight) -> dict:
        """The filter keywords of ``K.retrieve_ivf_topk`` / ``K.retrieve_ivf_topk_group`` for checked arguments."""
        _check_exclude(exclude_ids)
        tight = lambda t: t.contiguous()
        return dict(exclude_rows=_opt(exclude_ids, lambda x: self.rows_of(x).contiguous()),
                    tags=self.tags if tag_filter is not None else None, tag_filter=_opt(tag_filter, tight), bias=self.bias,
                    bias_weight=bias_weight, after_scores=_opt(after_scores, tight), after_ids=_opt(after_ids, tight))

    def topk(self, q: torch.Tensor, k: int, *, nprobe: int, normalize_q: bool = True,
             exclude_ids: Optional[torch.Tensor] = None, tag_filter: Optional[torch.Tensor] = None,
             after_scores: Optional[torch.Tensor] = None, after_ids: Optional[torch.Tensor] = None,
             bias_weight: Union[None, float, torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scores f32 [Q, k], ids int64 [Q, k]): per query the k first, under (score descending, id
        ascending), of the items that lie in its ``nprobe`` nearest lists, are not among its
        ``exclude_ids``, pass its ``tag_filter`` (int32 [Q, 3] = (all, any, none); the catalogue must
        carry tags) and lie strictly behind (``after_scores`` f32 [Q], ``after_ids`` int64 [Q]; together
        or neither), then (-inf, 0).  A catalogue that carries a ``bias`` scores item j as
        fma(w, bias[j], q . e_j), with ``bias_weight`` = w: None for 1, a number or f32 [Q]; one without
        refuses a weight.  Every score has the bits ``ItemCatalogue.topk`` returns for the same (query,
        item) and arguments, and with ``nprobe`` = L the whole result is ``to_flat().topk``'s.  The probes
        depend on ``q`` only, so with the same ``nprobe`` the last (score, id) of one page as the next
        page's cursor yields the following k items, and the (-inf, 0) of an exhausted page an empty one."""
        k, nprobe = self._check_call(k, nprobe)
        self._check_filters(q, tag_filter, after_scores, after_ids, bias_weight)
        kw = self._scan_args(exclude_ids, tag_filter, after_scores, after_ids, bias_weight)
        probes = self.probe(q, nprobe, normalize_q=normalize_q)
        return K.retrieve_ivf_topk(q, self.emb, self.row_ids, self.list_off, probes, k, normalize_q=normalize_q,
                                   deep=self.scans_deep, **kw)

    def _retrieve(self, q, k, nprobe, shortlist, exclude_ids, tag_filter, after_scores, after_ids, bias_weight):
        scores, item_ids = self.topk(q, k, nprobe=nprobe, normalize_q=True, exclude_ids=exclude_ids, tag_filter=tag_filter,
                                     after_scores=after_scores, after_ids=after_ids, bias_weight=bias_weight)
        return item_ids, scores

    def recall(self, q: torch.Tensor, k: int, nprobe: int, **filters) -> float:
        """The mean over the queries of the fraction of ``to_flat().topk(q, k, **filters)``'s ids that
        ``topk(q, k, nprobe=nprobe, **filters)`` returns (``filters``: ``exclude_ids``, ``tag_filter``,
        ``after_scores`` / ``after_ids``, ``bias_weight``), over the queries whose flat list is not
        empty (1.0 where every one is).  Never decreases in ``nprobe``; 1.0 at L."""
        if self._flat is None:
            self._flat = self.to_flat()
        return _hit_fraction(self._flat.topk(q, k, **filters)[0], self.topk(q, k, nprobe=nprobe, **filters)[1], k)


class DeepClusteredItemCatalogue(FilteredClusteredItemCatalogue):
    """``ClusteredItemCatalogue.with_deep(groups)``: the ``with_filters()`` view of the same tensors
    whose lists reach k = ``K.RETRIEVE_MAX_DEEP`` = 1024 (``K.retrieve_ivf_topk(deep=True)``;
    csrc/retrieve.hip ``retr_ivf_deep_topk_k``), the length a ranking stage or ``diversify`` takes.
    ``topk`` and ``recall`` are the filtered view's, argument for argument, with k in 1..1024: k <= 128
    runs the kernels it runs there, and above every score keeps the bits ``ItemCatalogue.topk``
    returns.  ``groups`` int32 [N] in the clustered row order, or None."""

    _MAX_K = K.RETRIEVE_MAX_DEEP
    _DIVERSIFY_QUERIES = 1024  # the queries of one diversify call: their pools' rows are gathered (256 MiB at M = 1024)

    @property
    def scans_deep(self) -> bool:
        return True

    @property
    def has_groups(self) -> bool:
        return self.groups is not None

    def with_deep(self, groups: Optional[torch.Tensor] = None) -> "DeepClusteredItemCatalogue":
        return self if groups is None else ClusteredItemCatalogue.with_deep(self, groups)

    def diversify(self, item_ids: torch.Tensor, scores: torch.Tensor, k: int, *,
                  lam: Union[float, torch.Tensor] = 1.0, group_cap: Optional[int] = None):
        """``ItemCatalogue.diversify`` on this catalogue's own rows, under its contract and checks:
        (item_ids int64 [Q, k], scores f32 [Q, k], objective f32 [Q, k]) in selection order, for a pool
        ``item_ids`` int64 [Q, M] / ``scores`` f32 [Q, M], M <= 1024, k <= 128, ``lam`` a number or a
        float tensor [Q] in [0, 1], ``group_cap`` with the ``groups`` given to ``with_deep``.  The
        result is, in all three outputs, what ``to_flat()`` with those groups returns for the pool.

        ``K.retrieve_diversify`` breaks ties by the lower row, and "the lower row" means "the lower
        id" only where rows ascend with ids, which the clustered order does not across lists.  So
        the pool's distinct items are gathered from the clustered ``emb`` (through ``rows_of``) into
        an id-ascending block, at most ``_DIVERSIFY_QUERIES`` queries' pools at a time, and the kernel
        runs on that block: the catalogue itself is neither copied nor re-ordered."""
        if item_ids.dtype != torch.int64 or item_ids.dim() != 2:
            raise ValueError(f"diversify takes int64 item_ids [Q, M] (got {item_ids.dtype} {tuple(item_ids.shape)})")
        if scores.dtype != torch.float32 or scores.shape != item_ids.shape:
            raise ValueError(f"diversify takes f32 scores of the ids' shape (got {scores.dtype} {tuple(scores.shape)})")
        if group_cap is not None and self.groups is None:
            raise ValueError("group_cap given, but this catalogue carries no groups")
        Q = item_ids.shape[0]
        dev = self.emb.device
        step = self._DIVERSIFY_QUERIES
        outs = []
        for q0 in range(0, max(Q, 1), step):
            pool = item_ids[q0:q0 + step].to(dev)
            held = torch.unique(pool)  # ascending
            rows = self.rows_of(held).long()
            held, rows = held[rows >= 0], rows[rows >= 0]
            if held.numel() == 0:  # no candidate at all: a catalogue is never empty, so one row stands in
                held, rows = self.row_ids[:1], torch.zeros(1, dtype=torch.int64, device=dev)
            block = ItemCatalogue(held, self.emb[rows], groups=None if self.groups is None else self.groups[rows])
            outs.append(block.diversify(pool, scores[q0:q0 + step], k, group_cap=group_cap,
                                        lam=lam[q0:q0 + step] if isinstance(lam, torch.Tensor) and lam.dim() == 1 else lam))
        return tuple(torch.cat([o[i] for o in outs]) for i in range(3))


class GroupedClusteredItemCatalogue(FilteredClusteredItemCatalogue):
    """``ClusteredItemCatalogue.with_heads()``: the ``with_filters()`` view of the same tensors whose
    queries come in groups, ``q`` [U, G, 128] with G <= ``K.RETRIEVE_MAX_GROUP`` = 8 per user
    (``K.retrieve_ivf_topk_group``; csrc/retrieve.hip ``retr_ivf_topk_k<true, true, TAGS, BIAS, true>``).
    An item's score is its best over the user's queries, taken inside the scan ahead of candidate
    selection, so an item takes one slot per user and the order of a user's queries does not matter.
    A user probes one set of lists: the ``nprobe`` centroids that score best for any of its queries.
    ``exclude_ids``, ``tag_filter``, ``after_scores`` / ``after_ids`` and ``bias_weight`` are the
    filtered view's, one per user; k stays in 1..128.  A 2-D ``q`` [Q, 128] is G = 1, the filtered
    view's own call."""

    @property
    def scans_heads(self) -> bool:
        return True

    def with_heads(self, groups: Optional[torch.Tensor] = None) -> "GroupedClusteredItemCatalogue":
        return self if groups is None else ClusteredItemCatalogue.with_heads(self, groups)

    @staticmethod
    def _grouped(q: torch.Tensor) -> torch.Tensor:
        if q.dim() == 2:
            return q[:, None, :]
        if q.dim() != 3 or not 1 <= q.shape[1] <= K.RETRIEVE_MAX_GROUP:
            raise ValueError(f"a with_heads() view takes [U, G, {WIDTH}] queries, G in 1..{K.RETRIEVE_MAX_GROUP} "
                             f"per user (got {tuple(q.shape)})")
        return q

    def probe(self, q: torch.Tensor, nprobe: int, *, normalize_q: bool = True) -> torch.Tensor:
        """int32 [U, nprobe]: per user the lists of the nprobe first centroids under (the centroid's best
        score over the user's queries descending, list ascending): ``K.retrieve_topk_group`` with the
        centroids as the catalogue.  At G = 1 (and for a 2-D ``q``) it is the plain catalogue's ``probe``."""
        _, nprobe = self._check_call(1, nprobe)
        q = self._grouped(q)
        if q.shape[1] == 1:
            return K.retrieve_topk(q[:, 0].contiguous(), self.centroids, nprobe, normalize_q=normalize_q)[1]
        return K.retrieve_topk_group(q.contiguous(), self.centroids, nprobe, normalize_q=normalize_q)[1]

    def topk(self, q: torch.Tensor, k: int, *, nprobe: int, normalize_q: bool = True,
             exclude_ids: Optional[torch.Tensor] = None, tag_filter: Optional[torch.Tensor] = None,
             after_scores: Optional[torch.Tensor] = None, after_ids: Optional[torch.Tensor] = None,
             bias_weight: Union[None, float, torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scores f32 [U, k], ids int64 [U, k]): the filtered view's ``topk``, argument for argument,
        for ``q`` [U, G, 128]: per user the k first, under (score descending, id ascending), of the items
        that lie in the user's ``nprobe`` lists (``probe``), are not among its ``exclude_ids`` [U, X],
        pass its ``tag_filter`` [U, 3] and lie strictly behind its cursor, then (-inf, 0), on the score
        max_g q[u, g] . e_j (with a bias, fma(w[u], bias[j], that maximum)).  No item appears twice in a
        user's list.  Every score has the bits ``ItemCatalogue.topk`` returns for the same 3-D ``q`` and
        arguments, and with ``nprobe`` = L the whole result is ``to_flat().topk``'s."""
        k, nprobe = self._check_call(k, nprobe)
        q = self._grouped(q)
        self._check_filters(q[:, 0], tag_filter, after_scores, after_ids, bias_weight)
        kw = self._scan_args(exclude_ids, tag_filter, after_scores, after_ids, bias_weight)
        probes = self.probe(q, nprobe, normalize_q=normalize_q)
        if q.shape[1] == 1:
            return K.retrieve_ivf_topk(q[:, 0].contiguous(), self.emb, self.row_ids, self.list_off, probes, k,
                                       normalize_q=normalize_q, **kw)
        return K.retrieve_ivf_topk_group(q.contiguous(), self.emb, self.row_ids, self.list_off, probes, k,
                                         normalize_q=normalize_q, **kw)


IVF_Q8_INDEX = "lthm-ivf-q8-v1"


class QuantizedClusteredItemCatalogue(_IdIndex):
    """``ClusteredItemCatalogue.quantize()``: the clustered catalogue stored as OCP e4m3fn codes, small and
    cheap to query at once, and still able to filter.

    ``row_ids`` int64 [N] in the clustered (list, id) order, ``list_off`` int64 [L + 1] and ``centroids``
    bf16 [L, 128] as the source has them; ``codes`` uint8 [N, 128] and ``scale`` f32 [N],
    ``K.quantize_catalogue_q8`` of the clustered rows; ``tags`` int32 [N] / ``bias`` f32 [N] in the rows'
    order or None; ``emb`` bf16 [N, 128], the exact rows, or None.  The centroids stay bf16 and ``probe`` is
    the bf16 catalogue's, so a query scans exactly the lists it scans there.  ``topk`` scans the probed
    lists' codes for a shortlist of the eligible rows (``K.retrieve_ivf_q8_topk``) and, where the exact
    rows are kept, re-scores the shortlist in bf16 with the prior (``K.retrieve_rescore_bias``): the
    result is the ``with_filters()`` / ``with_deep()`` list with the same arguments restricted to the
    shortlist, so it equals that list whenever the shortlist holds its first k.  One query per row;
    cursors, heads, diversification and target ranks are not offered here."""

    def __init__(self, row_ids: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor, list_off: torch.Tensor,
                 centroids: torch.Tensor, tags: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                 emb: Optional[torch.Tensor] = None):
        if row_ids.dtype != torch.int64 or row_ids.dim() != 1 or row_ids.shape[0] < 1:
            raise ValueError(f"clustered row_ids must be int64 [N], N >= 1 (got {row_ids.dtype} {tuple(row_ids.shape)})")
        N = row_ids.shape[0]
        if codes.dtype != torch.uint8 or tuple(codes.shape) != (N, WIDTH):
            raise ValueError(f"catalogue codes must be uint8 [N, {WIDTH}] (got {codes.dtype} {tuple(codes.shape)}, N={N})")
        if scale.dtype != torch.float32 or tuple(scale.shape) != (N,):
            raise ValueError(f"catalogue scales must be f32 [N] (got {scale.dtype} {tuple(scale.shape)}, N={N})")
        if emb is not None and (emb.dtype != torch.bfloat16 or tuple(emb.shape) != (N, WIDTH)):
            raise ValueError(f"clustered embeddings must be bf16 [N, {WIDTH}] (got {emb.dtype} {tuple(emb.shape)}, N={N})")
        if centroids.dim() != 2 or centroids.shape[1] != WIDTH or centroids.shape[0] < 1:
            raise ValueError(f"centroids must be [L, {WIDTH}], L >= 1 (got {tuple(centroids.shape)})")
        if centroids.dtype != torch.bfloat16:
            raise ValueError(f"centroids must be bf16, as the catalogue's rows are (got {centroids.dtype})")
        L = centroids.shape[0]
        if list_off.dtype != torch.int64 or tuple(list_off.shape) != (L + 1,):
            raise ValueError(f"list_off must be int64 [L + 1] (got {list_off.dtype} {tuple(list_off.shape)}, L={L})")
        dev = codes.device
        if any(t.device != dev for t in (row_ids, scale, list_off, centroids)) or (emb is not None and emb.device != dev):
            raise ValueError("a clustered catalogue's tensors must live on one device")
        if int(list_off[0]) != 0 or int(list_off[-1]) != N or bool((list_off[1:] < list_off[:-1]).any()):
            raise ValueError("list_off must ascend from 0 to N")
        ids, order = torch.sort(row_ids)
        if bool((ids == 0).any()):
            raise ValueError("catalogue ids must not hold 0, the pad id")
        if N > 1 and bool((ids[1:] == ids[:-1]).any()):
            raise ValueError("catalogue ids must be distinct")
        if N > 1:
            inside = torch.ones(N - 1, dtype=torch.bool, device=dev)  # row i and row i + 1 share a list
            cut = list_off[1:-1]
            cut = cut[(cut > 0) & (cut < N)]
            inside[cut - 1] = False
            if bool((inside & (row_ids[1:] <= row_ids[:-1])).any()):
                raise ValueError("the ids of a list must ascend")
        for t, name, dt in ((tags, "tags", torch.int32), (bias, "bias", torch.float32)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != (N,) or t.device != dev):
                raise ValueError(f"clustered {name} must be {dt} [N] on the catalogue's device "
                                 f"(got {t.dtype} {tuple(t.shape)})")
        self.row_ids = row_ids.contiguous()
        self.codes = codes.contiguous()
        self.scale = scale.contiguous()
        self.list_off = list_off.contiguous()
        self.centroids = centroids.contiguous()
        self.tags = None if tags is None else tags.contiguous()
        self.bias = None if bias is None else bias.contiguous()
        self.emb = None if emb is None else emb.contiguous()
        self._ids = ids.contiguous()      # ascending
        self._order = order.contiguous()  # the clustered row of every id of _ids
        self._exact = None                # the bf16 with_deep() view, for recall

    def __len__(self) -> int:
        return self.row_ids.shape[0]

    @property
    def nlist(self) -> int:
        return self.centroids.shape[0]

    @property
    def keep_exact(self) -> bool:
        return self.emb is not None

    list_lengths = ClusteredItemCatalogue.list_lengths
    filter_like = _IdIndex._filter_like

    def update(self, *args, **kwargs):
        """Refused: the codes and scales are made per catalogue by ``quantize()``."""
        _no_update("a QuantizedClusteredItemCatalogue", "update the bf16 ClusteredItemCatalogue and call quantize() again")

    def to(self, device) -> "QuantizedClusteredItemCatalogue":
        on = lambda t: _opt(t, lambda t: t.to(device))
        return QuantizedClusteredItemCatalogue(on(self.row_ids), on(self.codes), on(self.scale), on(self.list_off),
                                               on(self.centroids), on(self.tags), on(self.bias), on(self.emb))

    def to_clustered(self) -> ClusteredItemCatalogue:
        """The bf16 clustered catalogue over the same lists, tags and bias; needs ``keep_exact``."""
        if self.emb is None:
            raise ValueError("to_flat needs the exact rows: this catalogue was built with keep_exact=False")
        return ClusteredItemCatalogue(self.row_ids, self.emb, self.list_off, self.centroids, self.tags, self.bias)

    def to_flat(self) -> ItemCatalogue:
        """The exact id-sorted ``ItemCatalogue`` of the same items, with tags and bias; needs ``keep_exact``."""
        return self.to_clustered().to_flat()

    @staticmethod
    def default_shortlist(k: int) -> int:
        return QuantizedItemCatalogue.default_shortlist(k)

    _MAX_K = K.RETRIEVE_Q8_MAX_POOL
    _check_call = ClusteredItemCatalogue._check_call
    probe = ClusteredItemCatalogue.probe

    retrieve_takes = frozenset({*_TAGS, "bias_weight", "nprobe", "shortlist"})
    _REFUSAL = "retrieve with a quantised clustered catalogue does not take {}: use catalogue.to_clustered() for it"
    _NO_RANKS = ("catalogue_metrics does not take a quantised clustered catalogue: it counts exact ranks, "
                 "which take the flat scan (pass catalogue.to_flat())")

    def _check_retrieve(self, k, given: dict) -> None:
        _refuse_named(self, given)
        _need_nprobe(given)
        self._check_call(k, given["nprobe"])
        _check_shortlist(k, given["shortlist"], keyword=True)
        _check_bias_weight(self, given["bias_weight"])
        if any(given[name] is not None for name in _TAGS) and not self.has_tags:
            raise ValueError("tag_all / tag_any / tag_none given, but this catalogue carries no tags")

    def _retrieve(self, q, k, nprobe, shortlist, exclude_ids, tag_filter, after_scores, after_ids, bias_weight):
        return self.topk(q, k, nprobe=nprobe, shortlist=shortlist, rescore=self.keep_exact, normalize_q=True,
                         exclude_ids=exclude_ids, tag_filter=tag_filter, bias_weight=bias_weight)

    def topk(self, q: torch.Tensor, k: int, *, nprobe: int, shortlist: Optional[int] = None, rescore: bool = True,
             normalize_q: bool = True, exclude_ids: Optional[torch.Tensor] = None,
             tag_filter: Optional[torch.Tensor] = None,
             bias_weight: Union[None, float, torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(item_ids int64 [Q, k], scores f32 [Q, k]), empty slots (0, -inf), as ``QuantizedItemCatalogue.topk``
        returns them.  Stage one: of the rows that lie in the query's ``nprobe`` nearest lists, are not among
        its ``exclude_ids`` (int64 [Q, X], X <= 1024) and pass its ``tag_filter`` (int32 [Q, 3]), the
        ``shortlist`` first (default min(max(4 k, 128), 1024); in k..1024) under the approximate e4m3 score,
        which a catalogue that carries a ``bias`` ranks as fma(w, bias[j], s^) (``bias_weight`` = w: None for
        1, a number or f32 [Q]; a catalogue without a bias refuses a weight).  Stage two (``rescore=True``,
        needs ``keep_exact``): those rows get the exact score fma(w, bias[j], q . e_j), with the bits
        ``ClusteredItemCatalogue.with_filters()`` / ``with_deep()`` return, and the k first under (score
        descending, id ascending) are returned.  ``rescore=False`` returns the first k of the shortlist
        with the approximate scores.  ``k`` in 1..1024, ``q`` [Q, 128]."""
        k, nprobe = self._check_call(k, nprobe)
        M = _check_shortlist(k, shortlist)
        if rescore and self.emb is None:
            raise ValueError("rescore=True needs the exact rows: this catalogue was built with keep_exact=False "
                             "(pass rescore=False)")
        _check_tag_filter(self, tag_filter)
        _check_bias_weight(self, bias_weight)
        if q.dim() != 2:
            raise ValueError(f"a quantised catalogue takes [Q, {WIDTH}] queries, one per row (got {tuple(q.shape)})")
        _check_exclude(exclude_ids)
        _check_tag_filter(self, tag_filter, q.shape[0])
        _check_bias_weight(self, bias_weight, q.shape[0])
        xr = _opt(exclude_ids, lambda x: self.rows_of(x).contiguous())
        probes = self.probe(q, nprobe, normalize_q=normalize_q)
        scores, rows = K.retrieve_ivf_q8_topk(q, self.codes, self.scale, self.row_ids, self.list_off, probes, M,
                                              normalize_q=normalize_q, exclude_rows=xr,
                                              tags=self.tags if tag_filter is not None else None,
                                              tag_filter=_opt(tag_filter, lambda t: t.contiguous()),
                                              bias=self.bias, bias_weight=bias_weight)
        if rescore:
            scores, rows = K.retrieve_rescore_bias(q, self.emb, rows, k, normalize_q=normalize_q, bias=self.bias,
                                                   bias_weight=bias_weight, order_ids=self.row_ids)
        else:
            scores, rows = scores[:, :k].contiguous(), rows[:, :k].contiguous()
        return self._ids_of(rows), scores

    def recall(self, q: torch.Tensor, k: int, nprobe: int, shortlist: Optional[int] = None, **filters) -> float:
        """The mean over the queries of the fraction of the bf16 clustered list's ids (``with_deep()`` with
        the same ``nprobe`` and ``filters``: ``exclude_ids``, ``tag_filter``, ``bias_weight``) that
        ``topk(q, k, nprobe=nprobe, shortlist=shortlist, **filters)`` returns, over the queries whose bf16
        list is not empty (1.0 where every one is); needs ``keep_exact``."""
        if self._exact is None:
            self._exact = self.to_clustered().with_deep()
        return _hit_fraction(self._exact.topk(q, k, nprobe=nprobe, **filters)[1],
                             self.topk(q, k, nprobe=nprobe, shortlist=shortlist, **filters)[0], k)

    def save(self, path: str) -> None:
        """safetensors with the catalogue's tensors under their names (``emb`` where the exact rows are kept),
        all in the clustered order, and the format tag of this kind of catalogue."""
        _save(path, {"row_ids": self.row_ids, "codes": self.codes, "scale": self.scale, "list_off": self.list_off,
                     "centroids": self.centroids, "tags": self.tags, "bias": self.bias, "emb": self.emb}, IVF_Q8_INDEX)

    @classmethod
    def load(cls, path: str, *, device=None) -> "QuantizedClusteredItemCatalogue":
        with _opened(path, IVF_Q8_INDEX, "a quantised clustered item catalogue") as get:
            cat = cls(get("row_ids"), get("codes"), get("scale"), get("list_off"), get("centroids"), get("tags", True),
                      get("bias", True), get("emb", True))
        return cat.to(device) if device is not None else cat


class ShardedItemCatalogue(_Catalogue):
    """One catalogue held as shards: ``local_shards`` are the ``ItemCatalogue``s of this process (on
    one device or on several; disjoint ids, checked here), and with ``group`` the catalogue also
    covers the shards of the group's other ranks.  All shards agree on carrying tags and on carrying
    a bias.  At most ``K.RETRIEVE_MAX_SHARDS`` = 64 shards in all.  The merged catalogue carries no
    groups, whatever its shards hold: its lists are diversified against a flat catalogue over the
    same items (``ItemCatalogue.diversify`` takes the ids ``topk`` returns).

    With a ``group`` the constructor, ``topk``, ``filter_like``, ``holds``, ``target_ranks`` and
    ``validate`` are collectives: every rank calls them, with the same queries, and every rank gets
    the full result.  Disjointness across ranks is not checked here; ``validate()`` does it."""

    def __init__(self, local_shards: Sequence[ItemCatalogue], group=None):
        shards = list(local_shards)
        if not shards or not all(isinstance(s, ItemCatalogue) for s in shards):
            raise ValueError("ShardedItemCatalogue takes one or more ItemCatalogue shards")
        if len({s.has_tags for s in shards}) != 1:
            raise ValueError("the shards of a catalogue all carry tags, or none does")
        if len({s.has_bias for s in shards}) != 1:
            raise ValueError("the shards of a catalogue all carry a bias, or none does")
        dev = shards[0].ids.device
        ids = torch.sort(torch.cat([s.ids.to(dev) for s in shards]))[0]
        if ids.numel() > 1 and bool((ids[1:] == ids[:-1]).any()):
            bad = int(ids[1:][ids[1:] == ids[:-1]][0])
            raise ValueError(f"the shards of a catalogue hold disjoint ids (id {bad} is in two of them)")
        self.shards = shards
        self.group = group
        self.device = dev
        self._total = int(ids.numel())
        self._pad_to = len(shards)       # local lists per rank in a gather
        self._max_items = self._total    # most items of one rank
        n_all = len(shards)
        if group is not None:
            mine = torch.tensor([len(shards), self._total, int(shards[0].has_tags), int(shards[0].has_bias)],
                                dtype=torch.int64, device=dev)
            every = all_gather_stack(mine, group).cpu()
            if bool((every[:, 2] != every[0, 2]).any()) or bool((every[:, 3] != every[0, 3]).any()):
                raise ValueError("the shards of a catalogue all carry tags / a bias, or none does (the ranks disagree)")
            self._pad_to = int(every[:, 0].max())
            self._total = int(every[:, 1].sum())
            self._max_items = int(every[:, 1].max())
            n_all = self._pad_to * every.shape[0]  # the merge sees every rank's lists padded to the longest
        if n_all > K.RETRIEVE_MAX_SHARDS:
            raise ValueError(f"a sharded catalogue takes at most {K.RETRIEVE_MAX_SHARDS} shards (got {n_all})")

    def __len__(self) -> int:
        return self._total

    @property
    def has_tags(self) -> bool:
        return self.shards[0].has_tags

    @property
    def has_bias(self) -> bool:
        return self.shards[0].has_bias

    def update(self, *args, **kwargs):
        """Refused: an id belongs to one shard, and only the caller knows which."""
        _no_update("a ShardedItemCatalogue", "update the shards (ItemCatalogue.update) and construct the sharded catalogue again")

    def validate(self) -> None:
        """Disjointness of the ids across the ranks of the group: one all-gather of every rank's ids
        (padded with 0, which no catalogue holds, to the longest), one sort."""
        dev = self.device
        ids = torch.cat([s.ids.to(dev) for s in self.shards])
        if self.group is not None:
            pad = torch.zeros(self._max_items, dtype=torch.int64, device=dev)
            pad[:ids.numel()] = ids
            ids = all_gather_stack(pad, self.group).reshape(-1)
            ids = ids[ids != 0]
        ids = torch.sort(ids)[0]
        if ids.numel() > 1 and bool((ids[1:] == ids[:-1]).any()):
            bad = int(ids[1:][ids[1:] == ids[:-1]][0])
            raise ValueError(f"the shards of a catalogue hold disjoint ids (id {bad} is in two of them)")

    def _reduce_max(self, t: torch.Tensor) -> torch.Tensor:
        return t if self.group is None else all_reduce_max(t, self.group)

    def holds(self, ids: torch.Tensor) -> torch.Tensor:
        """bool, the shape of ``ids``: some shard holds this id."""
        dev = self.device
        found = torch.stack([s.holds(ids).to(dev) for s in self.shards]).any(dim=0)
        return self._reduce_max(found.to(torch.int32)).bool()

    def filter_like(self, target_ids: torch.Tensor, mask: int) -> torch.Tensor:
        """``ItemCatalogue.filter_like`` over the union: the target's tag word comes from the shard
        that holds it (at most one does: the words and a found flag are MAX-combined)."""
        if not self.has_tags:
            raise ValueError("filter_like needs a catalogue with tags")
        if target_ids.dim() != 1:
            raise ValueError("filter_like takes target ids [Q]")
        dev = self.device
        both = torch.zeros((2, target_ids.numel()), dtype=torch.int64, device=dev)  # found, the word's 32 bits
        for s in self.shards:
            rows = s.rows_of(target_ids).long()
            word = s.tags[rows.clamp(min=0)].long() & 0xFFFFFFFF
            both = torch.maximum(both, torch.stack([(rows >= 0).long(), torch.where(rows >= 0, word, 0)]).to(dev))
        both = self._reduce_max(both)
        t = both[1]
        return _filter_row(torch.where(t >= (1 << 31), t - (1 << 32), t), both[0] > 0, mask, dev)

    def _scan(self, q, k, normalize_q, target_ids, slab_rows, exclude_ids, tag_filter, after_scores, after_ids,
              bias_weight, use_bias):
        _check_tag_filter(self, tag_filter)
        _check_bias_weight(self, bias_weight)
        _check_cursor(after_scores, after_ids)
        _check_exclude(exclude_ids)
        k = int(k)
        if not 1 <= k <= K.RETRIEVE_MAX_DEEP:
            raise ValueError(f"topk takes k in 1..{K.RETRIEVE_MAX_DEEP} (got {k})")
        home = q.device
        call = K.retrieve_topk_group if q.dim() == 3 else K.retrieve_topk
        if isinstance(bias_weight, (int, float)) and not isinstance(bias_weight, bool) and use_bias:
            bias_weight = torch.full((q.shape[0],), float(bias_weight), dtype=torch.float32, device=home)
        on = lambda t, dev: None if t is None else t.to(dev).contiguous()
        # 1, 2: the target's score, from the one shard that holds the target
        tscore = tscore_out = None
        trows = [None] * len(self.shards)
        if target_ids is not None:
            tscore, tscore_out, trows = _sharded_target_score(self.shards, q, target_ids, normalize_q, bias_weight, use_bias,
                                                              self._reduce_max)
        # 3: every local shard's list, its rows as ids
        ls, li, lr = [], [], []
        for i, s in enumerate(self.shards):
            dev = s.ids.device
            with torch.cuda.device(dev):
                sc, rows, rank, _ = call(on(q, dev), s.emb, k, normalize_q=normalize_q, target_rows=trows[i],
                                         slab_rows=slab_rows,
                                         exclude_rows=None if exclude_ids is None else s.rows_of(exclude_ids).contiguous(),
                                         tags=s.tags if tag_filter is not None else None, tag_filter=on(tag_filter, dev),
                                         after_scores=on(after_scores, dev),
                                         after_rows=None if after_ids is None else s.cursor_rows(after_ids).contiguous(),
                                         deep=k > K.RETRIEVE_MAX_K, bias=s.bias if use_bias else None,
                                         bias_weight=on(bias_weight, dev) if use_bias else None,
                                         target_scores=on(tscore, dev))
                ids = s._ids_of(rows)
            ls.append(sc.to(home))
            li.append(ids.to(home))
            if rank is not None:
                lr.append(rank.to(home))
        # 4: the lists of every rank, each rank's padded with empty lists to the longest
        for _ in range(self._pad_to - len(self.shards)):
            ls.append(torch.full_like(ls[0], float("-inf")))
            li.append(torch.zeros_like(li[0]))
            if lr:
                lr.append(torch.zeros_like(lr[0]))
        scores, ids = torch.stack(ls), torch.stack(li)
        ranks = torch.stack(lr) if lr else None
        if self.group is not None:
            scores = all_gather_stack(scores, self.group).flatten(0, 1)
            ids = all_gather_stack(ids, self.group).flatten(0, 1)
            if ranks is not None:
                ranks = all_gather_stack(ranks, self.group).flatten(0, 1)
        # 5
        with torch.cuda.device(home):
            out_scores, out_ids, out_rank = K.retrieve_merge_shards(scores.contiguous(), ids.contiguous(),
                                                                    None if ranks is None else ranks.contiguous())
        return out_ids, out_scores, out_rank, tscore_out

    def topk(self, q: torch.Tensor, k: int, *, normalize_q: bool = True, target_ids: Optional[torch.Tensor] = None,
             slab_rows: int = 0, exclude_ids: Optional[torch.Tensor] = None,
             tag_filter: Optional[torch.Tensor] = None, after_scores: Optional[torch.Tensor] = None,
             after_ids: Optional[torch.Tensor] = None,
             bias_weight: Union[None, float, torch.Tensor] = None):
        """``ItemCatalogue.topk`` over the union of the shards, argument for argument: (item_ids int64
        [Q, k], scores f32 [Q, k], rank, target_score), bit for bit what one ``ItemCatalogue`` holding
        every item returns, but for ``rank``, which is int64 here.  ``slab_rows`` goes to every shard's
        scan.  The outputs are on ``q``'s device."""
        return self._scan(q, k, normalize_q, target_ids, slab_rows, exclude_ids, tag_filter, after_scores, after_ids,
                          bias_weight, True)

    retrieve_takes = frozenset({"heads", *_TAGS, "after", "bias_weight"})
    _check_retrieve = ItemCatalogue._check_retrieve
    _retrieve = ItemCatalogue._retrieve

    def target_ranks(self, q: torch.Tensor, target_ids: torch.Tensor, *, exclude_ids: Optional[torch.Tensor] = None,
                     tag_filter: Optional[torch.Tensor] = None, bias_weight: Optional[float] = None) -> torch.Tensor:
        """``ItemCatalogue.target_ranks`` over the union of the shards (int64)."""
        return self._scan(q, 1, True, target_ids, 0, exclude_ids, tag_filter, None, None, bias_weight,
                          bias_weight is not None)[2]


class ShardedClusteredItemCatalogue(_Catalogue):
    """One catalogue held as clustered shards: ``local_shards`` are ``ClusteredItemCatalogue``s of this
    process, all plain, all ``with_filters()`` views or all ``with_deep()`` views (on one device or on
    several; disjoint ids, checked here), and with ``group`` the catalogue also covers the shards of the
    group's other ranks.  Every shard has centroids and a number of lists of its own.  All shards agree on
    carrying tags and on carrying a bias; at most ``K.RETRIEVE_MAX_SHARDS`` = 64 shards in all.

    ``nprobe`` is per shard: every shard probes its own min(``nprobe``, ``shard.nlist``) nearest lists for
    every query, so a query scans up to ``nprobe`` lists in each shard.

    Contract of ``topk``: with every list of every shard probed (``nprobe`` >= every ``nlist``) the result is,
    ids and score bits, what one ``ItemCatalogue`` over all items returns for the same arguments (for plain
    shards: a catalogue without a bias, as for the plain ``ClusteredItemCatalogue``).  With fewer lists
    probed it is the exact top-k of the union of the probed rows, in the flat scan's total order (score
    descending, id ascending) with the flat scan's score bits.

    The local shards of one device go through ``K.retrieve_ivf_topk_shards``: one plan, one scan launch and
    one merge for all of them (as many calls as keep the shards' probe slots within 64 each).  With a
    ``group`` the constructor, ``topk``, ``filter_like``, ``holds`` and ``validate`` are collectives, as on
    ``ShardedItemCatalogue``: every rank merges its own shards, the ranks' lists are gathered and merged
    again, and every rank gets the full result.  ``target_ids`` give the target's score and its rank among
    the probed rows (``topk``, ``target_ranks``)."""

    _KINDS = {ClusteredItemCatalogue: 0, FilteredClusteredItemCatalogue: 1, DeepClusteredItemCatalogue: 2}

    def __init__(self, local_shards: Sequence[ClusteredItemCatalogue], group=None):
        shards = list(local_shards)
        if not shards or not all(type(s) in self._KINDS for s in shards):
            raise ValueError("ShardedClusteredItemCatalogue takes one or more ClusteredItemCatalogue shards, or "
                             "their with_filters() / with_deep() views")
        if len({type(s) for s in shards}) != 1:
            raise ValueError("the shards of a clustered catalogue are of one kind: all plain, all with_filters() "
                             "or all with_deep()")
        if len({s.has_tags for s in shards}) != 1:
            raise ValueError("the shards of a catalogue all carry tags, or none does")
        if len({s.has_bias for s in shards}) != 1:
            raise ValueError("the shards of a catalogue all carry a bias, or none does")
        dev = shards[0].emb.device
        ids = torch.sort(torch.cat([s._ids.to(dev) for s in shards]))[0]
        if ids.numel() > 1 and bool((ids[1:] == ids[:-1]).any()):
            bad = int(ids[1:][ids[1:] == ids[:-1]][0])
            raise ValueError(f"the shards of a catalogue hold disjoint ids (id {bad} is in two of them)")
        self.shards = shards
        self.group = group
        self.device = dev
        self._kind = self._KINDS[type(shards[0])]
        self._total = int(ids.numel())
        self._max_items = self._total
        self._flat = None
        n_all = len(shards)
        if group is not None:
            mine = torch.tensor([len(shards), self._total, int(shards[0].has_tags), int(shards[0].has_bias), self._kind],
                                dtype=torch.int64, device=dev)
            every = all_gather_stack(mine, group).cpu()
            if bool((every[:, 2] != every[0, 2]).any()) or bool((every[:, 3] != every[0, 3]).any()):
                raise ValueError("the shards of a catalogue all carry tags / a bias, or none does (the ranks disagree)")
            if bool((every[:, 4] != every[0, 4]).any()):
                raise ValueError("the shards of a clustered catalogue are of one kind (the ranks disagree)")
            self._total = int(every[:, 1].sum())
            self._max_items = int(every[:, 1].max())
            n_all = int(every[:, 0].max()) * every.shape[0]
        if n_all > K.RETRIEVE_MAX_SHARDS:
            raise ValueError(f"a sharded catalogue takes at most {K.RETRIEVE_MAX_SHARDS} shards (got {n_all})")

    def __len__(self) -> int:
        return self._total

    @property
    def has_tags(self) -> bool:
        return self.shards[0].has_tags

    @property
    def has_bias(self) -> bool:
        return self.shards[0].has_bias

    @property
    def scans_filters(self) -> bool:
        return self._kind >= 1

    @property
    def scans_deep(self) -> bool:
        return self._kind == 2

    @property
    def max_k(self) -> int:
        return K.RETRIEVE_MAX_DEEP if self.scans_deep else K.RETRIEVE_MAX_K

    def update(self, *args, **kwargs):
        """Refused: an id belongs to one shard, and only the caller knows which."""
        _no_update("a ShardedClusteredItemCatalogue",
                   "update the shards (ClusteredItemCatalogue.update) and construct the sharded catalogue again")

    def validate(self) -> None:
        """Disjointness of the ids across the ranks of the group, as ``ShardedItemCatalogue.validate``."""
        dev = self.device
        ids = torch.cat([s._ids.to(dev) for s in self.shards])
        if self.group is not None:
            pad = torch.zeros(self._max_items, dtype=torch.int64, device=dev)
            pad[:ids.numel()] = ids
            ids = all_gather_stack(pad, self.group).reshape(-1)
            ids = ids[ids != 0]
        ids = torch.sort(ids)[0]
        if ids.numel() > 1 and bool((ids[1:] == ids[:-1]).any()):
            bad = int(ids[1:][ids[1:] == ids[:-1]][0])
            raise ValueError(f"the shards of a catalogue hold disjoint ids (id {bad} is in two of them)")

    _reduce_max = ShardedItemCatalogue._reduce_max
    holds = ShardedItemCatalogue.holds
    filter_like = ShardedItemCatalogue.filter_like

    def to_flat(self) -> ItemCatalogue:
        """The id-sorted ``ItemCatalogue`` over the items of all shards, with their tags and bias; for a
        catalogue without a group."""
        if self.group is not None:
            raise ValueError("to_flat takes a catalogue without a group: the other ranks' items are not here")
        dev = self.device
        flats = [s.to_flat() for s in self.shards]
        cat = lambda name: None if getattr(flats[0], name) is None else torch.cat([getattr(f, name).to(dev) for f in flats])
        return ItemCatalogue.from_embeddings(cat("ids"), cat("emb"), cat("tags"), cat("bias"))

    def _check_call(self, k: int, nprobe) -> Tuple[int, int]:
        return _check_probe_call(k, nprobe, self.max_k)  # nprobe is per shard, which probes min(nprobe, its nlist)

    def _chunks(self, nprobe: int):
        """The local shards cut into the calls of ``K.retrieve_ivf_topk_shards``: consecutive shards of one
        device whose probe slots, min(nprobe, nlist) each, number at most ``K.RETRIEVE_MAX_PROBE`` together."""
        out, cur, slots = [], [], 0
        for s in self.shards:
            p = min(nprobe, s.nlist)
            if cur and (cur[0].emb.device != s.emb.device or slots + p > K.RETRIEVE_MAX_PROBE):
                out.append(cur)
                cur, slots = [], 0
            cur.append(s)
            slots += p
        out.append(cur)
        return out

    def _scan(self, q, k, nprobe, normalize_q, target_ids, exclude_ids, tag_filter, after_scores, after_ids,
              bias_weight, use_bias):
        k, nprobe = self._check_call(k, nprobe)
        if not self.scans_filters:
            given = {"tag_filter": tag_filter, "after_scores": after_scores, "after_ids": after_ids,
                     "bias_weight": bias_weight}
            bad = [name for name, v in given.items() if v is not None]
            if bad:
                raise ValueError(f"retrieve with a clustered catalogue does not take {', '.join(bad)}: "
                                 "use catalogue.to_flat() for it")
            if q.dim() != 2:
                raise ValueError(f"a clustered catalogue takes [Q, {WIDTH}] queries, one per row (got {tuple(q.shape)})")
        else:
            self.shards[0]._check_filters(q, tag_filter, after_scores, after_ids, bias_weight)
        _check_exclude(exclude_ids)
        if target_ids is not None and (target_ids.dtype != torch.int64 or tuple(target_ids.shape) != (q.shape[0],)):
            raise ValueError(f"target_ids must be int64 [Q] (got {target_ids.dtype} {tuple(target_ids.shape)})")
        home = q.device
        use_bias = use_bias and self.scans_filters and self.has_bias
        if isinstance(bias_weight, (int, float)) and not isinstance(bias_weight, bool):
            bias_weight = torch.full((q.shape[0],), float(bias_weight), dtype=torch.float32, device=home)
        on = lambda t, dev: None if t is None else t.to(dev).contiguous()
        tscore = tscore_out = None
        if target_ids is not None:
            tscore, tscore_out, _ = _sharded_target_score(self.shards, q, target_ids, normalize_q, bias_weight, use_bias,
                                                          self._reduce_max)
        ls, li, lr = [], [], []
        for chunk in self._chunks(nprobe):
            dev = chunk[0].emb.device
            tup = [(s.emb, s.row_ids, s.list_off, s.centroids, s.tags, s.bias) for s in chunk]
            rows = lambda ids: None if ids is None else torch.stack([s.rows_of(ids) for s in chunk]).to(dev).contiguous()
            with torch.cuda.device(dev):
                sc, ids, rk = K.retrieve_ivf_topk_shards(on(q, dev), tup, nprobe, k, normalize_q=normalize_q,
                                                         exclude_rows=rows(exclude_ids), tag_filter=on(tag_filter, dev),
                                                         use_bias=use_bias,
                                                         bias_weight=on(bias_weight, dev) if use_bias else None,
                                                         after_scores=on(after_scores, dev), after_ids=on(after_ids, dev),
                                                         target_rows=rows(target_ids), target_scores=on(tscore, dev))
            ls.append(sc.to(home))
            li.append(ids.to(home))
            if rk is not None:
                lr.append(rk.to(home))
        scores, ids = torch.stack(ls), torch.stack(li)
        rank = torch.stack(lr).sum(dim=0) if lr else None
        if self.group is not None:
            if scores.shape[0] > 1:  # one list per rank goes through the gather
                with torch.cuda.device(home):
                    sc, idm, _ = K.retrieve_merge_shards(scores.contiguous(), ids.contiguous())
                scores, ids = sc[None], idm[None]
            scores = all_gather_stack(scores[0].contiguous(), self.group)
            ids = all_gather_stack(ids[0].contiguous(), self.group)
            if rank is not None:
                rank = all_gather_stack(rank.contiguous(), self.group).sum(dim=0)
        if rank is not None:
            rank = torch.where(torch.isnan(tscore), torch.full_like(rank, -1), rank)
        if scores.shape[0] == 1:
            return ids[0], scores[0], rank, tscore_out
        with torch.cuda.device(home):
            out_scores, out_ids, _ = K.retrieve_merge_shards(scores.contiguous(), ids.contiguous())
        return out_ids, out_scores, rank, tscore_out

    def topk(self, q: torch.Tensor, k: int, *, nprobe: int, normalize_q: bool = True,
             target_ids: Optional[torch.Tensor] = None, exclude_ids: Optional[torch.Tensor] = None,
             tag_filter: Optional[torch.Tensor] = None, after_scores: Optional[torch.Tensor] = None,
             after_ids: Optional[torch.Tensor] = None, bias_weight: Union[None, float, torch.Tensor] = None):
        """(item_ids int64 [Q, k], scores f32 [Q, k], rank, target_score), the order of
        ``ShardedItemCatalogue.topk``: per query the k first, under (score descending, id ascending), of the
        items that lie in the min(``nprobe``, nlist) nearest lists of any shard (``nprobe`` is per shard), are
        not among its ``exclude_ids``, pass its ``tag_filter`` and lie strictly behind (``after_scores``,
        ``after_ids``), then (0, -inf).  ``tag_filter``, the cursor and ``bias_weight`` need ``with_filters()`` or
        ``with_deep()`` shards, which also score with the shards' bias where they carry one; k reaches 128, on
        ``with_deep()`` shards 1,024.  See the class for the contract against the flat catalogue.
        With ``target_ids`` int64 [Q], ``target_score`` is the target's score from the shard that holds it
        (-inf where none does), whether or not its list is probed, and ``rank`` (int64) the number of eligible
        items of the probed lists, other than the target, that score strictly above it, -1 where no shard
        holds the target: with every list probed the flat catalogue's rank, with fewer a lower bound of it.
        Else both are None.  The outputs are on ``q``'s device."""
        return self._scan(q, k, nprobe, normalize_q, target_ids, exclude_ids, tag_filter, after_scores, after_ids,
                          bias_weight, True)

    _REFUSAL = ClusteredItemCatalogue._REFUSAL
    _RANKS_TAKE_NPROBE = True

    @property
    def retrieve_takes(self) -> frozenset:
        """What a clustered catalogue of the shards' kind takes, but ``heads`` and what diversifies a list."""
        return self.shards[0].retrieve_takes - {"heads", "diversity", "pool", "group_cap"}

    def _check_retrieve(self, k, given: dict) -> None:
        if given["heads"] is not None:
            raise ValueError("retrieve with a sharded clustered catalogue does not take heads: several queries "
                             "per user over clustered shards are not supported (use catalogue.to_flat() for it)")
        _refuse_named(self, given, ("diversity", "pool", "group_cap", *_TAGS, "after", "bias_weight"))
        _need_nprobe(given)
        self._check_call(k, given["nprobe"])
        _refuse_shortlist(given)

    def _retrieve(self, q, k, nprobe, shortlist, exclude_ids, tag_filter, after_scores, after_ids, bias_weight):
        return self.topk(q, k, nprobe=nprobe, normalize_q=True, exclude_ids=exclude_ids, tag_filter=tag_filter,
                         after_scores=after_scores, after_ids=after_ids, bias_weight=bias_weight)[:2]

    def target_ranks(self, q: torch.Tensor, target_ids: torch.Tensor, *, nprobe: int,
                     exclude_ids: Optional[torch.Tensor] = None, tag_filter: Optional[torch.Tensor] = None,
                     bias_weight: Optional[float] = None) -> torch.Tensor:
        """``ItemCatalogue.target_ranks`` over the probed lists (int64): ``topk``'s ``rank`` at k = 1, on the
        plain dots unless ``bias_weight`` is given."""
        return self._scan(q, 1, nprobe, True, target_ids, exclude_ids, tag_filter, None, None, bias_weight,
                          bias_weight is not None)[2]

    def recall(self, q: torch.Tensor, k: int, nprobe: int, **filters) -> float:
        """The mean over the queries of the fraction of the flat union's list, ``to_flat().topk(q, k,
        **filters)`` (for plain shards on the plain dots), that ``topk(q, k, nprobe=nprobe, **filters)``
        returns, over the queries whose flat list is not empty (1.0 where every one is).  Never decreases
        in ``nprobe``; 1.0 once every list of every shard is probed.  For a catalogue without a group."""
        if self._flat is None:
            flat = self.to_flat()
            self._flat = flat if self.scans_filters else ItemCatalogue(flat.ids, flat.emb, flat.tags)
        return _hit_fraction(self._flat.topk(q, k, **filters)[0], self.topk(q, k, nprobe=nprobe, **filters)[0], k)


def shard_bounds(n: int, rank: int, world: int) -> Tuple[int, int]:
    """The slice [lo, hi) of n sorted ids that ``build_catalogue(shard=(rank, world))`` keeps."""
    return rank * n // world, (rank + 1) * n // world


@torch.no_grad()
def build_catalogue(wrapper, ids: torch.Tensor, chunk: int = 65536, tags: Optional[torch.Tensor] = None,
                    bias: Optional[torch.Tensor] = None, shard: Optional[Tuple[int, int]] = None,
                    groups: Optional[torch.Tensor] = None) -> ItemCatalogue:
    """The catalogue of ``ids`` under ``wrapper``'s current weights: per chunk, the item
    embedding module and the product tower on a [1, n] id row (the training kernels), then
    F.normalize to bf16 as the loss does (``K.rownorm``).  A row therefore equals the
    normalised ``current_token_emb`` row a forward produces for that id.  ``tags`` (int32, one
    word per entry of ``ids``) follow the ids through the sort and the de-duplication; an id given
    twice with different tags is refused.  ``bias`` (f32, one word per entry of ``ids``) follows
    them the same way, under the same rule, and so do ``groups`` (int32, one key per entry of ``ids``,
    0 = no group: ``ItemCatalogue.diversify``'s ``group_cap``).

    ``shard = (rank, world)``: this process's part of a catalogue built by ``world`` processes, for a
    ``ShardedItemCatalogue``.  Every rank passes the same ``ids`` (and ``tags`` / ``bias`` / ``groups``) and keeps
    the slice [rank n // world, (rank + 1) n // world) of the n sorted unique ids.  Every rank makes
    the same number of chunk calls, since the forward of a row-sharded item table is a collective: a
    rank whose slice has ended joins the remaining calls with a one-id row whose result it drops.
    A row-sharded item table at world size > 1 needs ``shard``."""
    from ....commons.layers import RowShardedKShiftEmbedding
    enc = wrapper._model
    if shard is None and isinstance(enc.product_emb_module, RowShardedKShiftEmbedding) and world_size() > 1:
        raise RuntimeError("build_catalogue does not take a row-sharded item table at world size > 1 "
                           "without shard=(rank, world): every rank then builds its own slice of the catalogue")
    if shard is not None:
        if len(shard) != 2 or not 0 <= int(shard[0]) < int(shard[1]):
            raise ValueError(f"shard takes (rank, world) with 0 <= rank < world (got {shard})")
    if ids.dtype != torch.int64 or ids.dim() != 1 or ids.numel() < 1:
        raise ValueError("build_catalogue takes int64 ids [N], N >= 1")
    if chunk < 1:
        raise ValueError("chunk must be positive")
    dev = next(wrapper.parameters()).device
    if tags is not None:
        if tags.dtype != torch.int32 or tags.shape != ids.shape:
            raise ValueError(f"build_catalogue takes int32 tags, one per id (got {tags.dtype} {tuple(tags.shape)})")
        tags = unique_tags(ids.to(dev), tags.to(dev))
    if bias is not None:
        if bias.dtype != torch.float32 or bias.shape != ids.shape:
            raise ValueError(f"build_catalogue takes f32 bias, one per id (got {bias.dtype} {tuple(bias.shape)})")
        bias = unique_bias(ids.to(dev), bias.to(dev))
    if groups is not None:
        if groups.dtype != torch.int32 or groups.shape != ids.shape:
            raise ValueError(f"build_catalogue takes int32 groups, one per id (got {groups.dtype} {tuple(groups.shape)})")
        groups = unique_groups(ids.to(dev), groups.to(dev))
    ids = torch.unique(ids.to(dev))  # sorted ascending
    if bool((ids == 0).any()):
        raise ValueError("catalogue ids must not hold 0, the pad id")
    calls = (ids.numel() + chunk - 1) // chunk
    if shard is not None:
        n, (r, w) = ids.numel(), (int(shard[0]), int(shard[1]))
        if w > n:
            raise ValueError(f"build_catalogue: {w} shards of {n} ids: a shard is never empty")
        lo, hi = shard_bounds(n, r, w)
        spare = ids[:1]  # the row of a call this rank only joins
        ids = ids[lo:hi]
        tags = None if tags is None else tags[lo:hi].contiguous()
        bias = None if bias is None else bias[lo:hi].contiguous()
        groups = None if groups is None else groups[lo:hi].contiguous()
        calls = ((n + w - 1) // w + chunk - 1) // chunk  # those of the longest slice, on every rank
    out = torch.empty((ids.numel(), WIDTH), dtype=torch.bfloat16, device=dev)
    for i in range(calls):
        lo = i * chunk
        row = (ids[lo:lo + chunk] if lo < ids.numel() else spare).view(1, -1).contiguous()
        _, prod, _ = enc.product_tower(row, enc.product_emb_module(row))
        if lo < ids.numel():
            out[lo:lo + row.numel()] = K.rownorm(prod.reshape(-1, WIDTH).contiguous())[0]
    return ItemCatalogue(ids.contiguous(), out, tags, bias, groups)


def unique_tags(ids: torch.Tensor, tags: torch.Tensor) -> torch.Tensor:
    """The tags of ``torch.unique(ids)``, row for row: ``tags[i]`` belongs to ``ids[i]``, and an
    id that occurs more than once must carry one tag word."""
    uniq, inv = torch.unique(ids, return_inverse=True)  # sorted ascending, as build_catalogue sorts
    out = torch.empty(uniq.numel(), dtype=tags.dtype, device=tags.device)
    out[inv] = tags  # of duplicates any one occurrence lands; the check below makes them equal
    if not bool((out[inv] == tags).all()):
        bad = ids[out[inv] != tags][0].item()
        raise ValueError(f"build_catalogue: id {bad} is given more than once with different tags")
    return out


def unique_groups(ids: torch.Tensor, groups: torch.Tensor) -> torch.Tensor:
    """The group keys of ``torch.unique(ids)``, row for row, as ``unique_tags`` does for tags: an id
    that occurs more than once must carry one key."""
    uniq, inv = torch.unique(ids, return_inverse=True)
    out = torch.empty(uniq.numel(), dtype=groups.dtype, device=groups.device)
    out[inv] = groups
    if not bool((out[inv] == groups).all()):
        bad = ids[out[inv] != groups][0].item()
        raise ValueError(f"build_catalogue: id {bad} is given more than once with different groups")
    return out


def unique_bias(ids: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """The bias of ``torch.unique(ids)``, row for row, as ``unique_tags`` does for tags: an id that
    occurs more than once must carry one bias (compared as bits, so -0 and +0 differ and a NaN is
    left for ``ItemCatalogue`` to refuse)."""
    uniq, inv = torch.unique(ids, return_inverse=True)
    out = torch.empty(uniq.numel(), dtype=bias.dtype, device=bias.device)
    out[inv] = bias
    same = out[inv].view(torch.int32) == bias.view(torch.int32)
    if not bool(same.all()):
        bad = ids[~same][0].item()
        raise ValueError(f"build_catalogue: id {bad} is given more than once with different biases")
    return out
