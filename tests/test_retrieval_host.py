"""CPU checks of the retrieval host code: ItemCatalogue (models/lthm/sequence/retrieval.py)
and the workspace query of the C ABI.  No kernel is launched."""
import re

import pytest
import torch

from recommendations_amd import _lib
from recommendations_amd.models.lthm.sequence.retrieval import FORMAT, ItemCatalogue


def _emb(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(torch.bfloat16)


def test_catalogue_rejects_bad_input():
    emb = _emb(4)
    with pytest.raises(ValueError, match="pad id"):
        ItemCatalogue.from_embeddings(torch.tensor([3, 0, 5, 9]), emb)
    with pytest.raises(ValueError, match="duplicates"):
        ItemCatalogue.from_embeddings(torch.tensor([3, 7, 3, 9]), emb)
    with pytest.raises(ValueError, match="bf16"):
        ItemCatalogue.from_embeddings(torch.tensor([1, 2, 3, 4]), emb[:, :64].contiguous())
    with pytest.raises(ValueError, match="bf16"):
        ItemCatalogue.from_embeddings(torch.tensor([1, 2, 3, 4]), emb.float())
    with pytest.raises(ValueError):
        ItemCatalogue.from_embeddings(torch.tensor([1, 2, 3]), emb)
    with pytest.raises(ValueError, match="int64"):
        ItemCatalogue.from_embeddings(torch.tensor([1, 2, 3, 4], dtype=torch.int32), emb)
    with pytest.raises(ValueError, match="ascending"):
        ItemCatalogue(torch.tensor([4, 3, 2, 1]), emb)  # the plain constructor does not sort


def test_catalogue_sorts_consistently():
    ids = torch.tensor([50, -7, 2 ** 40, 3, -(2 ** 62), 11])
    emb = _emb(6)
    cat = ItemCatalogue.from_embeddings(ids, emb)
    assert cat.ids.tolist() == sorted(ids.tolist())
    for i, v in enumerate(ids.tolist()):  # every id kept its own vector
        assert torch.equal(cat.emb[cat.ids.tolist().index(v)], emb[i])
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    again = ItemCatalogue.from_embeddings(ids[perm], emb[perm])
    assert torch.equal(again.ids, cat.ids) and torch.equal(again.emb, cat.emb)


def test_rows_of():
    cat = ItemCatalogue.from_embeddings(torch.tensor([50, -7, 3, 11]), _emb(4))
    rows = cat.rows_of(torch.tensor([[3, 4, 50], [0, -7, 2 ** 62], [11, -8, -(2 ** 63)]]))
    assert rows.dtype == torch.int32
    assert rows.tolist() == [[1, -1, 3], [-1, 0, -1], [2, -1, -1]]


def test_save_load_round_trip(tmp_path):
    cat = ItemCatalogue.from_embeddings(torch.tensor([9, 4, 2 ** 50, -3]), _emb(4, seed=3))
    path = str(tmp_path / "cat.safetensors")
    cat.save(path)
    back = ItemCatalogue.load(path)
    assert torch.equal(back.ids, cat.ids)
    assert back.emb.dtype == torch.bfloat16 and torch.equal(back.emb.view(torch.int16), cat.emb.view(torch.int16))
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        assert f.metadata()["format"] == FORMAT


def test_load_refuses_other_formats(tmp_path):
    from safetensors.torch import save_file
    path = str(tmp_path / "other.safetensors")
    save_file({"ids": torch.tensor([1, 2]), "emb": _emb(2)}, path, metadata={"format": "lthm-item-artifact-v1"})
    with pytest.raises(ValueError, match="not an item catalogue"):
        ItemCatalogue.load(path)
    save_file({"ids": torch.tensor([1, 2]), "emb": _emb(2)}, path)
    with pytest.raises(ValueError, match="not an item catalogue"):
        ItemCatalogue.load(path)


def test_ws_bytes():
    ws = _lib.load().lthm_retrieve_ws_bytes
    assert ws(256, 2_000_000, 100, 0) > 0
    for Q, N, k, sr in [(0, 100, 10, 0), (-1, 100, 10, 0), (4, 0, 10, 0), (4, -5, 10, 0), (4, 2 ** 31, 10, 0),
                        (4, 100, 0, 0), (4, 100, 129, 0), (4, 100, 10, 63), (4, 100, 10, 100), (4, 100, 10, -64),
                        (4, 64 * 65536, 10, 64)]:
        assert ws(Q, N, k, sr) == -1, (Q, N, k, sr)
    assert ws(4, 2 ** 31 - 1, 128, 0) > 0
    # monotone in Q (fixed slabs) and in the slab count (fixed Q)
    by_q = [ws(Q, 100_000, 100, 1024) for Q in (1, 2, 63, 64, 65, 1000, 4096)]
    assert by_q == sorted(by_q) and len(set(by_q)) == len(by_q)
    by_slabs = [ws(64, 100_000, 100, sr) for sr in (65536, 8192, 1024, 128, 64)]
    assert by_slabs == sorted(by_slabs) and len(set(by_slabs)) == len(by_slabs)


def test_abi_version_is_44():
    with open(_lib.HEADER) as f:
        assert int(re.search(r"#define\s+LTHM_ABI_VERSION\s+(\d+)", f.read()).group(1)) == 44
    assert _lib.load().lthm_abi_version() == 44
    assert "lthm_retrieve_desc" in _lib.STRUCTS
