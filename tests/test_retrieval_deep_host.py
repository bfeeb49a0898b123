"""CPU checks of the single-scan deep list's host layer: lthm_retrieve_deep_ws_bytes, the two new
prototypes, the unchanged `deep` defaults of the Python calls and the schema of the scripted op.
No kernel is launched."""
import ctypes
import inspect

import pytest
import torch

from recommendations_amd import _lib
from recommendations_amd import kernels as K

U, N = 70, 3000


def test_symbols():
    lib = _lib.load()
    protos = _lib.parse_header()
    assert protos["lthm_retrieve_deep_ws_bytes"] == ("int64_t", ["int64_t", "int32_t", "int64_t", "int32_t", "int32_t",
                                                                "int64_t"])
    assert protos["lthm_retrieve_topk_deep"] == protos["lthm_retrieve_topk_bias"]
    assert hasattr(lib, "lthm_retrieve_topk_deep") and hasattr(lib, "lthm_retrieve_deep_ws_bytes")
    assert lib.lthm_abi_version() == 44  # additive
    assert ctypes.sizeof(_lib.STRUCTS["lthm_retrieve_desc"]) == 104


@pytest.mark.parametrize("G,X,slab_rows", [(1, 0, 0), (1, 5, 64), (3, 0, 128), (8, 1024, 0)])
def test_ws_bytes_up_to_128_is_the_group_calls(G, X, slab_rows):
    lib = _lib.load()
    for k in (1, 100, 128):
        want = lib.lthm_retrieve_group_ws_bytes(U, G, N, k, slab_rows, X)
        assert want > 0 and lib.lthm_retrieve_deep_ws_bytes(U, G, N, k, slab_rows, X) == want


@pytest.mark.parametrize("G,X,slab_rows", [(1, 0, 0), (1, 5, 64), (3, 0, 128), (8, 1024, 0), (1, 0, 1024), (2, 7, 4096)])
def test_ws_bytes_deep(G, X, slab_rows):
    lib = _lib.load()
    got = [lib.lthm_retrieve_deep_ws_bytes(U, G, N, k, slab_rows, X) for k in (129, 1000, 1024)]
    assert all(b > 0 for b in got) and got == sorted(got)
    # at least the k keys of every (slab, user) that the merge reads
    sr = slab_rows or N
    nslab = -(-N // sr)
    assert got[2] >= nslab * U * 1024 * 8


def test_ws_bytes_refusals():
    lib = _lib.load()
    f = lib.lthm_retrieve_deep_ws_bytes
    assert f(U, 1, N, 300, 0, 0) > 0
    for k in (0, 1025, -1):
        assert f(U, 1, N, k, 0, 0) == -1
    for sr in (1, 63, 65, 100, -64):
        assert f(U, 1, N, 300, sr, 0) == -1
    for X in (-1, 1025):
        assert f(U, 1, N, 300, 0, X) == -1
    for G in (0, 9, -1):
        assert f(U, G, N, 300, 0, 0) == -1
    for u, n in ((0, N), (U, 0), (1 << 31, N), (U, 1 << 31)):
        assert f(u, 1, n, 300, 0, 0) == -1
    # the entries for k <= 128 keep refusing a deep k
    assert lib.lthm_retrieve_ws_bytes(U, N, 129, 0) == -1
    assert lib.lthm_retrieve_group_ws_bytes(U, 3, N, 129, 0, 0) == -1


def test_python_signatures_unchanged():
    for fn in (K.retrieve_topk, K.retrieve_topk_group):
        p = inspect.signature(fn).parameters["deep"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert K.RETRIEVE_MAX_DEEP == 1024 and K.RETRIEVE_MAX_K == 128
    assert K.retrieve_deep_passes(1024) == [128] * 8 and K.retrieve_deep_passes(129) == [128, 1]
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    assert "deep" not in inspect.signature(ItemCatalogue.topk).parameters
    assert "deep" not in inspect.signature(LTHMModelWrapper.retrieve).parameters


def test_op_schema():
    _lib.load_torch_ops()
    assert (str(torch.ops.lthm.retrieve_topk_deep.default._schema)
            == "lthm::retrieve_topk_deep(Tensor q, Tensor items, int k, bool normalize_q, Tensor? exclude_rows, "
               "Tensor? tags, Tensor? tag_filter, Tensor? after_scores, Tensor? after_rows, Tensor? bias, "
               "Tensor? bias_weight=None) -> (Tensor scores, Tensor rows)")


def test_abi_refuses_before_any_launch():
    """k = 1025, a short workspace and a misaligned cursor pointer: the error code, on the host."""
    lib = _lib.load()
    d = _lib.STRUCTS["lthm_retrieve_desc"]()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    d.items = d.q = d.scores = d.rows = d.workspace = base
    d.Q, d.N, d.q_dtype, d.normalize_q, d.slab_rows = 1, 1, _lib.F32, 0, 0
    call = lambda c=None: lib.lthm_retrieve_topk_deep(ctypes.addressof(d), None, None, None,
                                                      ctypes.addressof(c) if c is not None else None, None, None)
    d.k, d.ws_bytes = 1025, 1 << 30
    assert call() != 0
    d.k = 300
    d.ws_bytes = lib.lthm_retrieve_deep_ws_bytes(1, 1, 1, 300, 0, 0) - 1
    assert d.ws_bytes > 0 and call() != 0
    d.ws_bytes = 1 << 30
    c = _lib.STRUCTS["lthm_retrieve_cursor"]()
    for cs, cr in ((base + 2, base), (base, base + 1), (0, base), (base, 0)):
        c.after_score, c.after_row = cs or None, cr or None
        assert call(c) != 0
