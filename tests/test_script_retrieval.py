"""torch.ops.lthm.retrieve_topk (csrc/torch_ops/lthm_ops.cpp): a scripted serving module
compiles on the CPU and, on the GPU, returns what K.retrieve_topk returns."""
from typing import Tuple

import pytest
import torch
import torch.nn as nn

from recommendations_amd import _lib


class Serve(nn.Module):
    def forward(self, q: torch.Tensor, items: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        scores, rows = torch.ops.lthm.retrieve_topk(q, items, 7, True)
        return scores, rows


def test_scripts_on_cpu():
    _lib.load_torch_ops()
    assert (str(torch.ops.lthm.retrieve_topk.default._schema)
            == "lthm::retrieve_topk(Tensor q, Tensor items, int k, bool normalize_q) -> (Tensor scores, Tensor rows)")
    sm = torch.jit.script(Serve())
    assert "lthm::retrieve_topk" in str(sm.graph)
    with pytest.raises(RuntimeError):  # no CPU kernel: the dispatcher refuses
        sm(torch.zeros(2, 128), torch.zeros(9, 128, dtype=torch.bfloat16))


@pytest.mark.gpu
def test_scripted_matches_eager(dev):
    from recommendations_amd import kernels as K
    _lib.load_torch_ops()
    g = torch.Generator().manual_seed(2)
    q = torch.randn(37, 128, generator=g).to(dev)
    items = torch.nn.functional.normalize(torch.randn(3001, 128, generator=g), dim=-1).to(torch.bfloat16).to(dev)
    scores, rows = torch.jit.script(Serve())(q, items)
    e_scores, e_rows, _, _ = K.retrieve_topk(q, items, 7, normalize_q=True)
    assert torch.equal(scores, e_scores) and torch.equal(rows, e_rows)
    with pytest.raises(RuntimeError):
        torch.ops.lthm.retrieve_topk(q, items, 129, True)
