"""Top-k of rows above 16384 scores (head_topk.hip's streaming radix select, up to 65536): value
descending, ties to the lower index, against numpy's lexsort as test_topk_radix_select_cases."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3


def _scores(kind, S, g):
    if kind == "uniform":
        return torch.rand(B, S, generator=g)
    if kind == "all_equal":                                    # the select runs into the index bits above 2^14
        return torch.full((B, S), 0.75)
    if kind == "five_values":
        return torch.randint(0, 5, (B, S), generator=g).float() * 0.25 - 0.5
    s = torch.randn(B, S, generator=g)                         # "neg_inf": both signs, every third -inf
    s[:, ::3] = -float("inf")
    return s


@pytest.mark.parametrize("kind", ["uniform", "all_equal", "five_values", "neg_inf"])
@pytest.mark.parametrize("S,K", [(16385, 64), (20000, 256), (65536, 256), (65536, 1), (40000, 1024)])
def test_topk_large_rows(cuda, S, K, kind):
    from dvcp import ops
    s = _scores(kind, S, torch.Generator().manual_seed(S + K))
    got = ops.topk(s.to(cuda), K).cpu().numpy()
    for b in range(B):
        want = np.lexsort((np.arange(S), -s[b].numpy()))[:K]
        assert np.array_equal(got[b], want), (kind, b)


def test_topk_limits_named(cuda):
    from dvcp import ops
    with pytest.raises(RuntimeError, match="exceeds 65536"):
        ops.topk(torch.zeros(1, 65537, device=cuda), 4)
    with pytest.raises(RuntimeError, match="1024.*16384"):
        ops.topk(torch.zeros(1, 20000, device=cuda), 1025)
    # at or below 16384 any K <= S still runs (the block-argmax kernel above 1024)
    s = torch.rand(1, 16384, generator=torch.Generator().manual_seed(1))
    got = ops.topk(s.to(cuda), 1100).cpu()
    assert torch.equal(got, torch.topk(s, 1100, dim=1).indices)
