"""torch_ref.moe_tile_map, the CPU contract of the tiled route's tile map, and
the static bound the host sizes the map by. Holds the route cases that
tests/test_gpu_moe_tiled.py runs on the kernels."""
import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.ops import torch_ref
from tests import moe_cases as mc

# (T, topk, E): P above one placement block, a block boundary inside a segment
ROUTE_CASES = ((65, 2, 8), (513, 2, 8), (1025, 8, 64), "one", "ends_empty")


def route_topi(kind):
    """-> (topi [T, topk] int32, E) of a route case."""
    if kind == "one":                       # every token on one expert
        return torch.full((130, 1), 3, dtype=torch.int32), 8
    if kind == "ends_empty":                # first and last expert empty
        return torch.randint(1, 7, (300, 2), generator=mc._gen("ends"),
                             dtype=torch.int32), 8
    T, topk, E = kind
    return torch.rand(T, E, generator=mc._gen("route", kind)).argsort(-1)[
        :, :topk].int(), E


def _check_map(seg, BM):
    """The tiles ascend in expert, start inside their segment at a multiple
    of BM, cover every sorted row once in order, and respect the bound."""
    te, tr, n = torch_ref.moe_tile_map(seg, BM)
    seg = seg.tolist()
    P, E = seg[-1], len(seg) - 1
    assert n == len(te) == len(tr) <= P // BM + min(E, P)
    assert n == sum(-(-(seg[e + 1] - seg[e]) // BM) for e in range(E))
    assert te.tolist() == sorted(te.tolist())
    rows = []
    for e, r in zip(te.tolist(), tr.tolist()):
        assert seg[e] <= r < seg[e + 1] and (r - seg[e]) % BM == 0
        rows += range(r, min(r + BM, seg[e + 1]))
    assert rows == list(range(P))


@pytest.mark.parametrize("BM", ops.MOE_TILE_BMS)
@pytest.mark.parametrize("kind", ROUTE_CASES, ids=str)
def test_tile_map_route_cases(kind, BM):
    topi, E = route_topi(kind)
    seg, pair, te, tr, n = ops.moe_route_tiled(topi, E, BM)
    assert torch.equal(pair.long(), torch.argsort(topi.flatten().long(),
                                                  stable=True))
    assert n <= topi.numel() // BM + min(E, topi.numel())
    _check_map(seg, BM)


@pytest.mark.parametrize("BM", ops.MOE_TILE_BMS)
@pytest.mark.parametrize("counts", [(70,), (0, 65, 0, 3), (31, 33, 1, 0, 64),
                                    (129, 0, 127), (1,) * 64, (0, 0, 4096)])
def test_tile_map_counts(counts, BM):
    _check_map(torch.tensor([0] + list(counts)).cumsum(0).int(), BM)


def test_cpu_route_and_switch():
    topi = torch.tensor([[1, 0], [1, 2], [0, 1]], dtype=torch.int32)
    seg, pair, te, tr, n = ops.moe_route_tiled(topi, 4, 32)
    assert seg.tolist() == [0, 2, 5, 6, 6] and pair.tolist() == [1, 4, 0, 2, 5, 3]
    assert (te.tolist(), tr.tolist(), n) == ([0, 1, 2], [0, 2, 5], 3)
    assert ops.moe_tiled_enabled() is False
    ops.set_moe_tiled(True)
    assert ops.moe_tiled_enabled() is True
    ops.set_moe_tiled(None)
    assert ops.moe_tile_config(28672, 4096, 128, 2, 8, "fp8")[0] == 32
    assert ops.moe_tile_config(4096, 14336, 2048, 2, 8, "mxfp4")[0] == 128
    assert ops.moe_tile_config(48, 384, 128, 2, 8, "mxfp4") is None
    assert ops.moe_tile_config(48, 512, 64, 2, 8, "fp8") is None
