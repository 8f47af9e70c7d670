"""tests/sampler_cases.py on the CPU: every case is unambiguous under the
float64 reference alone, and `torch_ref.topkp_keep_mask` is the keep set of
the CPU engine path (`engine/sampling.py::_filter_topk_topp`) on every case,
so the two are one definition. The filter is run on float64 logits there: the
engine feeds it fp32, whose cumulative sum over V terms is not what the
margins of the cases are about, so the engine's fp32 path itself is not what
is compared (no case has a tie across the nucleus boundary, where the two
would differ in any precision). The HIP kernel is held to the same cases in
tests/test_gpu_sampler_filters.py."""
import pytest
import torch

from dynamo_amd.engine.sampling import _filter_topk_topp
from dynamo_amd.ops import torch_ref
from tests import sampler_cases as sc

ALL_V = sc.VOCABS + (sc.BIG_V,)


def _rows(V, groups):
    for g in groups(V):
        for b in range(g.B):
            yield g, b, int(g.top_k[b]), float(g.top_p[b])


def test_keep_mask_small_examples():
    x = torch.tensor([[0.0, 2.0, 1.0, 2.0, float("-inf"), -1.0]])
    keep = lambda k, p: torch_ref.topkp_keep_mask(x, k, p)[0].tolist()
    assert keep(0, 1.0) == [True, True, True, True, False, True]
    assert keep(6, 1.0) == keep(-1, 1.0) == keep(0, 1.0)
    assert keep(1, 1.0) == keep(2, 1.0) == [False, True, False, True,
                                            False, False]
    assert keep(3, 1.0) == [False, True, True, True, False, False]
    # softmax of (2, 2, 1, 0, -1): .387 .387 .142 .052 .019
    assert keep(0, 0.5) == keep(0, 0.0) == keep(0, -1.0) == keep(1, 1.0)
    assert keep(0, 0.8) == keep(3, 1.0)
    assert keep(0, 0.95) == [True, True, True, True, False, False]
    # after top-k = 3 the survivors are .422 .422 .155: 0.8 keeps only two
    assert keep(3, 0.8) == keep(1, 1.0)
    # per-row parameters; a row of -inf keeps everything
    y = torch.cat([x, x, torch.full_like(x, float("-inf"))])
    got = torch_ref.topkp_keep_mask(y, torch.tensor([3, 0, 2]),
                                    torch.tensor([1.0, 0.5, 0.3]))
    assert got[0].tolist() == keep(3, 1.0)
    assert got[1].tolist() == keep(0, 0.5)
    assert bool(got[2].all())


@pytest.mark.parametrize("V", ALL_V)
def test_cases_cover_the_grid(V):
    groups = sc.exact_groups(V)
    kinds = ("peaked",) if V == sc.BIG_V else sc.KIND_NAMES
    assert all(g.B <= sc.MAX_ROWS and g.V == V for g in groups)
    assert sum(g.B for g in groups) == len(kinds) * len(sc.param_list(V))
    seen = {(g.kinds[b], k) for g, b, k, _ in _rows(V, sc.exact_groups)}
    assert seen >= {(kind, k) for kind in kinds
                    for k in (-3, 0, 1, 5, 50, V - 1, V, V + 5)}
    crossed = {(g.kinds[b], k) for g, b, k, p in _rows(V, sc.exact_groups)
               if p < 1.0}
    assert crossed == {(kind, k) for kind in kinds for k in (0, 1, 5, 50)}
    if V != sc.BIG_V:
        assert any(sc.topk1_rows(g) for g in groups)
        argmax_at = {int(g.argmax[b]) for g, b, _, _ in
                     _rows(V, sc.exact_groups)}
        assert {0, V - 1} <= argmax_at
        few = [g.logits[b] for g, b, _, _ in _rows(V, sc.exact_groups)
               if g.kinds[b] == "masked_few"]
        assert all(int(torch.isfinite(r).sum()) == sc.FEW for r in few)
        masked = [g.logits[b] for g, b, _, _ in _rows(V, sc.exact_groups)
                  if g.kinds[b] == "masked"]
        assert all(int(torch.isinf(r).sum()) == int(0.7 * V) for r in masked)


@pytest.mark.parametrize("V", ALL_V)
def test_margins(V):
    for g, b, k, p in _rows(V, sc.exact_groups):
        row = g.logits[b]
        assert sc.k_boundary_ok(row, k), g.labels[b]
        if g.kinds[b] == "ties" and 0 < k < V:
            srt = row.sort(descending=True).values
            kt = sc.tie_rank(k, V)
            assert float(srt[kt - 1]) == float(srt[min(kt, V - 1)])
            assert float(srt[0]) > float(srt[1])
        if p >= 1.0:
            continue
        srt, prob, n = sc._sorted_probs(row, k)
        cum = prob.cumsum(-1)
        j = int((cum < p).sum())            # ranks 0 .. j are kept
        assert j < n, g.labels[b]
        assert float(cum[j]) - p >= sc.P_MARGIN, g.labels[b]
        assert p - float(cum[j] - prob[j]) >= sc.P_MARGIN, g.labels[b]
        assert j == n - 1 or float(srt[j]) != float(srt[j + 1]), g.labels[b]
        assert int(g.mask[b].sum()) == j + 1, g.labels[b]


@pytest.mark.parametrize("V", sc.VOCABS)
def test_crossed_cases_tell_the_filter_orders_apart(V):
    n = 0
    for g, b, k, p in _rows(V, sc.exact_groups):
        if k in (5, 50) and p < 1.0 and g.kinds[b] in sc.ORDER_KINDS:
            seq, both = sc.sequential_and_intersected(g.logits[b], k, p)
            assert torch.equal(seq, g.mask[b])
            assert bool((both & ~seq).any()) and not bool((seq & ~both).any())
            n += 1
    assert n == 2 * len(sc.ORDER_KINDS)


@pytest.mark.parametrize("V", ALL_V)
def test_reference_is_the_cpu_engine_filter(V):
    groups = sc.exact_groups(V)
    if V != sc.BIG_V:
        groups += sc.range_groups(V)
    for g in groups:
        for b in range(g.B):
            k, p = int(g.top_k[b]), float(g.top_p[b])
            if p == float(torch.tensor(0.999999)):
                continue        # a range case: no margin around this top_p
            # the filter is run in float64: the margins are about the HIP
            # kernel's error, not about a float32 cumsum over V terms
            kept = torch.isfinite(
                _filter_topk_topp(g.logits[b:b + 1].double(), k, p))
            assert torch.equal(kept[0], g.mask[b]), g.labels[b]
            assert bool(g.mask[b, g.argmax[b]])
            assert not bool((g.mask[b] & torch.isinf(g.logits[b])).any())


@pytest.mark.parametrize("V", sc.VOCABS)
def test_range_cases(V):
    for g, b, k, p in _rows(V, sc.range_groups):
        if p <= 1e-6:
            assert g.mask[b].nonzero().flatten().tolist() == \
                [int(g.argmax[b])], g.labels[b]
        if g.kinds[b] == "masked_few" and k > 0:
            assert k > int(torch.isfinite(g.logits[b]).sum())
