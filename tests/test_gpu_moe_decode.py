"""The routed MoE decode kernels (csrc/moe_decode.hip) and the opt-in
DYNAMO_MOE_FUSED route of `MoEMLP.forward` against the fp64 references and
the bounds of tests/moe_cases.py, which are used unchanged.

Measured on MI355X, worst case over each test's cases and table points (the
bounds are 1.0 and were never widened):

    routed GEMM, plain      0.7356  of 2^-8 |ref| + 2^-12 A
    down + combine          0.6621  of the same bound
    block, T 1 .. 64        0.1133  of tau_blk * S_row (T = 65, bmm: 0.1628)
"""
import functools

import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.models.layers import TPContext, linear
from dynamo_amd.models.mixtral import MoEMLP
from tests import moe_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
CONFIGS = ops.MOE_DECODE_CONFIGS
COUNTS = ((3, 0, 17, 5), (0, 17, 16), (16, 0, 0, 32), (1,), (0, 0, 1, 0),
          (33, 1), (0, 40, 0), (64,))


def _fits(K):
    return [c for c in CONFIGS if K % (c[0] * 64 * c[1]) == 0]


def _distinct_topi(gen, T, E, K, same_first=False):
    """[T, K] int32, distinct experts per token; with `same_first` every
    token's first pick is expert 0."""
    if not same_first:
        return torch.rand(T, E, generator=gen).argsort(-1)[:, :K].int()
    rest = 1 + torch.rand(T, E - 1, generator=gen).argsort(-1)[:, :K - 1]
    return torch.cat([torch.zeros(T, 1, dtype=torch.long), rest], 1).int()


def test_config_table():
    assert [tuple(c) for c in ops.hip().moe_decode_configs()] == list(CONFIGS)
    assert (1, 1, 2) in CONFIGS and len(CONFIGS) <= 8


@pytest.mark.parametrize("same_first", [False, True])
@pytest.mark.parametrize("E,K,T", [(8, 2, 1), (8, 2, 64), (4, 1, 17),
                                   (64, 8, 64), (8, 2, 5)])
def test_route(E, K, T, same_first):
    topi = _distinct_topi(mc._gen("moe_route", E, K, T), T, E, K, same_first)
    seg_start, pair_of = ops.moe_route(topi.to(DEV), E)
    flat = topi.flatten().long()
    assert torch.equal(pair_of.cpu().long(), torch.argsort(flat, stable=True))
    want = torch.zeros(E + 1, dtype=torch.long)
    want[1:] = torch.bincount(flat, minlength=E).cumsum(0)
    assert torch.equal(seg_start.cpu().long(), want)


@functools.lru_cache(maxsize=None)
def _gemm_case(counts, D, N):
    """Top-1 routing with the segment sizes `counts`, tokens in a shuffled
    order -> (x [T, D], w [E, N, D], topi [T, 1], rows = x in sorted order,
    ref, A)."""
    gen = mc._gen("moe_decode_gemm", counts, D, N)
    T = sum(counts)
    experts = torch.tensor([e for e, n in enumerate(counts) for _ in range(n)])
    topi = experts[torch.randperm(T, generator=gen)].view(T, 1).int()
    x = torch.randn(T, D, generator=gen).to(BF)
    w = torch.randn(len(counts), N, D, generator=gen).to(BF)
    rows = x[torch.argsort(topi.flatten().long(), stable=True)]
    return x, w, topi, rows, *mc.gemm_reference(rows, w, counts)


def _routed(case, cfg, gather, glu):
    x, w, topi, rows = (t.to(DEV) for t in case[:4])
    seg_start, pair_of = ops.moe_route(topi, w.shape[0])
    return ops.moe_routed_gemm(x if gather else rows, w, seg_start, pair_of,
                               1, gather=gather, glu=glu, cfg=cfg)


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "direct"])
@pytest.mark.parametrize("D,N", [(512, 48), (1024, 160)])
@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: "-".join(map(str, c)))
def test_routed_gemm_plain(counts, D, N, gather):
    case = _gemm_case(counts, D, N)
    worst = 0.0
    for cfg in _fits(D):
        y = _routed(case, cfg, gather, False)
        worst = max(worst, mc.assert_gemm_close(y, case[4], case[5],
                                                f"cfg {cfg}"))
    print(f"MOE_DECODE_RATIO plain {worst:.4f}")


def test_routed_gemm_top2_gather():
    """Two pairs per token: the gathered row of pair p is x[p // 2]."""
    E, T, K, D, N = 8, 16, 2, 512, 48
    gen = mc._gen("moe_decode_top2")
    topi = _distinct_topi(gen, T, E, K)
    x = torch.randn(T, D, generator=gen).to(BF)
    w = torch.randn(E, N, D, generator=gen).to(BF)
    order = torch.argsort(topi.flatten().long(), stable=True)
    counts = torch.bincount(topi.flatten().long(), minlength=E).tolist()
    ref, A = mc.gemm_reference(x[order // K], w, counts)
    seg_start, pair_of = ops.moe_route(topi.to(DEV), E)
    y = ops.moe_routed_gemm(x.to(DEV), w.to(DEV), seg_start, pair_of, K,
                            gather=True, glu=False)
    mc.assert_gemm_close(y, ref, A, "top-2 gather")


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "direct"])
@pytest.mark.parametrize("D,I", [(512, 48), (1024, 160)])
@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: "-".join(map(str, c)))
def test_routed_gemm_glu_bits(counts, D, I, gather):
    case = _gemm_case(counts, D, 2 * I)
    for cfg in _fits(D):
        fused = _routed(case, cfg, gather, True)
        plain = _routed(case, cfg, gather, False)
        assert fused.shape == (sum(counts), I)
        assert torch.equal(fused, ops.silu_mul(plain)), f"cfg {cfg}"


@pytest.mark.parametrize("T", [1, 17, 64])
@pytest.mark.parametrize("I,D", [(384, 48), (384, 256), (1024, 48),
                                 (1024, 256)])
def test_down_combine(I, D, T):
    E, K = 8, 2
    gen = mc._gen("moe_decode_down", I, D, T)
    topi = _distinct_topi(gen, T, E, K)
    topw = torch.rand(T, K, generator=gen) + 0.1
    topw = topw / topw.sum(-1, keepdim=True)
    act = torch.randn(T * K, I, generator=gen).to(BF)
    w = torch.randn(E, D, I, generator=gen).to(BF)
    flat = topi.flatten().long()
    inv = torch.argsort(torch.argsort(flat, stable=True))   # pair -> position
    counts = torch.bincount(flat, minlength=E).tolist()
    wt = topw.double().unsqueeze(-1)
    ref, A = ((t[inv].view(T, K, D) * wt).sum(1)
              for t in mc.gemm_reference(act, w, counts))
    seg_start, pair_of = ops.moe_route(topi.to(DEV), E)
    worst = 0.0
    for cfg in _fits(I):
        out = ops.moe_down_combine(act.to(DEV), w.to(DEV), seg_start, pair_of,
                                   topw.to(DEV), cfg=cfg)
        assert out.shape == (T, D) and out.dtype == BF
        worst = max(worst, mc.assert_gemm_close(out, ref, A, f"cfg {cfg}"))
    print(f"MOE_DECODE_RATIO down_combine {worst:.4f}")


# --------------------------------------------------------------------------
# block: MoEMLP.forward with DYNAMO_MOE_FUSED=1
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moe():
    m = MoEMLP(mc.block_config(), TPContext(), DEV, BF)
    mc.load_block_weights(m)
    return m


def _raise(*a, **kw):
    raise AssertionError("the fused route must not reach the bmm/seg routes")


def _forward(m, x):
    with torch.no_grad():
        out = m.forward(x)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T", [1, 5, 16, 17, 64, 65])
def test_block_fused(moe, monkeypatch, T):
    monkeypatch.setenv("DYNAMO_MOE_FUSED", "1")
    x = mc.block_x(T).to(DEV)
    ref = mc.block_reference(x.cpu(), linear(x, moe.router).float())
    if T <= 64:              # 65 is past the route's limit: today's routes
        monkeypatch.setattr(torch, "bmm", _raise)
        monkeypatch.setattr(ops, "moe_grouped_gemm_seg", _raise)
    worst = mc.assert_block_close(_forward(moe, x), ref, what=f"fused T={T}")
    print(f"MOE_BLOCK_RATIO fused T{T} {worst:.4f}")


def test_block_fused_graph_replay(moe, monkeypatch):
    """The routing is computed inside the captured graph: every replay routes
    its own x, and equals the eager result of that x bit for bit."""
    T = 16
    monkeypatch.setenv("DYNAMO_MOE_FUSED", "1")
    monkeypatch.setattr(torch, "bmm", _raise)
    xs = [mc.block_x(T, variant=v).to(DEV) for v in range(4)]
    picks = [ops.topk_gating(linear(x, moe.router).float(), mc.BLK_K)[1].cpu()
             for x in xs]
    assert all(not torch.equal(picks[i], picks[j])
               for i in range(4) for j in range(i)), "routings must differ"
    eager = [_forward(moe, x) for x in xs]
    static_x = xs[0].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():   # one stream, no branches
        static_out = moe.forward(static_x)
    for v in (1, 2, 3, 0):
        static_x.copy_(xs[v])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager[v]), f"replay of variant {v}"
