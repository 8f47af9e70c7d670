"""The tiled routed MoE kernels (csrc/moe_tile_gemm.hip) and the MoEMLP /
Mixtral engine on them, against torch_ref's route, fp64 on the exact
effective weights with the unchanged bounds of tests/moe_cases.py, and the
dense tiled kernel's bits. The route is opt-in: the tests switch it on through
ops.set_moe_tiled.

Measured on MI355X, worst case over each test's cases and table points (the
bounds are 1.0 and were never widened):

    routed GEMM, plain      fp8 0.7020  mxfp4 0.7075  of 2^-8 |ref| + 2^-12 A
    down + combine          fp8 0.7179  mxfp4 0.6829  of the same bound
    engine, logit error against the effective(bf16) twin over 8 steps:
      fp8 0.0117, mxfp4 0.0117
"""
import functools

import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.models.layers import linear
from dynamo_amd.models.mixtral import MoEMLP
from dynamo_amd.ops import torch_ref
from tests import moe_cases as mc
from tests.test_moe_tiled_cpu import ROUTE_CASES, route_topi
from tests.test_gpu_moe_decode_quant import (BF, DEV, HOLDERS, KS, PROMPTS,
                                             _blocks, _engine, _experts,
                                             _forward, _generate)

pytestmark = pytest.mark.gpu

FORMATS = ("fp8", "mxfp4")
COUNTS = ((70,), (0, 65, 0, 3), (31, 33, 1, 0, 64), (129, 0, 127), (1, 64))
ids = lambda c: "-".join(map(str, c))  # noqa: E731
fmt_p = pytest.mark.parametrize("fmt", FORMATS)
counts_p = pytest.mark.parametrize("counts", COUNTS, ids=ids)
gather_p = pytest.mark.parametrize("gather", [True, False],
                                   ids=["gather", "direct"])


@pytest.fixture(autouse=True)
def _switch_on():
    ops.set_moe_tiled(True)
    yield
    ops.set_moe_tiled(None)


def _fits(fmt, K):
    kstep = ops.MOE_DECODE_FORMATS[fmt][0]
    return [c for c in ops.MOE_TILE_CONFIGS[fmt]
            if K % (c[2] * kstep * c[4]) == 0]


@fmt_p
def test_config_tables(fmt):
    assert ([tuple(c) for c in ops.hip().moe_tile_configs()[fmt]]
            == list(ops.MOE_TILE_CONFIGS[fmt]))


@pytest.mark.parametrize("kind", ROUTE_CASES, ids=str)
def test_route(kind):
    topi, E = route_topi(kind)
    seg_ref, pair_ref = torch_ref.moe_route(topi, E)
    for BM in ops.MOE_TILE_BMS:
        seg, pair, te, tr, n = (t.cpu() for t in ops.moe_route_tiled(
            topi.to(DEV), E, BM))
        assert torch.equal(seg, seg_ref) and torch.equal(pair, pair_ref), BM
        te_ref, tr_ref, n_ref = torch_ref.moe_tile_map(seg_ref, BM)
        assert int(n) == n_ref <= topi.numel() // BM + min(E, topi.numel())
        assert torch.equal(te[:n_ref], te_ref), BM
        assert torch.equal(tr[:n_ref], tr_ref), BM


@functools.lru_cache(maxsize=None)
def _gemm_case(fmt, counts, K, N):
    """Top-1 routing with segment sizes `counts`, tokens shuffled ->
    (x, holder, topi, rows = x in sorted order, ref, A)."""
    gen = mc._gen("moe_tiled_gemm", fmt, counts, K, N)
    T = sum(counts)
    experts = torch.tensor([e for e, n in enumerate(counts) for _ in range(n)])
    topi = experts[torch.randperm(T, generator=gen)].view(T, 1).int()
    x = torch.randn(T, K, generator=gen).to(BF)
    h, eff = _experts(fmt, gen, len(counts), N, K)
    rows = x[torch.argsort(topi.flatten().long(), stable=True)]
    return (x.to(DEV), h, topi.to(DEV), rows.to(DEV),
            *mc.gemm_reference(rows, eff, counts))


def _routed(case, cfg, gather, glu, h=None):
    x, w, topi, rows = case[:4]
    route = ops.moe_route_tiled(topi, w.shape[0], cfg[0])
    return ops.moe_tiled_gemm(x if gather else rows, h or w, route, 1,
                              gather=gather, glu=glu, cfg=cfg)


def _dense(fmt, rows, h, e, wk):
    """The dense tiled kernel on `rows` with expert e's weight, at WK = wk."""
    K = rows.shape[1]
    point = next(c for c in ops.TILE_GEMM_CONFIGS[fmt] if c[2] == wk
                 and K % (wk * ops.TILE_GEMM_KSTEP[fmt] * c[4]) == 0)
    y = torch.empty(rows.shape[0], h.shape[1], dtype=BF, device=DEV)
    getattr(ops.hip(), fmt + "_tile_gemm")(y, rows, h.q[e], h.scale[e],
                                           *point, False)
    return y


@gather_p
@pytest.mark.parametrize("N", [48, 160])
@pytest.mark.parametrize("ki", [0, 1])
@counts_p
@fmt_p
def test_tiled_gemm_plain(fmt, counts, ki, N, gather):
    """Within the fp64 bound, and every segment bit-equal to the dense tiled
    kernel on its rows with w[e] at the same WK."""
    case = _gemm_case(fmt, counts, KS[fmt][ki], N)
    seg = [0] + torch.tensor(counts).cumsum(0).tolist()
    dense, worst = {}, 0.0
    for cfg in _fits(fmt, KS[fmt][ki]):
        out = _routed(case, cfg, gather, False)
        worst = max(worst, mc.assert_gemm_close(out, case[4], case[5],
                                                f"cfg {cfg}"))
        for e, n in enumerate(counts):
            if n == 0:
                continue
            if (e, cfg[2]) not in dense:
                dense[e, cfg[2]] = _dense(fmt, case[3][seg[e]:seg[e + 1]],
                                          case[1], e, cfg[2])
            assert torch.equal(out[seg[e]:seg[e + 1]], dense[e, cfg[2]]), (
                f"cfg {cfg} expert {e}")
    print(f"MOE_TILED_RATIO {fmt} plain {worst:.4f}")


@gather_p
@pytest.mark.parametrize("ki,I", [(0, 48), (1, 160)])
@counts_p
@fmt_p
def test_tiled_gemm_glu_bits(fmt, counts, ki, I, gather):
    case = _gemm_case(fmt, counts, KS[fmt][ki], 2 * I)
    for cfg in _fits(fmt, KS[fmt][ki]):
        fused = _routed(case, cfg, gather, True)
        assert fused.shape == (sum(counts), I)
        assert torch.equal(fused, ops.silu_mul(_routed(case, cfg, gather,
                                                       False))), f"cfg {cfg}"


@pytest.mark.parametrize("T", [65, 130])
@pytest.mark.parametrize("D", [48, 256])
@fmt_p
def test_down_combine(fmt, D, T):
    E, K, I = 8, 2, KS[fmt][0]
    gen = mc._gen("moe_tiled_down", fmt, D, T)
    topi = torch.rand(T, E, generator=gen).argsort(-1)[:, :K].int()
    topw = torch.rand(T, K, generator=gen) + 0.1
    topw = topw / topw.sum(-1, keepdim=True)
    act = torch.randn(T * K, I, generator=gen).to(BF)
    h, eff = _experts(fmt, gen, E, D, I)
    flat = topi.flatten().long()
    inv = torch.argsort(torch.argsort(flat, stable=True))   # pair -> position
    counts = torch.bincount(flat, minlength=E).tolist()
    ref, A = ((t[inv].view(T, K, D) * topw.double().unsqueeze(-1)).sum(1)
              for t in mc.gemm_reference(act, eff, counts))
    worst = 0.0
    for cfg in _fits(fmt, I):
        route = ops.moe_route_tiled(topi.to(DEV), E, cfg[0])
        out = ops.moe_tiled_down_combine(act.to(DEV), h, route, topw.to(DEV),
                                         cfg=cfg)
        assert out.shape == (T, D) and out.dtype == BF
        worst = max(worst, mc.assert_gemm_close(out, ref, A, f"cfg {cfg}"))
    print(f"MOE_TILED_RATIO {fmt} down_combine {worst:.4f}")


@pytest.mark.parametrize("counts", [(0, 65, 0, 3), (129, 0, 127)], ids=ids)
@fmt_p
def test_idle_experts_are_not_read(fmt, counts):
    """NaN codes and scales (0x7F e4m3 / NaN fp32; 0xFF e8m0) in every idle
    expert: read anywhere, they would reach the output or change its bits."""
    K = KS[fmt][1]
    case = _gemm_case(fmt, counts, K, 96)
    q, scale = case[1].q.clone(), case[1].scale.clone()
    for e, n in enumerate(counts):
        if n == 0:
            q[e].view(torch.uint8).fill_(0x7F if fmt == "fp8" else 0xFF)
            scale[e].fill_(float("nan") if fmt == "fp8" else 0xFF)
    for cfg in _fits(fmt, K):
        for glu in (False, True):
            out = _routed(case, cfg, True, glu, HOLDERS[fmt](q, scale))
            assert bool(torch.isfinite(out).all()), f"cfg {cfg}"
            assert torch.equal(out, _routed(case, cfg, True, glu)), f"cfg {cfg}"


def _raise(*a, **kw):
    raise AssertionError("the tiled route must not reach the expert loop")


@pytest.mark.parametrize("T", [65, 130, 257])
@fmt_p
def test_block(fmt, T, monkeypatch):
    """MoEMLP.forward stays on the device, and is no further from fp64 on the
    effective weights than twice the bf16 twin; switched off, the same call
    takes the host loop."""
    I = 512
    q, twin, egu, ed = _blocks(fmt, I)
    x = mc.block_x(T).to(DEV)
    assert ops.moe_tiled_ready(x, mc.BLK_K, q.w_gate_up, q.w_down)
    topw, topi = (t.cpu() for t in ops.topk_gating(
        linear(x, q.router).float(), mc.BLK_K))
    gu = torch.einsum("td,end->etn", x.cpu().double(), egu)
    g, u = gu[..., :I], gu[..., I:]
    Y = torch.einsum("eti,edi->etd", g * torch.sigmoid(g) * u, ed)
    tok = torch.arange(T).repeat_interleave(mc.BLK_K)
    ref = torch.zeros(T, mc.BLK_D, dtype=torch.float64).index_add_(
        0, tok, Y[topi.flatten().long(), tok]
        * topw.double().flatten().unsqueeze(-1))
    e_base = float(mc.block_ratio(_forward(twin, x), ref).max())
    monkeypatch.setattr(MoEMLP, "_expert_loop", _raise)
    monkeypatch.setattr(torch, "bmm", _raise)
    e_new = float(mc.block_ratio(_forward(q, x), ref).max())
    print(f"MOE_TILED_BLOCK {fmt} T{T} new {e_new:.5f} base {e_base:.5f}")
    assert e_new <= 2 * e_base
    ops.set_moe_tiled(False)
    with pytest.raises(AssertionError, match="expert loop"):
        _forward(q, x)


@fmt_p
def test_block_graph_replay(fmt, monkeypatch):
    """The routing and the tile map are computed inside the captured graph:
    every replay routes its own x, and equals the eager result of that x bit
    for bit."""
    q = _blocks(fmt, 512)[0]
    monkeypatch.setattr(MoEMLP, "_expert_loop", _raise)
    xs = [mc.block_x(96, variant=v).to(DEV) for v in range(4)]
    eager = [_forward(q, x) for x in xs]
    static_x = xs[0].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():   # one stream, no branches
        static_out = q.forward(static_x)
    for v in (1, 2, 3, 0):
        static_x.copy_(xs[v])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager[v]), f"replay of variant {v}"


# Worst |logit difference| between a quantised engine whose prefill takes the
# tiled route and its effective(bf16) twin over the 8 steps below, measured on
# MI355X (fp8 0.0117, mxfp4 0.0117), times 2: the
# argument of LOGIT_ERR in test_gpu_moe_decode_quant.py.
LOGIT_ERR = {"fp8": 0.0234, "mxfp4": 0.0234}


@fmt_p
def test_engine(fmt, monkeypatch):
    """The 80-token prompt prefills through the tiled route (the host loop
    raises), then decodes through the routed decode kernels; repeatable
    across engines and across graphs on and off, and within LOGIT_ERR of the
    twin at every step. A first token difference at a top-2 gap below
    LOGIT_ERR is reported, not failed."""
    monkeypatch.setattr(MoEMLP, "_expert_loop", _raise)
    toks = _generate(_engine(fmt), PROMPTS)
    assert all(len(t) == 8 for t in toks)
    assert _generate(_engine(fmt), PROMPTS) == toks
    assert _generate(_engine(fmt, enable_hip_graphs=False), PROMPTS) == toks
    eager = _engine(fmt, enable_hip_graphs=False)
    twin = _engine("bf16", enable_hip_graphs=False)
    for lq, lt in zip(eager.runner.model.layers, twin.runner.model.layers):
        for sub, name in (("attn", "wqkv"), ("attn", "wo"),
                          ("moe", "w_gate_up"), ("moe", "w_down")):
            getattr(getattr(lt, sub), name).copy_(
                getattr(getattr(lq, sub), name).effective(BF))
    a, b = _generate(eager, PROMPTS[:1])[0], _generate(twin, PROMPTS[:1])[0]
    i = next((i for i in range(8) if a[i] != b[i]), 8)   # first difference
    errs = [float((p - t).abs().max())
            for p, t in zip(eager.logits[:i + 1], twin.logits)]
    print(f"MOE_TILED_ENGINE {fmt} first difference {i} logit err "
          f"{max(errs):.4f}")
    assert max(errs) <= LOGIT_ERR[fmt]
    if i < 8:
        top2 = twin.logits[i].topk(2).values
        gap = float(top2[0] - top2[1])
        print(f"MOE_TILED_ENGINE {fmt} token {i} differs at top-2 gap {gap:.4f}")
        assert gap < LOGIT_ERR[fmt], f"token {i} differs at a decisive gap"


@fmt_p
def test_engine_batch_limit(fmt, monkeypatch):
    """The switch lifts the hipGraph batch refusal from the decode kernels'
    64 to MOE_TILE_MAX_T, and no further: a batch of 65 decodes under graphs
    on the tiled route, with the tokens of the eager engine. Off, 65 is
    refused as before."""
    monkeypatch.setattr(MoEMLP, "_expert_loop", _raise)
    prompts = [[7 + i, 8, 9] for i in range(65)]
    eng = _engine(fmt, max_num_seqs=65)
    assert eng.runner.cfg.enable_hip_graphs
    toks = _generate(eng, prompts)           # decodes 65 rows per step
    assert all(len(t) == 8 for t in toks)
    assert toks == _generate(_engine(fmt, max_num_seqs=65,
                                     enable_hip_graphs=False), prompts)
    with pytest.raises(ValueError, match=f"up to {ops.MOE_TILE_MAX_T} tokens"):
        _engine(fmt, max_num_seqs=ops.MOE_TILE_MAX_T + 1)
    ops.set_moe_tiled(False)
    with pytest.raises(ValueError, match=f"up to {ops.MOE_DECODE_MAX_T} tokens"):
        _engine(fmt, max_num_seqs=65)
