"""The routed MoE decode kernels for fp8 / mxfp4 experts (csrc/moe_decode.hip,
moe_skinny_gemm_q_kernel) and the quantised MoEMLP / Mixtral engine, against
fp64 on the exact effective weights and the unchanged bounds of
tests/moe_cases.py.

Measured on MI355X, worst case over each test's cases and table points (the
bounds are 1.0 and were never widened):

    routed GEMM, plain      fp8 0.7692  mxfp4 0.6807  of 2^-8 |ref| + 2^-12 A
    down + combine          fp8 0.6944  mxfp4 0.6298  of the same bound
    block, worst row err / max |ref row|, quantised against the bf16 twin
      fp8   T 1 .. 64  0.0033-0.0066 against 0.0055-0.0110; T 65 0.0097 / 0.0125
      mxfp4 T 1 .. 64  0.0033-0.0063 against 0.0062-0.0092 (I = 512); at
            I = 384 and at T = 65 both run the same library GEMMs: equal
    engine, logit error against the effective(bf16) twin over 8 steps:
      fp8 0.0117, mxfp4 0.0088; the 8 tokens were equal
"""
import dataclasses
import functools

import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS
from dynamo_amd.models.layers import TPContext, linear
from dynamo_amd.models.mixtral import MoEMLP
from tests import moe_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
FORMATS = ("fp8", "mxfp4")
HOLDERS = {"fp8": ops.Fp8ExpertWeight, "mxfp4": ops.Mxfp4ExpertWeight}
KS = {"fp8": (512, 1024), "mxfp4": (1024, 2048)}   # reach every table point
COUNTS = ((3, 0, 17, 5), (0, 17, 16), (16, 0, 0, 32), (33, 1), (0, 40, 0),
          (64,), (1,), (5, 0, 9))     # the last: several rows at T <= 16
ids = lambda c: "-".join(map(str, c))  # noqa: E731
fmt_p = pytest.mark.parametrize("fmt", FORMATS)


def _fits(fmt, K):
    kstep, configs, _ = ops.MOE_DECODE_FORMATS[fmt]
    return [c for c in configs if K % (c[0] * kstep * c[1]) == 0]


def _experts(fmt, gen, E, N, K):
    """Expert e drawn at std 0.02 * 2^(e mod 4), quantised by the project's
    quantiser -> (holder on the GPU, exact fp64 effective weights)."""
    std = 0.02 * 2.0 ** (torch.arange(E) % 4).view(E, 1, 1)
    h = HOLDERS[fmt].from_tensor((torch.randn(E, N, K, generator=gen)
                                  * std).to(BF))
    eff = (h.q.float().double() * h.scale.double()[:, :, None] if fmt == "fp8"
           else h.effective(torch.float64))
    return HOLDERS[fmt](h.q.to(DEV), h.scale.to(DEV)), eff


@functools.lru_cache(maxsize=None)
def _gemm_case(fmt, counts, K, N):
    """Top-1 routing with segment sizes `counts`, tokens shuffled ->
    (x, holder, topi, rows = x in sorted order, ref, A)."""
    gen = mc._gen("moe_quant_gemm", fmt, counts, K, N)
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
    seg_start, pair_of = ops.moe_route(topi, w.shape[0])
    return ops.moe_routed_gemm(x if gather else rows, h or w, seg_start,
                               pair_of, 1, gather=gather, glu=glu, cfg=cfg)


@fmt_p
def test_config_tables(fmt):
    assert ([tuple(c) for c in ops.hip().moe_decode_quant_configs()[fmt]]
            == list(ops.MOE_DECODE_FORMATS[fmt][1]))


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "direct"])
@pytest.mark.parametrize("N", [48, 160])
@pytest.mark.parametrize("ki", [0, 1])
@pytest.mark.parametrize("counts", COUNTS, ids=ids)
@fmt_p
def test_routed_gemm_plain(fmt, counts, ki, N, gather):
    case = _gemm_case(fmt, counts, KS[fmt][ki], N)
    worst = max(mc.assert_gemm_close(_routed(case, cfg, gather, False),
                                     case[4], case[5], f"cfg {cfg}")
                for cfg in _fits(fmt, KS[fmt][ki]))
    print(f"MOE_QUANT_RATIO {fmt} plain {worst:.4f}")


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "direct"])
@pytest.mark.parametrize("ki,I", [(0, 48), (1, 160)])
@pytest.mark.parametrize("counts", COUNTS, ids=ids)
@fmt_p
def test_routed_gemm_glu_bits(fmt, counts, ki, I, gather):
    case = _gemm_case(fmt, counts, KS[fmt][ki], 2 * I)
    for cfg in _fits(fmt, KS[fmt][ki]):
        fused = _routed(case, cfg, gather, True)
        assert fused.shape == (sum(counts), I)
        assert torch.equal(fused, ops.silu_mul(_routed(case, cfg, gather,
                                                       False))), f"cfg {cfg}"


@pytest.mark.parametrize("T", [1, 17, 64])
@pytest.mark.parametrize("D", [48, 256])
@fmt_p
def test_down_combine(fmt, D, T):
    E, K, I = 8, 2, KS[fmt][0]
    gen = mc._gen("moe_quant_down", fmt, D, T)
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
    seg_start, pair_of = ops.moe_route(topi.to(DEV), E)
    worst = 0.0
    for cfg in _fits(fmt, I):
        out = ops.moe_down_combine(act.to(DEV), h, seg_start, pair_of,
                                   topw.to(DEV), cfg=cfg)
        assert out.shape == (T, D) and out.dtype == BF
        worst = max(worst, mc.assert_gemm_close(out, ref, A, f"cfg {cfg}"))
    print(f"MOE_QUANT_RATIO {fmt} down_combine {worst:.4f}")


@pytest.mark.parametrize("counts", [(3, 0, 17, 5), (0, 40, 0)], ids=ids)
@fmt_p
def test_idle_experts_are_not_read(fmt, counts):
    """NaN codes and scales (0x7F e4m3 / NaN fp32; 0xFF e8m0) in every idle
    expert: read anywhere, they would reach the output or change its bits."""
    K = KS[fmt][1]
    case = _gemm_case(fmt, counts, K, 96)
    h = case[1]
    q, scale = h.q.clone(), h.scale.clone()
    for e, n in enumerate(counts):
        if n == 0:
            q[e].view(torch.uint8).fill_(0x7F if fmt == "fp8" else 0xFF)
            scale[e].fill_(float("nan") if fmt == "fp8" else 0xFF)
    for cfg in _fits(fmt, K):
        for glu in (False, True):
            out = _routed(case, cfg, True, glu, HOLDERS[fmt](q, scale))
            assert bool(torch.isfinite(out).all()), f"cfg {cfg}"
            assert torch.equal(out, _routed(case, cfg, True, glu)), f"cfg {cfg}"


# block: MoEMLP.forward with quantised experts. I = 384 is moe_cases' block
# (mxfp4 cannot route K = 384: its every T takes the host loop); I = 512
# routes in both formats.
@functools.lru_cache(maxsize=None)
def _blocks(fmt, I):
    """(quantised MoEMLP, its bf16 twin holding effective(bf16), fp64
    effective gate/up and down)."""
    cfg = dataclasses.replace(mc.block_config(), intermediate_size=I)
    q, twin = (MoEMLP(cfg, TPContext(), DEV, BF) for _ in range(2))
    mc.load_block_weights(q) if I == mc.BLK_I else q.router.copy_(
        mc.block_weights()[0])
    eff = []
    for name in ("w_gate_up", "w_down"):
        w = getattr(q, name)
        if I != mc.BLK_I:
            w.copy_(torch.randn(w.shape, generator=mc._gen(name, I))
                    / w.shape[2] ** 0.5)
        h = HOLDERS[fmt].from_tensor(w)
        setattr(q, name, h)
        eff.append(h.effective(torch.float64).cpu())
        getattr(twin, name).copy_(h.effective(BF))
    twin.router.copy_(q.router)
    return q, twin, eff[0], eff[1]


def _raise(*a, **kw):
    raise AssertionError("codes must not reach the bmm / grouped-seg routes")


def _forward(m, x):
    with torch.no_grad():
        out = m.forward(x)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T", [1, 17, 33, 64, 65])
@pytest.mark.parametrize("I", [mc.BLK_I, 512])
@fmt_p
def test_block(fmt, I, T, monkeypatch):
    q, twin, egu, ed = _blocks(fmt, I)
    x = mc.block_x(T).to(DEV)
    assert ops.moe_decode_ready(x, mc.BLK_K, q.w_gate_up, q.w_down) == (
        T <= 64 and (fmt == "fp8" or I == 512))
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
    monkeypatch.setattr(torch, "bmm", _raise)
    monkeypatch.setattr(ops, "moe_grouped_gemm_seg", _raise)
    e_new = float(mc.block_ratio(_forward(q, x), ref).max())
    print(f"MOE_QUANT_BLOCK {fmt} I{I} T{T} new {e_new:.5f} base {e_base:.5f}")
    assert e_new <= 2 * e_base


@fmt_p
def test_block_graph_replay(fmt, monkeypatch):
    """The routing is computed inside the captured graph: every replay routes
    its own x, and equals the eager result of that x bit for bit."""
    q = _blocks(fmt, 512)[0]
    monkeypatch.setattr(torch, "bmm", _raise)
    xs = [mc.block_x(16, variant=v).to(DEV) for v in range(4)]
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


# engine: tiny-mixtral-gpu
def _engine(fmt, model="tiny-mixtral-gpu", pool=None, **kw):
    cfg = EngineConfig(model=PRESETS[model], device=DEV,
                       max_num_seqs=kw.pop("max_num_seqs", 8),
                       max_batched_tokens=512, max_model_len=2048,
                       page_size=64, kv_pool_pages=256, weight_dtype=fmt, **kw)
    eng = LLMEngine(cfg, seed=7, weight_pool=pool)
    eng.logits = []            # an eager engine's last logits row, per step
    inner = eng.runner.model.compute_logits

    def record(h):
        out = inner(h)
        eng.logits.append(out[-1].float().cpu())
        return out
    if not cfg.enable_hip_graphs:
        eng.runner.model.compute_logits = record
    return eng


def _generate(eng, prompts):
    outs = [[] for _ in prompts]
    for i, p in enumerate(prompts):
        eng.add_request(str(i), p, SamplingParams(max_tokens=8))
    while eng.has_work():
        for so in eng.step():
            outs[int(so.req_id)].append(so.new_token)
    return outs


PROMPTS = [list(range(100, 180)), [7, 8, 9] * 10]
# Worst |logit difference| between a quantised engine and its effective(bf16)
# twin over the 8 steps below, measured on MI355X (fp8 0.0117, mxfp4 0.0088),
# times 2: both compute on the same effective weights and differ in summation
# order and rounding points only, and one more crossed bf16 rounding boundary
# doubles such a difference at most (the argument of test_gpu_fp8_weights.py).
LOGIT_ERR = {"fp8": 0.0234, "mxfp4": 0.0176}


@fmt_p
def test_engine(fmt):
    """An 80-token prompt prefills through the host loop, then decodes
    through the routed kernels. The logits stay within LOGIT_ERR of the
    twin's at every step, and the 8 tokens are the twin's; a first difference
    at a top-2 gap below LOGIT_ERR is reported, not failed."""
    eng = _engine(fmt)
    for layer in eng.runner.model.layers:
        assert isinstance(layer.moe.w_gate_up, HOLDERS[fmt])
        assert isinstance(layer.moe.w_down, HOLDERS[fmt])
    toks = _generate(eng, PROMPTS)
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
    # the engines see the same inputs up to and including step i
    errs = [float((p - t).abs().max())
            for p, t in zip(eager.logits[:i + 1], twin.logits)]
    print(f"MOE_QUANT_ENGINE {fmt} first difference {i} logit err "
          f"{max(errs):.4f}")
    assert max(errs) <= LOGIT_ERR[fmt]
    if i < 8:
        top2 = twin.logits[i].topk(2).values
        gap = float(top2[0] - top2[1])
        print(f"MOE_QUANT_ENGINE {fmt} token {i} differs at top-2 gap {gap:.4f}")
        assert gap < LOGIT_ERR[fmt], f"token {i} differs at a decisive gap"


@fmt_p
def test_engine_refusals(fmt):
    from dynamo_amd.gms import WeightPool
    from dynamo_amd.gms.pool import estimate_pool_bytes
    base = PRESETS["tiny-mixtral-gpu"]
    PRESETS["tiny-mixtral-ep"] = dataclasses.replace(base, moe_ep=True)
    PRESETS["tiny-mixtral-odd"] = dataclasses.replace(   # I % 128 != 0
        base, intermediate_size=1000)
    pool = WeightPool(estimate_pool_bytes(PRESETS["tiny-mixtral-gpu"]), "cpu")
    try:
        for what, kw in (("moe_ep", dict(model="tiny-mixtral-ep")),
                         ("'opt'", dict(model="tiny-opt")),
                         ("GMS", dict(pool=pool)),
                         ("max_num_seqs", dict(max_num_seqs=65)),
                         ("do not take", dict(model="tiny-mixtral-odd"))):
            with pytest.raises(ValueError, match=what):
                _engine(fmt, **kw)
    finally:
        del PRESETS["tiny-mixtral-ep"], PRESETS["tiny-mixtral-odd"]
    eng = _engine(fmt, max_num_seqs=65, enable_hip_graphs=False)
    from dynamo_amd.models.loader import export_hf
    for what, call in (("load_lora", lambda: eng.load_lora("a", rank=4)),
                       ("apply_weight_delta",
                        lambda: eng.apply_weight_delta(1, 1e-3)),
                       ("export_hf", lambda: export_hf(eng.runner.model, "x"))):
        with pytest.raises(ValueError, match=what):
            call()
