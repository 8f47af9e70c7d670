"""SwiGLU fused into the in-tree gate/up decode GEMM (the GLU mode of
csrc/skinny_gemm_impl.h), its dispatch (ops.linear_silu_mul) and its use by
SwiGLUMLP.

Every comparison is torch.equal against the two-kernel path on the same
device: ops.silu_mul of the unfused in-tree GEMM at the same configuration.
That path has its own tests against fp32 references, so equality carries
their guarantees over and no tolerance appears here.

Inputs are seeded: x ~ N(0, 1), W ~ N(0, 0.02) with every row scaled by its
own factor in [0.5, 2) (a gate/up pairing that is shifted by a tile or taken
from the wrong half then changes the result), and four gate rows aligned with
x[0] so that gate[0, j] is about +-200, where __expf(-gate) overflows or
vanishes.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS
from dynamo_amd.ops import (Fp8Weight, Mxfp4Weight, quantize_fp8_rowwise,
                            quantize_mxfp4)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7B7B

# format -> (binding, k per pipeline step, smallest K, M values that reach
# every MT of the format)
FORMATS = {
    "bf16_coalesced": ("skinny_gemm", 64, 2048, (1, 7, 16)),
    "fp8": ("fp8_skinny_gemm", 128, 0, (1, 7, 16, 17, 33, 64)),
    "mxfp4": ("mxfp4_skinny_gemm", 256, 0, (1, 7, 16, 17, 32)),
}
TABLES = {
    # the header's SKINNY_GEMM_COAL_CONFIGS; test_tables_agree checks it
    "bf16_coalesced": ((8, 1, 2), (8, 1, 4), (8, 2, 2), (4, 2, 2), (8, 2, 4),
                       (2, 2, 8), (1, 4, 2), (1, 2, 4), (1, 4, 4), (1, 8, 2),
                       (1, 2, 2), (1, 1, 8), (1, 2, 8)),
    "fp8": ops.FP8_GEMM_CONFIGS,
    "mxfp4": ops.MXFP4_GEMM_CONFIGS,
}
GLU_CASES = [(fmt, cfg) for fmt, table in TABLES.items() for cfg in table
             if ops.glu_capable(fmt, cfg)]


@pytest.fixture(autouse=True)
def _switch_follows_default(monkeypatch):
    monkeypatch.delenv("DYNAMO_FUSED_GLU", raising=False)
    monkeypatch.delenv("DYNAMO_SKINNY_GEMM", raising=False)
    ops.set_fused_glu(None)
    ops.set_skinny_gemm(None)
    yield
    ops.set_fused_glu(None)
    ops.set_skinny_gemm(None)


def _case_k(fmt, cfg):
    """Three pipeline rounds of the configuration, so that prologue, main
    loop and drain all run; at least the format's smallest K."""
    _, kstep, min_k, _ = FORMATS[fmt]
    return max(3 * cfg[0] * kstep * cfg[1], min_k)


@functools.lru_cache(maxsize=None)
def _case(fmt, K, I):
    """Seeded (x64 [64, K] bf16, weight arguments of the format's binding for
    a gate/up weight [2I, K]); read-only."""
    g = torch.Generator(device=DEV)
    g.manual_seed(100003 * K + 2 * I + len(fmt))
    x = torch.randn(64, K, generator=g, device=DEV).to(torch.bfloat16)
    w = torch.randn(2 * I, K, generator=g, device=DEV) * 0.02
    w *= 0.5 + 1.5 * torch.rand(2 * I, 1, generator=g, device=DEV)
    # gate rows of the first and the last tile: gate[0, j] ~ +-200
    x0 = x[0].float()
    for j, s in ((0, 200.0), (1, -200.0), (I - 1, 200.0), (I - 2, -200.0)):
        w[j] = x0 * (s / x0.square().sum())
    w = w.to(torch.bfloat16)
    if fmt == "fp8":
        return x, quantize_fp8_rowwise(w)
    if fmt == "mxfp4":
        return x, quantize_mxfp4(w)
    return x, (w,)


def _launch(fmt, y, x, wargs, cfg, nt, glu):
    tail = (nt, True, glu) if fmt == "bf16_coalesced" else (nt, glu)
    getattr(ops.hip(), FORMATS[fmt][0])(y, x, *wargs, *cfg, *tail)
    return y


def _two_kernels(fmt, x, wargs, cfg, nt):
    """(silu_mul of the unfused in-tree GEMM, that GEMM's result)."""
    gu = torch.empty(x.shape[0], wargs[0].shape[0], dtype=torch.bfloat16,
                     device=DEV)
    _launch(fmt, gu, x, wargs, cfg, nt, False)
    return ops.silu_mul(gu), gu


@pytest.mark.parametrize("nt", [False, True], ids=["default", "nt"])
@pytest.mark.parametrize("fmt,cfg", GLU_CASES,
                         ids=[f"{f}-{c}" for f, c in GLU_CASES])
def test_kernel_equals_two_kernels(fmt, cfg, nt):
    # I: the block's NT / 2 tiles and one more. For NT >= 4 the last block is
    # half empty and the col < I guard acts; for NT = 2 a block owns one tile
    # and I % 16 == 0 leaves every block full, so the guard never fires there.
    K, I = _case_k(fmt, cfg), 16 * (cfg[2] // 2) + 16
    x64, wargs = _case(fmt, K, I)
    for M in FORMATS[fmt][3]:
        x = x64[:M]
        expect, gu = _two_kernels(fmt, x, wargs, cfg, nt)
        if M == FORMATS[fmt][3][0]:
            gate0 = gu[0, :I].float()
            assert gate0.max() > 90 and gate0.min() < -90
        buf = torch.full((M + 2, I), SENTINEL, dtype=torch.int16, device=DEV)
        y = buf[1:M + 1].view(torch.bfloat16)
        _launch(fmt, y, x, wargs, cfg, nt, True)
        assert torch.equal(y, expect), f"M={M}"
        assert torch.isfinite(y.float()).all()
        assert (buf[0] == SENTINEL).all() and (buf[M + 1] == SENTINEL).all()


def test_tables_agree():
    """The Python copies of the tables and of the GLU predicate against what
    the extension can launch."""
    hip = ops.hip()
    plain, glu = hip.skinny_gemm_configs(), hip.skinny_gemm_glu_configs()
    for fmt, table in TABLES.items():
        assert set(plain[fmt]) == set(table)
        assert set(glu[fmt]) == {c for c in table if ops.glu_capable(fmt, c)}
    assert glu["bf16_plain"] == []
    assert not any(ops.glu_capable("bf16_plain", c)
                   for c in plain["bf16_plain"])
    # every shipped gate/up configuration has a fused form
    assert ops.glu_capable("bf16_coalesced", ops.SKINNY_GEMM_SHAPES[
        (57344, 8192)])
    for shapes, fmt in ((ops.FP8_GEMM_SHAPES, "fp8"),
                        (ops.MXFP4_GEMM_SHAPES, "mxfp4")):
        for cfg in shapes[(57344, 8192)]:
            assert ops.glu_capable(fmt, cfg)


def test_binding_rejects_what_it_cannot_fuse():
    hip = ops.hip()
    x64, (q, scale) = _case("fp8", 384, 32)
    y = torch.empty(16, 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):      # odd NT
        hip.fp8_skinny_gemm(y, x64[:16], q, scale, 1, 1, 1, True, True)
    with pytest.raises(RuntimeError):      # y must be [M, N / 2]
        hip.fp8_skinny_gemm(torch.empty(16, 64, dtype=torch.bfloat16,
                                        device=DEV),
                            x64[:16], q, scale, 1, 1, 2, True, True)
    with pytest.raises(RuntimeError):      # N = 48: I is no multiple of 16
        hip.fp8_skinny_gemm(torch.empty(16, 24, dtype=torch.bfloat16,
                                        device=DEV),
                            x64[:16], q[:48].contiguous(),
                            scale[:48].contiguous(), 1, 1, 2, True, True)
    x64, (w,) = _case("bf16_coalesced", 2048, 32)
    with pytest.raises(RuntimeError):      # the plain format has no GLU form
        hip.skinny_gemm(y, x64[:16], w, 4, 4, 2, False, False, True)
    with pytest.raises(RuntimeError):      # bf16 (8, 1, 4) is not built
        hip.skinny_gemm(y, x64[:16], w, 8, 1, 4, True, True, True)


# ---- dispatch --------------------------------------------------------------
def _unfused(x, w):
    return ops.silu_mul(ops.linear(x, w))


def _assert_falls_back(x, w):
    assert ops.fused_glu_config(x, w) is None
    assert torch.equal(ops.linear_silu_mul(x, w), _unfused(x, w))


def test_dispatch_quantised_takes_the_fused_kernel(monkeypatch):
    for fmt, holder, binding, path in (
            ("fp8", Fp8Weight, "fp8_skinny_gemm", ops.fp8_linear_path),
            ("mxfp4", Mxfp4Weight, "mxfp4_skinny_gemm",
             ops.mxfp4_linear_path)):
        x64, wargs = _case(fmt, 1024, 48)
        w = holder(*wargs)
        for M in (1, 16, 32):
            x = x64[:M]
            name, cfg = ops.fused_glu_config(x, w)
            assert name == binding and ("kernel", cfg) == path(x, w)
            y = ops.linear_silu_mul(x, w)
            assert y.shape == (M, 48)
            ops.set_fused_glu(False)
            assert torch.equal(y, ops.linear_silu_mul(x, w))
            assert torch.equal(y, _unfused(x, w))
            ops.set_fused_glu(None)
        # a format that is not listed as shipped stays on two kernels
        with monkeypatch.context() as m:
            m.setattr(ops, "FUSED_GLU_FORMATS", ("bf16_coalesced",))
            _assert_falls_back(x64[:16], w)


def test_dispatch_falls_back_on_odd_nt(monkeypatch):
    x64, wargs = _case("fp8", 1024, 48)
    w = Fp8Weight(*wargs)
    monkeypatch.setattr(ops, "FP8_GEMM_SHAPES",
                        {(96, 1024): ((1, 1, 1), (1, 1, 1))})
    assert ops.fp8_linear_path(x64[:16], w) == ("kernel", (1, 1, 1))
    _assert_falls_back(x64[:16], w)


def test_dispatch_falls_back_when_i_is_no_tile_multiple():
    x64, (q, scale) = _case("fp8", 1024, 48)
    w = Fp8Weight(q[:80].contiguous(), scale[:80].contiguous())   # I = 40
    assert ops.fp8_linear_path(x64[:16], w)[0] == "kernel"
    _assert_falls_back(x64[:16], w)


def test_dispatch_falls_back_above_the_formats_m_limit():
    x64, wargs = _case("fp8", 1024, 48)
    x65 = torch.cat([x64, x64[:1]])
    _assert_falls_back(x65, Fp8Weight(*wargs))
    x64, wargs = _case("mxfp4", 1024, 48)
    _assert_falls_back(x64[:33], Mxfp4Weight(*wargs))


def test_dispatch_switch_off(monkeypatch):
    x64, wargs = _case("fp8", 1024, 48)
    w, x = Fp8Weight(*wargs), x64[:16]
    assert ops.fused_glu_config(x, w) is not None
    ops.set_fused_glu(False)
    _assert_falls_back(x, w)
    ops.set_fused_glu(None)
    monkeypatch.setenv("DYNAMO_FUSED_GLU", "0")
    _assert_falls_back(x, w)
    ops.set_fused_glu(True)     # the override wins over the environment
    assert ops.fused_glu_config(x, w) is not None
    # bf16 the same
    x64, (wb,) = _case("bf16_coalesced", 2048, 48)
    xb = x64[:16]
    monkeypatch.setattr(ops, "SKINNY_GEMM_SHAPES",
                        {(96, 2048): (1, 2, 2, True, True)})
    ops.set_fused_glu(None)
    _assert_falls_back(xb, wb)                # the env still says 0
    monkeypatch.setenv("DYNAMO_FUSED_GLU", "1")
    assert ops.fused_glu_config(xb, wb) is not None
    monkeypatch.delenv("DYNAMO_FUSED_GLU")
    assert ops.fused_glu_config(xb, wb) is not None
    ops.set_fused_glu(False)
    _assert_falls_back(xb, wb)


def test_dispatch_falls_back_on_non_contiguous_x():
    x64, wargs = _case("fp8", 1024, 48)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    x = torch.randn(16, 2048, generator=g,
                    device=DEV).to(torch.bfloat16)[:, :1024]
    assert not x.is_contiguous()
    _assert_falls_back(x, Fp8Weight(*wargs))


@pytest.mark.parametrize("cfg", [(1, 2, 2, True, True), (1, 4, 2, True, True)])
def test_dispatch_bf16_shape_hit_equals_the_library(monkeypatch, cfg):
    """A WPB = 1 entry sums K in order in one accumulator, as the library's
    kernel for these shapes does: the fused result equals silu_mul(F.linear)."""
    x64, (w,) = _case("bf16_coalesced", 2048, 48)
    x = x64[:16]
    _assert_falls_back(x, w)                  # not a shipped shape
    monkeypatch.setattr(ops, "SKINNY_GEMM_SHAPES", {(96, 2048): cfg})
    assert ops.fused_glu_config(x, w) == ("skinny_gemm", cfg)
    y = ops.linear_silu_mul(x, w)
    assert torch.equal(y, ops.silu_mul(F.linear(x, w)))
    assert torch.equal(y, _unfused(x, w))
    ops.set_skinny_gemm(False)                # library GEMM: nothing to fuse
    _assert_falls_back(x, w)


def test_graph_replay_equals_eager():
    x64, wargs = _case("fp8", 1024, 48)
    w = Fp8Weight(*wargs)
    xs = x64[:16].clone()
    eager = ops.linear_silu_mul(xs, w)
    assert ops.fused_glu_config(xs, w) is not None
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.linear_silu_mul(xs, w)            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.linear_silu_mul(xs, w)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    # the graph reads xs at replay time
    xs.copy_(x64[16:32])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.linear_silu_mul(x64[16:32].contiguous(), w))


# ---- engine ------------------------------------------------------------------
PROMPTS = [list(range(100, 180)), [7, 8, 9] * 10, list(range(300, 340))]


def _engine(**kw):
    cfg = EngineConfig(model=PRESETS["tiny-llama-gpu"], device=DEV,
                       max_num_seqs=8, max_batched_tokens=512,
                       max_model_len=2048, page_size=64, kv_pool_pages=256,
                       **kw)
    return LLMEngine(cfg, seed=7)


def _generate(engine, max_tokens=8):
    outs = {f"r{i}": [] for i in range(len(PROMPTS))}
    for i, p in enumerate(PROMPTS):
        engine.add_request(f"r{i}", p, SamplingParams(max_tokens=max_tokens))
    steps = 0
    while engine.has_work():
        for so in engine.step():
            outs[so.req_id].append(so.new_token)
        steps += 1
        assert steps < 1000
    return [outs[f"r{i}"] for i in range(len(PROMPTS))]


@pytest.fixture
def fused_hits(monkeypatch):
    """Counts the linear_silu_mul calls that take the fused kernel."""
    hits, inner = [], ops.fused_glu_config

    def spy(x, w):
        hit = inner(x, w)
        if hit is not None:
            hits.append(hit)
        return hit

    monkeypatch.setattr(ops, "fused_glu_config", spy)
    return hits


def test_engine_tokens_do_not_depend_on_the_switch(fused_hits):
    ops.set_fused_glu(True)
    on = _generate(_engine(weight_dtype="fp8"))
    assert fused_hits and {h[0] for h in fused_hits} == {"fp8_skinny_gemm"}
    n = len(fused_hits)
    ops.set_fused_glu(False)
    off = _generate(_engine(weight_dtype="fp8"))
    assert len(fused_hits) == n
    assert on == off and all(len(t) == 8 for t in on)


def test_static_lora_on_gate_up_keeps_two_kernels(monkeypatch):
    """With an adapter on gate_up the delta lands before the activation, so
    the MLP must not ask for the fused form at all."""
    calls = []
    inner = ops.linear_silu_mul
    monkeypatch.setattr(ops, "linear_silu_mul",
                        lambda x, w: calls.append(1) or inner(x, w))

    def run(switch):
        ops.set_fused_glu(switch)
        eng = _engine()
        eng.load_lora("a", rank=8, seed=3)
        assert "gate_up" in eng.runner.model.layers[0].mlp.lora
        return _generate(eng)

    on = run(True)
    assert not calls
    assert on == run(False) and all(len(t) == 8 for t in on)
    # without the adapter the same engine does ask for it
    ops.set_fused_glu(True)
    base = _generate(_engine())
    assert calls and base != on


def test_mlp_takes_the_fused_kernel_only_without_an_adapter(monkeypatch,
                                                             fused_hits):
    """SwiGLUMLP at a size the bf16 in-tree kernel takes (K = 2048)."""
    import dataclasses
    from dynamo_amd.models.layers import SwiGLUMLP, TPContext
    cfg = dataclasses.replace(PRESETS["tiny-llama-gpu"], hidden_size=2048,
                              intermediate_size=48)
    torch.manual_seed(11)
    mlp = SwiGLUMLP(cfg, TPContext(), DEV, torch.bfloat16)
    monkeypatch.setattr(ops, "SKINNY_GEMM_SHAPES",
                        {(96, 2048): (1, 2, 2, True, True)})
    x64, _ = _case("bf16_coalesced", 2048, 48)
    x = x64[:16]
    with torch.no_grad():
        fused = mlp(x)
        assert len(fused_hits) == 1
        ops.set_fused_glu(False)
        assert torch.equal(fused, mlp(x))
        ops.set_fused_glu(None)
        A = torch.randn(8, 2048, device=DEV).to(torch.bfloat16) * 0.1
        B = torch.randn(96, 8, device=DEV).to(torch.bfloat16) * 0.1
        mlp.lora = {"gate_up": (A, B, 2.0)}
        with_adapter = mlp(x)
        assert len(fused_hits) == 1
        gu = ops.linear(x, mlp.w_gate_up) + F.linear(F.linear(x, A), B) * 2.0
        expect = ops.linear(ops.silu_mul(gu), mlp.w_down)
        assert torch.equal(with_adapter, expect)
        assert not torch.equal(with_adapter, fused)
