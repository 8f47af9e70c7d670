"""The tiled W8A16 / W4A16 GEMM (csrc/quant_tile_gemm.hip) on the GPU: the
kernel at every launchable point, its opt-in dispatch (ops.set_tile_gemm) and
an engine that runs on it.

Inputs are seeded: x ~ N(0, 1) in bf16, W ~ N(0, 0.02) quantised by the
project's quantisers. W_exact is q * scale (fp8) or effective() (mxfp4) and
ref = x.double() @ W_exact.double().T. The accuracy criterion is the one
tests/test_gpu_fp8_weights.py argues, with no fixed tolerance:
max|kernel - ref| <= 2 * max|lib - ref|, lib = fp32 F.linear on W_exact
rounded once to bf16.
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
FMTS = ("fp8", "mxfp4")
HOLDER = {"fp8": Fp8Weight, "mxfp4": Mxfp4Weight}
PATH = {"fp8": ops.fp8_linear_path, "mxfp4": ops.mxfp4_linear_path}
SKINNY_MAX = {"fp8": ops.FP8_GEMM_MAX_M, "mxfp4": ops.MXFP4_GEMM_MAX_M}
POINTS = [(f, p) for f in FMTS for p in ops.TILE_GEMM_CONFIGS[f]]


def _kstep(fmt, p):
    return p[2] * ops.TILE_GEMM_KSTEP[fmt] * p[4]


@functools.lru_cache(maxsize=None)
def _case(fmt, K, N):
    """Seeded (x [256, K], q, scale, W_exact float64 [N, K], ref [256, N]
    float64); read-only."""
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 * K + N)
    x = torch.randn(256, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    if fmt == "fp8":
        q, scale = quantize_fp8_rowwise(w)
        wx = q.double() * scale.double()[:, None]
    else:
        q, scale = quantize_mxfp4(w)
        wx = Mxfp4Weight(q, scale).effective(torch.bfloat16).double()
    return x, q, scale, wx, x.double() @ wx.T


def _kernel(fmt, x, q, scale, point, glu=False):
    N = q.shape[0] // 2 if glu else q.shape[0]
    y = torch.empty(x.shape[0], N, dtype=torch.bfloat16, device=x.device)
    getattr(ops.hip(), f"{fmt}_tile_gemm")(y, x, q, scale, *point, glu)
    return y


def _check_against_reference(fmt, M, K, N, point):
    xs, q, scale, wx, refs = _case(fmt, K, N)
    x, ref = xs[:M], refs[:M]
    lib = F.linear(x.float(), wx.float()).to(torch.bfloat16)
    e_lib = (lib.double() - ref).abs().max().item()
    e_new = (_kernel(fmt, x, q, scale, point).double() - ref).abs().max().item()
    print(f"{fmt} M={M} K={K} N={N} {point}: e_lib={e_lib:.6g} "
          f"e_new={e_new:.6g}")
    assert e_new <= 2 * e_lib


@pytest.mark.parametrize("M", [17, 64, 65, 129, 200])
@pytest.mark.parametrize("K,N", [(512, 48), (1536, 1040)])
@pytest.mark.parametrize("fmt", FMTS)
def test_matches_reference(fmt, K, N, M):
    point = ops.TILE_GEMM_CONFIGS[fmt][0]
    assert _kstep(fmt, point) == ops.TILE_GEMM_KSTEP[fmt]   # takes every K
    _check_against_reference(fmt, M, K, N, point)


@pytest.mark.parametrize("fmt,point", POINTS)
def test_every_point(fmt, point):
    # smallest eligible K, a ragged column block and a ragged second M tile
    _check_against_reference(fmt, point[0] + 1, _kstep(fmt, point),
                             point[1] * point[3] * 16 + 16, point)


def test_tables_agree():
    launchable = ops.hip().tile_gemm_configs()
    for fmt in FMTS:
        assert sorted(launchable[fmt]) == sorted(ops.TILE_GEMM_CONFIGS[fmt])


@pytest.mark.parametrize("fmt,point", POINTS)
def test_exact_layout_probe(fmt, point):
    """One-hot rows of x: y[m, n] must be bf16(W_exact[n, k_m]), and the
    launches put every k in both M tiles."""
    K, N, M = 512, 48, 2 * point[0]
    _, q, scale, wx, _ = _case(fmt, K, N)
    rows = torch.arange(M, device=DEV)
    for j in range(K // M):
        ks = (rows * (K // M) + j) % K
        x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        x[rows, ks] = 1.0
        if fmt == "fp8":    # the kernel's own fp32 product, rounded once
            expect = (q.float()[:, ks].T * scale[None, :]).to(torch.bfloat16)
        else:
            expect = wx[:, ks].T.to(torch.bfloat16)
        y = _kernel(fmt, x, q, scale, point)
        assert torch.equal(y, expect)
        nz = expect != 0
        assert torch.equal(y.view(torch.int16)[nz],
                           expect.view(torch.int16)[nz])


@pytest.mark.parametrize("fmt,point", POINTS)
def test_rows_do_not_depend_on_m(fmt, point):
    x, q, scale, _, _ = _case(fmt, 1536, 1040)
    y200 = _kernel(fmt, x[:200], q, scale, point)
    assert torch.equal(y200[:65], _kernel(fmt, x[:65], q, scale, point))
    assert torch.equal(y200, _kernel(fmt, x[:200], q, scale, point))
    if point[2] == 1:   # WK = 1: the skinny kernel's order of sums at WPB = 1
        m = SKINNY_MAX[fmt]
        ys = torch.empty(m, 1040, dtype=torch.bfloat16, device=DEV)
        getattr(ops.hip(), f"{fmt}_skinny_gemm")(ys, x[:m], q, scale, 1, 1, 2)
        assert torch.equal(_kernel(fmt, x[:m], q, scale, point), ys)


@pytest.mark.parametrize("fmt,point", POINTS)
def test_glu_has_the_bits_of_silu_mul(fmt, point):
    x, q, scale, _, _ = _case(fmt, 1536, 1040 - 16)   # N % 32 == 0
    plain = _kernel(fmt, x[:65], q, scale, point)
    assert torch.equal(_kernel(fmt, x[:65], q, scale, point, glu=True),
                       ops.silu_mul(plain))


@pytest.mark.parametrize("fmt", FMTS)
def test_dispatch(fmt, monkeypatch):
    x, q, scale, _, _ = _case(fmt, 512, 48)
    w = HOLDER[fmt](q, scale)
    M = SKINNY_MAX[fmt] + 1
    monkeypatch.delenv("DYNAMO_QUANT_TILE_GEMM", raising=False)
    monkeypatch.setattr(ops, "_tile_gemm_override", None)
    assert not ops.tile_gemm_enabled()
    assert PATH[fmt](x[:M], w) == ("dequant", None)
    ops.set_tile_gemm(True)
    point = ops.tile_gemm_config(fmt, M, 48, 512)
    assert PATH[fmt](x[:M], w) == ("tile", point)
    assert torch.equal(ops.linear(x[:M], w),
                       _kernel(fmt, x[:M], q, scale, point))
    for m in range(1, ops.TILE_GEMM_MAX_M[fmt] + 1):
        assert PATH[fmt](x[:1].expand(m, 512).contiguous(), w)[0] in (
            "kernel", "tile")
    big = torch.zeros(ops.TILE_GEMM_MAX_M[fmt] + 1, 512, dtype=torch.bfloat16,
                      device=DEV)
    assert PATH[fmt](big, w) == ("dequant", None)
    wide = torch.zeros(M, 1024, dtype=torch.bfloat16, device=DEV)[:, :512]
    assert PATH[fmt](wide, w) == ("dequant", None)
    w288 = HOLDER[fmt].from_tensor(
        torch.ones(48, 288, dtype=torch.bfloat16, device=DEV))
    x288 = torch.zeros(M, 288, dtype=torch.bfloat16, device=DEV)
    assert PATH[fmt](x288, w288) == ("dequant", None)


@pytest.mark.parametrize("fmt", FMTS)
def test_binding_rejects_what_the_kernel_cannot_do(fmt):
    x, q, scale, _, _ = _case(fmt, 512, 48)
    gemm = getattr(ops.hip(), f"{fmt}_tile_gemm")
    point = ops.TILE_GEMM_CONFIGS[fmt][0]

    def y(M, N, dtype=torch.bfloat16):
        return torch.empty(M, N, dtype=dtype, device=DEV)

    with pytest.raises(RuntimeError):   # fp16 x
        gemm(y(65, 48, torch.float16), x[:65].to(torch.float16), q, scale,
             *point)
    with pytest.raises(RuntimeError):   # N = 40
        gemm(y(65, 40), x[:65], q[:40].contiguous(), scale[:40].contiguous(),
             *point)
    with pytest.raises(RuntimeError):   # unknown point
        gemm(y(65, 48), x[:65], q, scale, 96, 4, 1, 2, 1)
    x, q, scale, _, _ = _case(fmt, 768, 48)
    wide = next(p for p in ops.TILE_GEMM_CONFIGS[fmt] if 768 % _kstep(fmt, p))
    with pytest.raises(RuntimeError):   # K = 768 is no multiple of its step
        gemm(y(65, 48), x[:65], q, scale, *wide)


# ---- engine -------------------------------------------------------------
PROJ = (("attn", "wqkv"), ("attn", "wo"), ("mlp", "w_gate_up"),
        ("mlp", "w_down"))
PROMPTS = [list(range(100, 180)), [7, 8, 9] * 10]


def _generate(fmt, **kw):
    cfg = EngineConfig(model=PRESETS["tiny-llama-gpu"], device=DEV,
                       max_num_seqs=8, max_batched_tokens=512,
                       max_model_len=2048, page_size=64, kv_pool_pages=256,
                       weight_dtype=fmt, **kw)
    engine = LLMEngine(cfg, seed=7)
    for layer in engine.runner.model.layers:
        for sub, name in PROJ:
            w = getattr(getattr(layer, sub), name)
            x = torch.zeros(80, w.shape[1], dtype=torch.bfloat16, device=DEV)
            assert PATH[fmt](x, w)[0] == "tile"
    outs = {f"r{i}": [] for i in range(len(PROMPTS))}
    for i, p in enumerate(PROMPTS):
        engine.add_request(f"r{i}", p, SamplingParams(max_tokens=8))
    steps = 0
    while engine.has_work():
        for so in engine.step():
            outs[so.req_id].append(so.new_token)
        steps += 1
        assert steps < 1000
    return [outs[f"r{i}"] for i in range(len(PROMPTS))]


@pytest.mark.parametrize("fmt", FMTS)
def test_engine_on_the_tiled_kernel(fmt, monkeypatch):
    monkeypatch.setattr(ops, "_tile_gemm_override", True)
    tokens = _generate(fmt)
    assert all(len(t) == 8 for t in tokens)
    assert _generate(fmt) == tokens
    assert _generate(fmt, enable_hip_graphs=False) == tokens
