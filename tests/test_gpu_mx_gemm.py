"""The W8A8 / W4A8 prefill GEMM (csrc/mx_gemm.hip) on the GPU: the activation
quantiser against its Python definition, the kernel at every launchable point,
its opt-in dispatch (ops.set_mx_gemm) and an engine that runs on it.

Inputs are seeded as in test_gpu_quant_tile_gemm.py: x ~ N(0, 1) in bf16,
W ~ N(0, 0.02) quantised by the project's quantisers. xd is x through
quantize_mxfp8_rows and back, W_exact is q * scale (fp8) or effective()
(mxfp4), ref = xd.double() @ W_exact.double().T, and the criterion is the
project's own: max|kernel - ref| <= 2 * max|lib - ref|, lib = fp32 F.linear on
(xd, W_exact) rounded once to bf16.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS
from dynamo_amd.ops import (Fp8Weight, Mxfp4Weight, dequantize_mxfp8_rows,
                            quantize_fp8_rowwise, quantize_mxfp4,
                            quantize_mxfp8_rows)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FMTS = ("fp8", "mxfp4")
HOLDER = {"fp8": Fp8Weight, "mxfp4": Mxfp4Weight}
PATH = {"fp8": ops.fp8_linear_path, "mxfp4": ops.mxfp4_linear_path}
POINTS = [(f, p) for f in FMTS for p in ops.MX_GEMM_CONFIGS[f]]
BM0 = ops.MX_GEMM_POINTS[0][0]


def _weight(fmt, w):
    if fmt == "fp8":
        q, scale = quantize_fp8_rowwise(w)
        return q, scale, q.double() * scale.double()[:, None]
    q, scale = quantize_mxfp4(w)
    return q, scale, Mxfp4Weight(q, scale).effective(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def _case(fmt, K, N):
    """Seeded (x bf16 [512, K], xq, xs, xd float64, q, scale, W_exact float64
    [N, K], ref float64 [512, N]); read-only."""
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 * K + N)
    x = torch.randn(512, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    xq, xs = quantize_mxfp8_rows(x)
    xd = dequantize_mxfp8_rows(xq, xs, torch.float64)
    q, scale, wx = _weight(fmt, w)
    return x, xq, xs, xd, q, scale, wx, xd @ wx.T


def _kernel(fmt, xq, xs, q, scale, point, glu=False):
    N = q.shape[0] // 2 if glu else q.shape[0]
    y = torch.empty(xq.shape[0], N, dtype=torch.bfloat16, device=DEV)
    getattr(ops.hip(), f"{fmt}_mx_gemm")(y, xq.contiguous(), xs.contiguous(),
                                         q, scale, *point, glu)
    return y


@pytest.mark.parametrize("K", [128, 1536])
@pytest.mark.parametrize("M", [1, 257])
def test_quantise_kernel_has_the_python_bytes(M, K):
    g = torch.Generator(device=DEV)
    g.manual_seed(M + K)
    x = torch.randn(M, K, generator=g, device=DEV)
    x[0, :32] = 0
    x[0, 32:64] *= 2.0 ** 20
    x[0, 64:96] *= 2.0 ** -20
    x[0, 97:128:2] *= 2.0 ** -12        # e4m3 subnormals and zeros
    if M > 1:
        x[3] = 0
        x[5] *= 2.0 ** 20
        x[7] *= 2.0 ** -20
    x = x.to(torch.bfloat16)
    xq = torch.empty(M, K, dtype=torch.float8_e4m3fn, device=DEV)
    xs = torch.empty(M, K // 32, dtype=torch.uint8, device=DEV)
    ops.hip().mxfp8_quantize_rows(xq, xs, x)
    want_q, want_s = quantize_mxfp8_rows(x)
    assert torch.equal(xs, want_s)
    assert torch.equal(xq.view(torch.uint8), want_q.view(torch.uint8))


def _check_against_reference(fmt, M, K, N, point):
    _, xq, xs, xd, q, scale, wx, refs = _case(fmt, K, N)
    ref = refs[:M]
    lib = F.linear(xd[:M].float(), wx.float()).to(torch.bfloat16)
    e_lib = (lib.double() - ref).abs().max().item()
    y = _kernel(fmt, xq[:M], xs[:M], q, scale, point)
    e_new = (y.double() - ref).abs().max().item()
    print(f"{fmt} M={M} K={K} N={N} {point}: e_lib={e_lib:.6g} "
          f"e_new={e_new:.6g} ratio={e_new / e_lib:.3f}")
    assert e_new <= 2 * e_lib


@pytest.mark.parametrize("M", [1, 17, 257, BM0 + 1, 2 * BM0])
@pytest.mark.parametrize("K,N", [(128, 48), (256, 48), (1536, 1040)])
@pytest.mark.parametrize("fmt", FMTS)
def test_matches_reference(fmt, K, N, M):
    _check_against_reference(fmt, M, K, N, ops.MX_GEMM_CONFIGS[fmt][0])


@pytest.mark.parametrize("fmt,point", POINTS)
def test_every_point(fmt, point):
    # smallest K, a ragged column block and a ragged second M tile
    _check_against_reference(fmt, point[0] + 1, ops.MX_GEMM_KSTEP,
                             point[1] + 16, point)


def test_tables_agree():
    launchable = ops.hip().mx_gemm_configs()
    for fmt in FMTS:
        assert sorted(launchable[fmt]) == sorted(ops.MX_GEMM_CONFIGS[fmt])


@pytest.mark.parametrize("fmt,point", POINTS)
def test_exact_layout_probe(fmt, point):
    """One nonzero 2^(m % 5) per x row at k_m = (2 m + j) % K: every k falls
    in every M tile over the two launches, rows quantise exactly, and
    y[m, n] must be bf16(W_exact[n, k_m] * 2^(m % 5))."""
    K, N, M = 256, 48, 2 * point[0]
    _, _, _, _, q, scale, wx, _ = _case(fmt, K, N)
    rows = torch.arange(M, device=DEV)
    val = (2.0 ** (rows % 5)).float()
    for j in range(2):
        ks = (2 * rows + j) % K
        x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        x[rows, ks] = val.to(torch.bfloat16)
        xq, xs = quantize_mxfp8_rows(x)
        assert torch.equal(dequantize_mxfp8_rows(xq, xs, torch.bfloat16), x)
        if fmt == "fp8":    # the kernel's own fp32 product, rounded once
            expect = ((q.float()[:, ks].T * val[:, None])
                      * scale[None, :]).to(torch.bfloat16)
        else:
            expect = (wx[:, ks].T * val[:, None].double()).to(torch.bfloat16)
        assert torch.equal(_kernel(fmt, xq, xs, q, scale, point), expect)


@pytest.mark.parametrize("fmt,point", POINTS)
def test_rows_do_not_depend_on_m(fmt, point):
    _, xq, xs, _, q, scale, _, _ = _case(fmt, 1536, 1040)
    M = 512    # 2 BM or 4 BM; 257 ends one row into an M tile of every BM
    big = _kernel(fmt, xq[:M], xs[:M], q, scale, point)
    assert torch.equal(big[:257], _kernel(fmt, xq[:257], xs[:257], q, scale,
                                          point))
    assert torch.equal(big, _kernel(fmt, xq[:M], xs[:M], q, scale, point))


@pytest.mark.parametrize("fmt,point", POINTS)
def test_glu_has_the_bits_of_silu_mul(fmt, point):
    _, xq, xs, _, q, scale, _, _ = _case(fmt, 1536, 1040 - 16)  # N % 32 == 0
    plain = _kernel(fmt, xq[:257], xs[:257], q, scale, point)
    assert torch.equal(_kernel(fmt, xq[:257], xs[:257], q, scale, point, True),
                       ops.silu_mul(plain))


@pytest.mark.parametrize("fmt", FMTS)
def test_dispatch(fmt, monkeypatch):
    x, _, _, _, q, scale, _, _ = _case(fmt, 256, 48)
    w = HOLDER[fmt](q, scale)
    lo = ops.MX_GEMM_MIN_M[fmt]
    monkeypatch.delenv("DYNAMO_MX_GEMM", raising=False)
    monkeypatch.setattr(ops, "_mx_gemm_override", None)
    monkeypatch.setattr(ops, "_tile_gemm_override", False)
    assert not ops.mx_gemm_enabled()
    assert PATH[fmt](x[:257], w) == ("dequant", None)
    ops.set_mx_gemm(True)
    point = ops.mx_gemm_config(fmt, lo, 48, 256)
    assert PATH[fmt](x[:lo], w) == ("mx", point)
    xq = torch.empty(lo, 256, dtype=torch.float8_e4m3fn, device=DEV)
    xs = torch.empty(lo, 8, dtype=torch.uint8, device=DEV)
    ops.hip().mxfp8_quantize_rows(xq, xs, x[:lo])
    assert torch.equal(ops.linear(x[:lo], w),
                       _kernel(fmt, xq, xs, q, scale, point))
    assert PATH[fmt](x[:lo - 1], w)[0] != "mx"
    wide = torch.zeros(lo, 512, dtype=torch.bfloat16, device=DEV)[:, :256]
    assert PATH[fmt](wide, w) == ("dequant", None)
    w288 = HOLDER[fmt].from_tensor(
        torch.ones(48, 288, dtype=torch.bfloat16, device=DEV))
    x288 = torch.zeros(lo, 288, dtype=torch.bfloat16, device=DEV)
    assert PATH[fmt](x288, w288) == ("dequant", None)


@pytest.mark.parametrize("fmt", FMTS)
def test_binding_rejects_what_the_kernel_cannot_do(fmt):
    x, xq, xs, _, q, scale, _, _ = _case(fmt, 256, 48)
    gemm = getattr(ops.hip(), f"{fmt}_mx_gemm")
    point = ops.MX_GEMM_CONFIGS[fmt][0]

    def y(M, N, dtype=torch.bfloat16):
        return torch.empty(M, N, dtype=dtype, device=DEV)

    with pytest.raises(RuntimeError):   # fp16 x
        ops.hip().mxfp8_quantize_rows(xq[:65].contiguous(),
                                      xs[:65].contiguous(),
                                      x[:65].to(torch.float16))
    with pytest.raises(RuntimeError):   # fp16 y
        gemm(y(65, 48, torch.float16), xq[:65], xs[:65], q, scale, *point)
    with pytest.raises(RuntimeError):   # N = 40
        gemm(y(65, 40), xq[:65], xs[:65], q[:40].contiguous(),
             scale[:40].contiguous(), *point)
    with pytest.raises(RuntimeError):   # unknown point
        gemm(y(65, 48), xq[:65], xs[:65], q, scale, 96, 128, 2, 2)
    w192 = HOLDER[fmt].from_tensor(
        torch.ones(48, 192, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError):   # K = 192 is no multiple of 128
        gemm(y(65, 48), xq[:65, :192].contiguous(),
             xs[:65, :6].contiguous(), w192.q, w192.scale, *point)


# ---- engine -------------------------------------------------------------
PROJ = (("attn", "wqkv"), ("attn", "wo"), ("mlp", "w_gate_up"),
        ("mlp", "w_down"))
PROMPTS = [[100 + i % 700 for i in range(300)], [7, 8, 9] * 10]


def _generate(fmt, **kw):
    cfg = EngineConfig(model=PRESETS["tiny-llama-gpu"], device=DEV,
                       max_num_seqs=8, max_batched_tokens=512,
                       max_model_len=2048, page_size=64, kv_pool_pages=256,
                       weight_dtype=fmt, **kw)
    engine = LLMEngine(cfg, seed=7)
    for layer in engine.runner.model.layers:
        for sub, name in PROJ:
            w = getattr(getattr(layer, sub), name)
            x = torch.zeros(300, w.shape[1], dtype=torch.bfloat16, device=DEV)
            assert PATH[fmt](x, w)[0] == "mx"
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
def test_engine_on_the_mx_kernel(fmt, monkeypatch):
    monkeypatch.setattr(ops, "_mx_gemm_override", True)
    tokens = _generate(fmt)
    assert all(len(t) == 8 for t in tokens)
    assert _generate(fmt) == tokens
    assert _generate(fmt, enable_hip_graphs=False) == tokens
