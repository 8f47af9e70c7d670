"""FP8 (e4m3) weights on the GPU: the W8A16 decode GEMM and the dequantise
kernel (csrc/skinny_gemm_impl.h), their dispatch (ops.linear with an
Fp8Weight) and an engine built with weight_dtype="fp8".

Inputs are seeded: x ~ N(0, 1) in bf16, W ~ N(0, 0.02) quantised by the
project's quantiser. The accuracy criterion has no fixed tolerance: with
ref = (x.double() @ q.double().T) * scale.double(), e_new = max|kernel - ref|
must not exceed 2 * e_lib, where e_lib is the same error of
(F.linear(x.float(), q.float()) * scale).to(bf16). Both sides round one fp32
sum to bf16; a differently ordered fp32 sum can land across one rounding
boundary (the argument of tests/test_gpu_skinny_gemm.py).

The exact probes compare values with torch.equal and bit patterns wherever
the expected value is not zero: a sum of products that are all +-0 is +0 in
any fp32 accumulation, so the code -0 comes out as +0.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS
from dynamo_amd.ops import Fp8Weight, quantize_fp8_rowwise

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEFAULT = ops.FP8_GEMM_DEFAULT


@functools.lru_cache(maxsize=None)
def _case(K, N):
    """Seeded (x64 [64, K], q [N, K], scale [N], ref [64, N] float64);
    read-only."""
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 * K + N)
    x = torch.randn(64, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    q, scale = quantize_fp8_rowwise(w)
    ref = (x.double() @ q.double().T) * scale.double()
    return x, q, scale, ref


def _kernel(x, q, scale, cfg=DEFAULT, y=None):
    if y is None:
        y = torch.empty(x.shape[0], q.shape[0], dtype=torch.bfloat16,
                        device=x.device)
    ops.hip().fp8_skinny_gemm(y, x, q, scale, *cfg)
    return y


def _check_against_reference(M, K, N, cfg):
    x64, q, scale, ref64 = _case(K, N)
    x, ref = x64[:M], ref64[:M]
    lib = (F.linear(x.float(), q.float()) * scale).to(torch.bfloat16)
    e_lib = (lib.double() - ref).abs().max().item()
    e_new = (_kernel(x, q, scale, cfg).double() - ref).abs().max().item()
    print(f"M={M} K={K} N={N} cfg={cfg}: e_lib={e_lib:.6g} e_new={e_new:.6g}")
    assert e_new <= 2 * e_lib


SHAPES = [(512, 16), (512, 48), (1536, 1040), (28672, 48)]


@pytest.mark.parametrize("M", [1, 3, 16, 17, 33, 64])
@pytest.mark.parametrize("K,N", SHAPES)
def test_matches_reference(M, K, N):
    _check_against_reference(M, K, N, DEFAULT)


def _kstep(cfg):
    return cfg[0] * 128 * cfg[1]


@pytest.mark.parametrize("M", [16, 64])
@pytest.mark.parametrize("cfg", ops.FP8_GEMM_CONFIGS)
def test_every_configuration(cfg, M):
    # smallest eligible K; smallest N that fills one block (NT tiles) plus a
    # ragged group (1 tile)
    _check_against_reference(M, _kstep(cfg), cfg[2] * 16 + 16, cfg)


def test_default_is_launchable_and_takes_every_k():
    launchable = ops.hip().skinny_gemm_configs()["fp8"]
    assert len(launchable) == len(ops.FP8_GEMM_CONFIGS)
    assert set(launchable) == set(ops.FP8_GEMM_CONFIGS)
    assert DEFAULT in ops.FP8_GEMM_CONFIGS
    assert _kstep(DEFAULT) == 128
    assert ops.FP8_GEMM_SPLIT_K in ops.FP8_GEMM_CONFIGS
    for (N, K), cfgs in ops.FP8_GEMM_SHAPES.items():
        for cfg in cfgs:
            assert cfg in ops.FP8_GEMM_CONFIGS
            assert K % _kstep(cfg) == 0 and N % 16 == 0
        assert ops.fp8_gemm_config(16, N, K) == cfgs[0]
        assert ops.fp8_gemm_config(17, N, K) == cfgs[1]
        assert ops.fp8_gemm_config(64, N, K) == cfgs[1]
        assert ops.fp8_gemm_config(65, N, K) is None
    # outside the table: the K split where K allows, else the default
    assert ops.fp8_gemm_config(16, 48, 512) == ops.FP8_GEMM_SPLIT_K
    assert ops.fp8_gemm_config(16, 48, 384) == DEFAULT
    assert ops.fp8_gemm_config(16, 40, 512) is None
    assert ops.fp8_gemm_config(16, 48, 520) is None
    _check_against_reference(16, 128, 48, DEFAULT)
    _check_against_reference(64, 384, 48, DEFAULT)


def _bits(t):
    return t.view(torch.int16)


def _assert_exact(y, expect):
    assert torch.equal(y, expect)
    nz = expect != 0
    assert torch.equal(_bits(y)[nz], _bits(expect)[nz])


def _one_hot_probe(q, scale, cfg):
    """y[m, n] for one-hot rows of x must be bf16(float(q[n, k_m]) *
    scale[n]); eight launches of 64 rows cover every k of K = 512."""
    N, K = q.shape
    qf = q.float()
    for j in range(K // 64):
        ks = torch.arange(64, device=DEV) * (K // 64) + j   # k of row m
        x = torch.zeros(64, K, dtype=torch.bfloat16, device=DEV)
        x[torch.arange(64, device=DEV), ks] = 1.0
        expect = (qf[:, ks].T * scale[None, :]).to(torch.bfloat16)
        _assert_exact(_kernel(x, q, scale, cfg), expect)


@pytest.mark.parametrize("cfg", [DEFAULT, (4, 1, 2), (1, 2, 2)])
def test_exact_layout_probe(cfg):
    _, q, scale, _ = _case(512, 48)
    _one_hot_probe(q, scale, cfg)


def test_exact_all_codes():
    """A W whose rows together hold all 254 finite e4m3 codes, -0 and the
    subnormals included, with scale 1: every code converts exactly."""
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F],
                         dtype=torch.uint8, device=DEV)
    assert codes.numel() == 254
    n = torch.arange(48, device=DEV)[:, None]
    k = torch.arange(512, device=DEV)[None, :]
    q = codes[(n * 7 + k) % 254].view(torch.float8_e4m3fn).contiguous()
    assert torch.isfinite(q.float()).all()
    assert q.view(torch.uint8).unique().numel() == 254
    _one_hot_probe(q, torch.ones(48, device=DEV), DEFAULT)


def test_scale_is_per_column():
    x64, q, _, _ = _case(512, 48)
    ones = torch.ones(48, device=DEV)
    scale = 2.0 ** -(1.0 + (torch.arange(48, device=DEV) % 8).float())
    assert scale.unique().numel() == 8
    assert scale.min() == 2.0 ** -8 and scale.max() == 2.0 ** -1
    for M in (16, 64):
        y1 = _kernel(x64[:M], q, ones)
        ys = _kernel(x64[:M], q, scale)
        assert torch.equal(ys, (y1.float() * scale[None, :]).to(torch.bfloat16))


@pytest.mark.parametrize("cfg", ops.FP8_GEMM_CONFIGS)
def test_batch_invariant_and_deterministic(cfg):
    # K = 3 k-steps of the configuration: the main loop runs
    K, N = 3 * _kstep(cfg), cfg[2] * 16 + 16
    x64, q, scale, _ = _case(K, N)
    _check_against_reference(64, K, N, cfg)
    y64 = _kernel(x64, q, scale, cfg)
    assert torch.equal(y64, _kernel(x64, q, scale, cfg))
    for m in (0, 7, 15, 16, 63):
        y1 = _kernel(x64[m:m + 1], q, scale, cfg)
        assert torch.equal(y1[0], y64[m]), f"row {m} depends on M"
    # two and three accumulator tiles per column tile
    for M in (17, 33, 48):
        assert torch.equal(_kernel(x64[:M], q, scale, cfg), y64[:M]), \
            f"M = {M} differs from the M = 64 run"


@pytest.mark.parametrize("M", [1, 3, 17])
def test_writes_only_y(M):
    x64, q, scale, _ = _case(512, 48)
    N, pad = 48, 4096
    buf = torch.full((pad + M * N + pad,), 0x7B7B, dtype=torch.int16,
                     device=DEV)
    y = buf[pad:pad + M * N].view(torch.bfloat16).view(M, N)
    _kernel(x64[:M], q, scale, y=y)
    torch.cuda.synchronize()
    assert (buf[:pad] == 0x7B7B).all() and (buf[pad + M * N:] == 0x7B7B).all()
    assert torch.equal(y, _kernel(x64[:M], q, scale))


@pytest.mark.parametrize("M", [1, 3, 17])
def test_reads_only_the_first_m_rows(M):
    x64, q, scale, _ = _case(512, 48)
    xbuf = torch.full_like(x64, float("nan"))
    xbuf[:M] = x64[:M]
    y = _kernel(xbuf[:M], q, scale)
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y, _kernel(x64[:M].contiguous(), q, scale))


@pytest.mark.parametrize("N,K", [(1, 16), (37, 528), (1040, 1536)])
def test_dequant(N, K):
    g = torch.Generator(device=DEV)
    g.manual_seed(N * 10000 + K)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    q, scale = quantize_fp8_rowwise(w)
    pad = 1024
    buf = torch.full((pad + N * K + pad,), 0x7B7B, dtype=torch.int16,
                     device=DEV)
    out = buf[pad:pad + N * K].view(torch.bfloat16).view(N, K)
    ops.hip().fp8_dequant(out, q, scale)
    torch.cuda.synchronize()
    assert torch.equal(out, (q.float() * scale[:, None]).to(torch.bfloat16))
    assert (buf[:pad] == 0x7B7B).all() and (buf[pad + N * K:] == 0x7B7B).all()


# ---- dispatch ---------------------------------------------------------
def _rand(*shape, seed, dtype=torch.bfloat16, std=1.0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * std).to(dtype)


def test_dispatch_takes_kernel_when_eligible():
    x64, q, scale, _ = _case(512, 48)
    w = Fp8Weight(q, scale)
    cfg = ops.FP8_GEMM_SPLIT_K          # K = 512 allows the 4-wave K split
    assert ops.fp8_linear_path(x64, w) == ("kernel", cfg)
    assert torch.equal(ops.linear(x64, w), _kernel(x64, q, scale, cfg))
    assert ops.fp8_linear_path(x64[:1], w) == ("kernel", cfg)
    assert torch.equal(ops.linear(x64[:1], w),
                       _kernel(x64[:1], q, scale, cfg))
    # K = 384 does not: the default configuration
    x, q2, scale2, _ = _case(384, 48)
    w2 = Fp8Weight(q2, scale2)
    assert ops.fp8_linear_path(x, w2) == ("kernel", DEFAULT)
    assert torch.equal(ops.linear(x, w2), _kernel(x, q2, scale2, DEFAULT))


def _other_calls():
    _, q, scale, _ = _case(512, 48)
    w520 = Fp8Weight(*quantize_fp8_rowwise(_rand(48, 520, seed=3, std=0.02)))
    return {
        "M=65": (_rand(65, 512, seed=1), Fp8Weight(q, scale), "dequant"),
        "K=520": (_rand(16, 520, seed=2), w520, "torch"),
        "non-contiguous x": (_rand(16, 1024, seed=4)[:, :512],
                             Fp8Weight(q, scale), "dequant"),
    }


@pytest.mark.parametrize("case", ["M=65", "K=520", "non-contiguous x"])
def test_dispatch_other_calls_use_w_eff(case):
    x, w, path = _other_calls()[case]
    assert ops.fp8_linear_path(x, w) == (path, None)
    w_eff = (w.q.float() * w.scale[:, None]).to(torch.bfloat16)
    assert torch.equal(ops.linear(x, w), F.linear(x, w_eff))


def test_binding_rejects_what_the_kernel_cannot_do():
    x64, q, scale, _ = _case(512, 48)
    hip = ops.hip()

    def y(M, N, dtype=torch.bfloat16):
        return torch.empty(M, N, dtype=dtype, device=DEV)

    with pytest.raises(RuntimeError):   # M = 65
        hip.fp8_skinny_gemm(y(65, 48), _rand(65, 512, seed=1), q, scale,
                            *DEFAULT)
    with pytest.raises(RuntimeError):   # N = 40
        hip.fp8_skinny_gemm(y(16, 40), x64[:16], q[:40].contiguous(),
                            scale[:40].contiguous(), *DEFAULT)
    with pytest.raises(RuntimeError):   # fp16 x
        hip.fp8_skinny_gemm(y(16, 48, torch.float16),
                            x64[:16].to(torch.float16), q, scale, *DEFAULT)
    with pytest.raises(RuntimeError):   # unknown configuration
        hip.fp8_skinny_gemm(y(16, 48), x64[:16], q, scale, 3, 1, 2)
    with pytest.raises(RuntimeError):   # K = 512 is no multiple of 8*128
        hip.fp8_skinny_gemm(y(16, 48), x64[:16], q, scale, 8, 1, 2)


# ---- engine -------------------------------------------------------------
PROJ = (("attn", "wqkv"), ("attn", "wo"), ("mlp", "w_gate_up"),
        ("mlp", "w_down"))


def make_engine(**kw):
    kw.setdefault("kv_pool_pages", 256)
    kw.setdefault("weight_dtype", "fp8")
    cfg = EngineConfig(model=PRESETS["tiny-llama-gpu"], device="cuda:0",
                       max_num_seqs=8, max_batched_tokens=512,
                       max_model_len=2048, page_size=64, **kw)
    return LLMEngine(cfg, seed=7)


def generate(engine, prompts, max_tokens=8):
    outs = {}
    for i, p in enumerate(prompts):
        engine.add_request(f"r{i}", p, SamplingParams(max_tokens=max_tokens))
        outs[f"r{i}"] = []
    steps = 0
    while engine.has_work():
        for so in engine.step():
            outs[so.req_id].append(so.new_token)
        steps += 1
        assert steps < 1000
    return [outs[f"r{i}"] for i in range(len(prompts))]


PROMPTS = [list(range(100, 180)), [7, 8, 9] * 10]


@functools.lru_cache(maxsize=None)
def _fp8_tokens():
    return generate(make_engine(), PROMPTS)


def test_engine_two_builds_agree():
    o = generate(make_engine(), PROMPTS)
    assert o == _fp8_tokens()
    assert all(len(t) == 8 for t in o)


def test_engine_graphs_on_and_off_agree():
    assert generate(make_engine(enable_hip_graphs=False),
                    PROMPTS) == _fp8_tokens()


def test_engine_with_fp8_kv_cache():
    o = generate(make_engine(kv_cache_dtype="fp8"), PROMPTS)
    assert all(len(t) == 8 for t in o)


def test_engine_decode_shapes_take_the_kernel():
    eng = make_engine()
    for layer in eng.runner.model.layers:
        for sub, name in PROJ:
            w = getattr(getattr(layer, sub), name)
            assert isinstance(w, Fp8Weight)
            assert w.q.dtype == torch.float8_e4m3fn
            for M in (1, 8, 64):
                x = torch.zeros(M, w.shape[1], dtype=torch.bfloat16,
                                device=DEV)
                assert ops.fp8_linear_path(x, w)[0] == "kernel"
            x = torch.zeros(80, w.shape[1], dtype=torch.bfloat16, device=DEV)
            assert ops.fp8_linear_path(x, w) == ("dequant", None)


def test_engine_prefill_matches_w_eff_twin():
    """An 80-token prefill runs the dequantise path: the same library call
    on the same bits as an unquantised twin holding W_eff."""
    fp8 = make_engine(enable_hip_graphs=False)
    twin = make_engine(enable_hip_graphs=False, weight_dtype="bf16")
    for lf, lt in zip(fp8.runner.model.layers, twin.runner.model.layers):
        for sub, name in PROJ:
            h = getattr(getattr(lf, sub), name)
            with torch.no_grad():
                getattr(getattr(lt, sub), name).copy_(
                    h.effective(torch.bfloat16))
    prompt = [list(range(100, 180))]
    a = generate(fp8, prompt, max_tokens=1)
    b = generate(twin, prompt, max_tokens=1)
    assert a == b and len(a[0]) == 1
