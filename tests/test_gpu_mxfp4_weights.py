"""MXFP4 (e2m1 + e8m0) weights on the GPU: the W4A16 decode GEMM and the
dequantise kernel (csrc/skinny_gemm_impl.h), their dispatch (ops.linear with
an Mxfp4Weight) and an engine built with weight_dtype="mxfp4".

Inputs are seeded: x ~ N(0, 1) in bf16, W ~ N(0, 0.02) quantised by the
project's quantiser. The accuracy criterion has no fixed tolerance: with
ref = x.double() @ W_eff.double().T, e_new = max|kernel - ref| must not
exceed 2 * e_lib, where e_lib is the same error of
F.linear(x.float(), W_eff.float()).to(bf16). Both sides round one fp32 sum
to bf16; a differently ordered fp32 sum can land across one rounding
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
from dynamo_amd.ops import Mxfp4Weight, quantize_mxfp4

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEFAULT = ops.MXFP4_GEMM_DEFAULT
MAX_M = ops.MXFP4_GEMM_MAX_M


@functools.lru_cache(maxsize=None)
def _case(K, N):
    """Seeded (x [MAX_M, K], q, scale, W_eff bf16 [N, K], ref [MAX_M, N]
    float64); read-only."""
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 * K + N)
    x = torch.randn(MAX_M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    q, scale = quantize_mxfp4(w)
    w_eff = Mxfp4Weight(q, scale).effective(torch.bfloat16)
    ref = x.double() @ w_eff.double().T
    return x, q, scale, w_eff, ref


def _kernel(x, q, scale, cfg=DEFAULT, y=None):
    if y is None:
        y = torch.empty(x.shape[0], q.shape[0], dtype=torch.bfloat16,
                        device=x.device)
    ops.hip().mxfp4_skinny_gemm(y, x, q, scale, *cfg)
    return y


def _check_against_reference(M, K, N, cfg):
    xs, q, scale, w_eff, refs = _case(K, N)
    x, ref = xs[:M], refs[:M]
    lib = F.linear(x.float(), w_eff.float()).to(torch.bfloat16)
    e_lib = (lib.double() - ref).abs().max().item()
    e_new = (_kernel(x, q, scale, cfg).double() - ref).abs().max().item()
    print(f"M={M} K={K} N={N} cfg={cfg}: e_lib={e_lib:.6g} e_new={e_new:.6g}")
    assert e_new <= 2 * e_lib


SHAPES = [(256, 16), (512, 48), (1536, 1040), (28672, 48)]
MS = [1, 3, 16] + [m for m in (17, 33, 64) if m <= MAX_M]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K,N", SHAPES)
def test_matches_reference(M, K, N):
    _check_against_reference(M, K, N, DEFAULT)


def _kstep(cfg):
    return cfg[0] * 256 * cfg[1]


@pytest.mark.parametrize("M", sorted({16, MAX_M}))
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("cfg", ops.MXFP4_GEMM_CONFIGS)
def test_every_configuration(cfg, steps, M):
    # the smallest eligible K, and three k-steps so that the main loop runs;
    # the smallest N that fills one block (NT tiles) plus a ragged one
    _check_against_reference(M, steps * _kstep(cfg), cfg[2] * 16 + 16, cfg)


def test_tables_match_the_extension():
    launchable = ops.hip().skinny_gemm_configs()["mxfp4"]
    assert len(launchable) == len(ops.MXFP4_GEMM_CONFIGS)
    assert set(launchable) == set(ops.MXFP4_GEMM_CONFIGS)
    assert ops.hip().mxfp4_gemm_max_m() == MAX_M
    assert DEFAULT in ops.MXFP4_GEMM_CONFIGS
    assert _kstep(DEFAULT) == 256
    assert ops.MXFP4_GEMM_SPLIT_K in ops.MXFP4_GEMM_CONFIGS
    for (N, K), cfgs in ops.MXFP4_GEMM_SHAPES.items():
        for cfg in cfgs:
            assert cfg in ops.MXFP4_GEMM_CONFIGS
            assert K % _kstep(cfg) == 0 and N % 16 == 0
        assert ops.mxfp4_gemm_config(16, N, K) == cfgs[0]
        if MAX_M > 16:
            assert ops.mxfp4_gemm_config(17, N, K) == cfgs[1]
            assert ops.mxfp4_gemm_config(MAX_M, N, K) == cfgs[1]
        assert ops.mxfp4_gemm_config(MAX_M + 1, N, K) is None
    # the other formats' tables are what they were
    others = ops.hip().skinny_gemm_configs()
    assert set(others) == {"bf16_plain", "bf16_coalesced", "fp8", "mxfp4"}
    assert set(others["fp8"]) == set(ops.FP8_GEMM_CONFIGS)


def _bits(t):
    return t.view(torch.int16)


def _assert_exact(y, expect):
    assert torch.equal(y, expect)
    nz = expect != 0
    assert torch.equal(_bits(y)[nz], _bits(expect)[nz])


def _one_hot_probe(q, scale, cfg):
    """y[m, n] for one-hot rows of x must be bf16(W_eff[n, k_m]); K / MAX_M
    launches of MAX_M rows cover every k."""
    N, K = q.shape[0], q.shape[1] * 2
    w_eff = Mxfp4Weight(q, scale).effective(torch.bfloat16)
    rows = torch.arange(MAX_M, device=DEV)
    for j in range(K // MAX_M):
        ks = rows * (K // MAX_M) + j   # k of row m
        x = torch.zeros(MAX_M, K, dtype=torch.bfloat16, device=DEV)
        x[rows, ks] = 1.0
        _assert_exact(_kernel(x, q, scale, cfg), w_eff[:, ks].T.contiguous())


# the default, one K split and one U = 2 configuration
@pytest.mark.parametrize("cfg", [DEFAULT, (2, 1, 2), (1, 2, 2)])
def test_exact_layout_probe(cfg):
    assert cfg in ops.MXFP4_GEMM_CONFIGS
    _, q, scale, _, _ = _case(512, 48)
    _one_hot_probe(q, scale, cfg)


def test_exact_all_codes_and_scales():
    """A hand-built W: all 16 codes in each of the 8 nibble positions of a
    dword, scale bytes that change from block to block and include both ends
    of the quantiser's range (27, 227) and 127, and, for every row and
    256-k step, bytes c and c + 4 of the step's eight different from each
    other. Catches swapped nibbles, a swapped c / c + 4 scale and denormal
    handling."""
    N, K = 48, 512
    n = torch.arange(N, device=DEV)[:, None]
    k = torch.arange(K, device=DEV)[None, :]
    codes = ((n * 5 + k * 3 + k // 8) % 16).to(torch.uint8)
    for pos in range(8):
        assert codes[:, pos::8].unique().numel() == 16
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    table = torch.tensor([27, 127, 227, 120, 133, 100, 140],
                         dtype=torch.uint8, device=DEV)
    b = torch.arange(K // 32, device=DEV)[None, :]
    scale = table[(n + b) % 7].contiguous()
    s = scale.view(N, K // 256, 8)
    assert (s[:, :, :4] != s[:, :, 4:]).all()
    assert (scale[:, 1:] != scale[:, :-1]).all()
    assert {27, 127, 227} <= set(scale.unique().tolist())
    w_eff = Mxfp4Weight(q, scale).effective(torch.float32)
    assert w_eff.abs().max() == 6 * 2.0 ** 100
    assert w_eff[w_eff != 0].abs().min() == 2.0 ** -101
    _one_hot_probe(q, scale, DEFAULT)


@pytest.mark.parametrize("cfg", ops.MXFP4_GEMM_CONFIGS)
def test_batch_invariant_and_deterministic(cfg):
    # K = 3 k-steps of the configuration: the main loop runs
    K, N = 3 * _kstep(cfg), cfg[2] * 16 + 16
    xs, q, scale, _, _ = _case(K, N)
    full = _kernel(xs, q, scale, cfg)
    assert torch.equal(full, _kernel(xs, q, scale, cfg))
    for m in sorted({0, 7, 15, 16, MAX_M - 1}):
        y1 = _kernel(xs[m:m + 1], q, scale, cfg)
        assert torch.equal(y1[0], full[m]), f"row {m} depends on M"
    for M in (3, 16, 17):
        if M <= MAX_M:
            assert torch.equal(_kernel(xs[:M], q, scale, cfg), full[:M]), \
                f"M = {M} differs from the M = {MAX_M} run"


@pytest.mark.parametrize("M", [1, 3, 17])
def test_writes_only_y(M):
    xs, q, scale, _, _ = _case(512, 48)
    N, pad = 48, 4096
    buf = torch.full((pad + M * N + pad,), 0x7B7B, dtype=torch.int16,
                     device=DEV)
    y = buf[pad:pad + M * N].view(torch.bfloat16).view(M, N)
    _kernel(xs[:M], q, scale, y=y)
    torch.cuda.synchronize()
    assert (buf[:pad] == 0x7B7B).all() and (buf[pad + M * N:] == 0x7B7B).all()
    assert torch.equal(y, _kernel(xs[:M], q, scale))


@pytest.mark.parametrize("M", [1, 3, 17])
def test_reads_only_the_first_m_rows(M):
    xs, q, scale, _, _ = _case(512, 48)
    xbuf = torch.full_like(xs, float("nan"))
    xbuf[:M] = xs[:M]
    y = _kernel(xbuf[:M], q, scale)
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y, _kernel(xs[:M].contiguous(), q, scale))


@pytest.mark.parametrize("N,K", [(1, 32), (37, 544), (1040, 1536)])
def test_dequant(N, K):
    g = torch.Generator(device=DEV)
    g.manual_seed(N * 10000 + K)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    q, scale = quantize_mxfp4(w)
    pad = 1024
    buf = torch.full((pad + N * K + pad,), 0x7B7B, dtype=torch.int16,
                     device=DEV)
    out = buf[pad:pad + N * K].view(torch.bfloat16).view(N, K)
    ops.hip().mxfp4_dequant(out, q, scale)
    torch.cuda.synchronize()
    _assert_exact(out, Mxfp4Weight(q, scale).effective(torch.bfloat16))
    assert (buf[:pad] == 0x7B7B).all() and (buf[pad + N * K:] == 0x7B7B).all()


# ---- dispatch ---------------------------------------------------------
def _rand(*shape, seed, dtype=torch.bfloat16, std=1.0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * std).to(dtype)


def test_dispatch_takes_kernel_when_eligible():
    xs, q, scale, _, _ = _case(1024, 48)
    w = Mxfp4Weight(q, scale)
    cfg = ops.MXFP4_GEMM_SPLIT_K        # K = 1024 allows the 4-wave K split
    assert ops.mxfp4_linear_path(xs, w) == ("kernel", cfg)
    assert torch.equal(ops.linear(xs, w), _kernel(xs, q, scale, cfg))
    assert ops.mxfp4_linear_path(xs[:1], w) == ("kernel", cfg)
    assert torch.equal(ops.linear(xs[:1], w), _kernel(xs[:1], q, scale, cfg))
    # K = 512 does not: the default configuration
    x, q2, scale2, _, _ = _case(512, 48)
    w2 = Mxfp4Weight(q2, scale2)
    assert ops.mxfp4_linear_path(x, w2) == ("kernel", DEFAULT)
    assert torch.equal(ops.linear(x, w2), _kernel(x, q2, scale2, DEFAULT))


def _other_calls():
    _, q, scale, _, _ = _case(512, 48)
    w288 = Mxfp4Weight(*quantize_mxfp4(_rand(48, 288, seed=3, std=0.02)))
    return {
        "M=MAX_M+1": (_rand(MAX_M + 1, 512, seed=1), Mxfp4Weight(q, scale)),
        "K=288": (_rand(16, 288, seed=2), w288),
        "non-contiguous x": (_rand(16, 1024, seed=4)[:, :512],
                             Mxfp4Weight(q, scale)),
    }


@pytest.mark.parametrize("case", ["M=MAX_M+1", "K=288", "non-contiguous x"])
def test_dispatch_other_calls_dequantise(case):
    x, w = _other_calls()[case]
    assert ops.mxfp4_linear_path(x, w) == ("dequant", None)
    assert torch.equal(ops.linear(x, w),
                       F.linear(x, w.effective(torch.bfloat16)))


def test_binding_rejects_what_the_kernel_cannot_do():
    xs, q, scale, _, _ = _case(512, 48)
    hip = ops.hip()

    def y(M, N, dtype=torch.bfloat16):
        return torch.empty(M, N, dtype=dtype, device=DEV)

    with pytest.raises(RuntimeError):   # M too large
        hip.mxfp4_skinny_gemm(y(MAX_M + 1, 48), _rand(MAX_M + 1, 512, seed=1),
                              q, scale, *DEFAULT)
    with pytest.raises(RuntimeError):   # N = 40
        hip.mxfp4_skinny_gemm(y(16, 40), xs[:16], q[:40].contiguous(),
                              scale[:40].contiguous(), *DEFAULT)
    with pytest.raises(RuntimeError):   # fp16 x
        hip.mxfp4_skinny_gemm(y(16, 48, torch.float16),
                              xs[:16].to(torch.float16), q, scale, *DEFAULT)
    with pytest.raises(RuntimeError):   # unknown configuration
        hip.mxfp4_skinny_gemm(y(16, 48), xs[:16], q, scale, 3, 1, 2)
    with pytest.raises(RuntimeError):   # K = 512 is no multiple of 4 * 256
        hip.mxfp4_skinny_gemm(y(16, 48), xs[:16], q, scale, 4, 1, 2)
    with pytest.raises(RuntimeError):   # q [N, K]: one code per byte
        hip.mxfp4_skinny_gemm(y(16, 48), xs[:16],
                              torch.zeros(48, 512, dtype=torch.uint8,
                                          device=DEV), scale, *DEFAULT)
    with pytest.raises(RuntimeError):   # scale [N, K / 64]
        hip.mxfp4_skinny_gemm(y(16, 48), xs[:16], q,
                              scale[:, :8].contiguous(), *DEFAULT)
    with pytest.raises(RuntimeError):   # scale [N]: one per row
        hip.mxfp4_skinny_gemm(y(16, 48), xs[:16], q,
                              scale[:, 0].contiguous(), *DEFAULT)
    with pytest.raises(RuntimeError):   # scale of another dtype
        hip.mxfp4_skinny_gemm(y(16, 48), xs[:16], q, scale.float(), *DEFAULT)
    out = y(48, 512)
    with pytest.raises(RuntimeError):   # dequant: wrong scale shape
        hip.mxfp4_dequant(out, q, scale[:, :8].contiguous())
    with pytest.raises(RuntimeError):   # dequant: wrong q shape
        hip.mxfp4_dequant(out, q[:, :128].contiguous(), scale)


# ---- engine -------------------------------------------------------------
PROJ = (("attn", "wqkv"), ("attn", "wo"), ("mlp", "w_gate_up"),
        ("mlp", "w_down"))


def make_engine(**kw):
    kw.setdefault("kv_pool_pages", 256)
    kw.setdefault("weight_dtype", "mxfp4")
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
def _mxfp4_tokens():
    return generate(make_engine(), PROMPTS)


def test_engine_two_builds_agree():
    o = generate(make_engine(), PROMPTS)
    assert o == _mxfp4_tokens()
    assert all(len(t) == 8 for t in o)


def test_engine_graphs_on_and_off_agree():
    assert generate(make_engine(enable_hip_graphs=False),
                    PROMPTS) == _mxfp4_tokens()


def test_engine_with_fp8_kv_cache():
    o = generate(make_engine(kv_cache_dtype="fp8"), PROMPTS)
    assert all(len(t) == 8 for t in o)


def test_engine_decode_shapes_take_the_kernel():
    eng = make_engine()
    for layer in eng.runner.model.layers:
        for sub, name in PROJ:
            w = getattr(getattr(layer, sub), name)
            assert isinstance(w, Mxfp4Weight)
            assert w.q.dtype == torch.uint8 and w.scale.dtype == torch.uint8
            assert w.shape[1] % 256 == 0
            for M in sorted({1, 8, MAX_M}):
                x = torch.zeros(M, w.shape[1], dtype=torch.bfloat16,
                                device=DEV)
                assert ops.mxfp4_linear_path(x, w)[0] == "kernel"
            x = torch.zeros(80, w.shape[1], dtype=torch.bfloat16, device=DEV)
            assert ops.mxfp4_linear_path(x, w) == ("dequant", None)


def test_engine_prefill_matches_w_eff_twin():
    """An 80-token prefill runs the dequantise path: the same library call
    on the same bits as an unquantised twin holding W_eff."""
    mx = make_engine(enable_hip_graphs=False)
    twin = make_engine(enable_hip_graphs=False, weight_dtype="bf16")
    for lf, lt in zip(mx.runner.model.layers, twin.runner.model.layers):
        for sub, name in PROJ:
            h = getattr(getattr(lf, sub), name)
            with torch.no_grad():
                getattr(getattr(lt, sub), name).copy_(
                    h.effective(torch.bfloat16))
    prompt = [list(range(100, 180))]
    a = generate(mx, prompt, max_tokens=1)
    b = generate(twin, prompt, max_tokens=1)
    assert a == b and len(a[0]) == 1
