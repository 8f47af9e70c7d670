"""Opt-in MXFP4 (e2m1 + e8m0) weights, CPU side: the quantiser, the weight
holder, quantize_model_mxfp4, the weight_dtype option and what an mxfp4
engine refuses.

The quantiser bound follows from its construction (ops/mxfp4_weights.py):
e = floor(log2(amax_block)) - 2 puts every |w| / 2^e of the block in [0, 8);
the e2m1 grid {0, 0.5, 1, 1.5, 2, 3, 4, 6} has spacing at most 2 up to 6, so
rounding to nearest loses at most 1, and saturating (6, 8) at 6 loses less
than 2: |w - W_eff| < 2 * 2^e per element. Scaling by a power of two is exact
in fp32, so the bound carries no rounding allowance.
"""
import pytest
import torch
import torch.nn.functional as F

from dynamo_amd import envs, ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS
from dynamo_amd.ops import Mxfp4Weight, quantize_mxfp4

PROJ = (("attn", "wqkv"), ("attn", "wo"), ("mlp", "w_gate_up"),
        ("mlp", "w_down"))
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def codes_of(q):
    """q [N, K/2] -> codes [N, K]: even k from the low nibble."""
    return torch.stack((q & 15, q >> 4), dim=2).view(q.shape[0], -1)


def w_eff(q, scale):
    """W_eff by the definition, in float64 and independent of the module's
    own dequantiser."""
    c = codes_of(q).long()
    mag = torch.tensor(GRID, dtype=torch.float64)[c & 7]
    sign = torch.where((c & 8) != 0, -1.0, 1.0).double()
    s = torch.pow(2.0, scale.double() - 127).repeat_interleave(32, dim=1)
    return mag * sign * s


def block(values, fill=0.0):
    """One 32-element block [1, 32] starting with `values`."""
    w = torch.full((1, 32), fill, dtype=torch.float32)
    w[0, :len(values)] = torch.tensor(values, dtype=torch.float32)
    return w


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(1040 * 1536)
    w = (torch.randn(1040, 1536, generator=g) * 0.02).to(torch.bfloat16)
    q, scale = quantize_mxfp4(w)
    return w, q, scale, w_eff(q, scale)


def test_shapes_and_coverage(case):
    w, q, scale, _ = case
    assert q.dtype == torch.uint8 and q.shape == (1040, 768)
    assert scale.dtype == torch.uint8 and scale.shape == (1040, 48)
    assert codes_of(q).unique().numel() == 16
    assert scale.unique().numel() >= 3


def test_w_eff_is_exact_in_bf16(case):
    _, q, scale, eff = case
    assert torch.equal(eff.to(torch.bfloat16).double(), eff)
    h = Mxfp4Weight(q, scale)
    assert torch.equal(h.effective(torch.float32).double(), eff)
    assert torch.equal(h.effective(torch.bfloat16).double(), eff)


def test_quantiser_is_idempotent(case):
    _, q, scale, eff = case
    q2, scale2 = quantize_mxfp4(eff.to(torch.bfloat16))
    assert torch.equal(scale2, scale)
    c, c2 = codes_of(q), codes_of(q2)
    # modulo the sign of zero: codes 0 and 8
    zero = (c & 7) == 0
    assert torch.equal(c2 & 7, c & 7)
    assert torch.equal(c2[~zero], c[~zero])


def test_quantiser_bound(case):
    w, _, scale, eff = case
    unit = torch.pow(2.0, scale.double() - 127 ).repeat_interleave(32, dim=1)
    ratio = ((w.double() - eff).abs() / unit).max().item()
    print(f"worst |w - W_eff| / 2^e = {ratio:.6f} (bound 2)")
    assert ratio < 2.0
    # the block maximum lands on code 6 or 7 (4 or 6)
    top = (codes_of(case[1]) & 7).view(1040, 48, 32).amax(dim=2)
    assert (top >= 6).all()


@pytest.mark.parametrize("p", [-20, -3, 0, 5])
def test_ties_go_to_the_even_code(p):
    s = 2.0 ** p
    # 4s pins e = p (amax / 2^e = 4); then the seven midpoints of the grid
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    vals = [4.0] + ties + [-t for t in ties]
    q, scale = quantize_mxfp4(block([v * s for v in vals]))
    assert scale[0, 0] == 127 + p
    c = codes_of(q)[0]
    assert c[0] == 6
    assert c[1:8].tolist() == [0, 2, 2, 4, 4, 6, 6]
    assert c[8:15].tolist() == [8, 10, 10, 12, 12, 14, 14]
    # just off a midpoint goes to the nearer neighbour
    eps = 2.0 ** -10
    q, _ = quantize_mxfp4(block([4.0 * s] + [(t + eps) * s for t in ties]
                                + [(t - eps) * s for t in ties]))
    c = codes_of(q)[0]
    assert c[1:8].tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert c[8:15].tolist() == [0, 1, 2, 3, 4, 5, 6]


def test_saturates_at_six():
    # amax 7.75 -> e = 0; 6.5, 7, 7.75 lie in (6, 8) and saturate
    q, scale = quantize_mxfp4(block([7.75, 7.0, 6.5, -7.5, 6.0, 5.5]))
    assert scale[0, 0] == 127
    assert codes_of(q)[0, :6].tolist() == [7, 7, 7, 15, 7, 7]
    eff = w_eff(q, scale)[0, :6]
    assert eff.tolist() == [6.0, 6.0, 6.0, -6.0, 6.0, 6.0]


def test_all_zero_block():
    w = torch.zeros(2, 64)
    w[1, 40] = -0.0
    w[0, 5] = 3.0
    q, scale = quantize_mxfp4(w)
    assert scale[0, 1] == 127 and scale[1, 0] == 127 and scale[1, 1] == 127
    assert (w_eff(q, scale)[1] == 0).all()
    assert (codes_of(q)[0, 32:] == 0).all()
    assert w_eff(q, scale)[0, 5] == 3.0


def test_exponent_clamp():
    big, small = 2.0 ** 120, 2.0 ** -120
    w = torch.cat([block([big, -big, big / 2, 2.0 ** 100]),
                   block([small, -small]),
                   block([6 * 2.0 ** -100, 0.5 * 2.0 ** -100,
                          0.2 * 2.0 ** -100])], dim=1)
    q, scale = quantize_mxfp4(w)
    assert scale[0].tolist() == [227, 27, 27]
    c = codes_of(q)[0]
    # above the clamp everything saturates; 2^100 = 1 * 2^100 is code 2
    assert c[:4].tolist() == [7, 15, 7, 2]
    # below it the block rounds to zero, keeping the signs
    assert c[32:34].tolist() == [0, 8]
    assert c[64:67].tolist() == [7, 1, 0]
    eff = w_eff(q, scale)[0]
    assert eff[0] == 6 * 2.0 ** 100 and eff[65] == 2.0 ** -101
    # the smallest nonzero and the largest W_eff are normal bf16 numbers
    tiny = torch.finfo(torch.bfloat16).tiny
    assert 0.5 * 2.0 ** -100 >= tiny
    assert 6 * 2.0 ** 100 <= torch.finfo(torch.bfloat16).max


def test_nibble_order():
    # k = 0 -> 1.0 (code 2), k = 1 -> -6.0 (code 15), k = 2 -> 0.5 (code 1)
    q, scale = quantize_mxfp4(block([1.0, -6.0, 0.5, 4.0]))
    assert scale[0, 0] == 127
    assert q[0, 0] == (2 | (15 << 4))
    assert q[0, 1] == (1 | (6 << 4))
    assert (q[0, 2:] == 0).all()


@pytest.mark.parametrize("K", [16, 48, 1000])
def test_k_must_be_a_multiple_of_32(K):
    with pytest.raises(ValueError, match="32"):
        quantize_mxfp4(torch.zeros(4, K))


def test_holder_is_not_a_tensor(case):
    _, q, scale, eff = case
    h = Mxfp4Weight.from_tensor(case[0])
    assert not isinstance(h, torch.Tensor)
    assert torch.equal(h.q, q) and torch.equal(h.scale, scale)
    assert tuple(h.shape) == (1040, 1536) and h.dim() == 2
    assert h.device == q.device
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 1536, generator=g)
    assert ops.mxfp4_linear_path(x, h) == ("torch", None)
    assert torch.equal(ops.linear(x, h), F.linear(x, eff.float()))
    xb = x.to(torch.bfloat16)
    assert torch.equal(ops.linear(xb, h),
                       F.linear(xb, eff.to(torch.bfloat16)))


def test_gemm_config_tables():
    cfgs = ops.MXFP4_GEMM_CONFIGS
    assert ops.MXFP4_GEMM_DEFAULT in cfgs and ops.MXFP4_GEMM_SPLIT_K in cfgs
    d = ops.MXFP4_GEMM_DEFAULT
    assert d[0] * d[1] == 1                 # accepts every K % 256 == 0
    assert ops.MXFP4_GEMM_MAX_M in (16, 32, 64)
    assert any(c[2] == 8 for c in cfgs)
    assert set(ops.MXFP4_GEMM_SHAPES) == {(10240, 8192), (8192, 8192),
                                          (57344, 8192), (8192, 28672)}
    for (N, K), pair in ops.MXFP4_GEMM_SHAPES.items():
        for cfg in pair:
            assert cfg in cfgs and K % (cfg[0] * 256 * cfg[1]) == 0
        assert ops.mxfp4_gemm_config(16, N, K) == pair[0]
        assert ops.mxfp4_gemm_config(ops.MXFP4_GEMM_MAX_M + 1, N, K) is None
    assert ops.mxfp4_gemm_config(16, 48, 1024) == ops.MXFP4_GEMM_SPLIT_K
    assert ops.mxfp4_gemm_config(16, 48, 768) == d
    assert ops.mxfp4_gemm_config(16, 40, 1024) is None
    assert ops.mxfp4_gemm_config(16, 48, 288) is None
    assert ops.mxfp4_gemm_config(0, 48, 1024) is None


# ---- engine and options ---------------------------------------------------
def make_engine(model="tiny-llama", seed=7, **kw):
    cfg = EngineConfig(model=PRESETS[model], device="cpu", max_num_seqs=4,
                       max_batched_tokens=256, max_model_len=256,
                       kv_pool_pages=64, page_size=16, **kw)
    return LLMEngine(cfg, seed=seed)


def generate(engine, prompts, n=8):
    outs = {}
    for i, p in enumerate(prompts):
        engine.add_request(f"r{i}", p, SamplingParams(max_tokens=n))
        outs[f"r{i}"] = []
    while engine.has_work():
        for so in engine.step():
            outs[so.req_id].append(so.new_token)
    return [outs[f"r{i}"] for i in range(len(prompts))]


def test_twin_engine_equality():
    """An mxfp4 engine generates what an unquantised engine generates whose
    projections were overwritten with W_eff."""
    mx = make_engine(weight_dtype="mxfp4")
    twin = make_engine(weight_dtype="bf16")
    assert mx.runner.model.weight_dtype == "mxfp4"
    for lf, lt in zip(mx.runner.model.layers, twin.runner.model.layers):
        for sub, name in PROJ:
            h = getattr(getattr(lf, sub), name)
            t = getattr(getattr(lt, sub), name)
            assert isinstance(h, Mxfp4Weight) and isinstance(t, torch.Tensor)
            assert tuple(h.shape) == tuple(t.shape)
            assert h.q.dtype == torch.uint8 and h.scale.dtype == torch.uint8
            assert h.q.shape == (t.shape[0], t.shape[1] // 2)
            assert h.scale.shape == (t.shape[0], t.shape[1] // 32)
            with torch.no_grad():
                t.copy_(h.effective(t.dtype))
    # embedding, lm_head and norms keep the compute dtype
    model = mx.runner.model
    assert model.embed.dtype == torch.bfloat16
    assert model.lm_head.dtype == torch.bfloat16
    assert model.layers[0].input_norm_w.dtype == torch.bfloat16
    prompts = [list(range(3, 43)), [5, 9, 2] * 11]
    a, b = generate(mx, prompts), generate(twin, prompts)
    assert a == b
    assert all(len(o) == 8 for o in a)


def test_option_resolution(monkeypatch):
    assert "mxfp4" in envs.ENV_VARS["DYNAMO_WEIGHT_DTYPE"]
    monkeypatch.delenv("DYNAMO_WEIGHT_DTYPE", raising=False)
    assert EngineConfig().resolved_weight_dtype == "bf16"
    assert EngineConfig(weight_dtype="mxfp4").resolved_weight_dtype == "mxfp4"
    monkeypatch.setenv("DYNAMO_WEIGHT_DTYPE", "mxfp4")
    assert EngineConfig().resolved_weight_dtype == "mxfp4"
    assert isinstance(make_engine().runner.model.layers[0].attn.wqkv,
                      Mxfp4Weight)
    # an explicit value wins over the environment
    assert EngineConfig(weight_dtype="bf16").resolved_weight_dtype == "bf16"
    assert EngineConfig(weight_dtype="fp8").resolved_weight_dtype == "fp8"
    monkeypatch.setenv("DYNAMO_WEIGHT_DTYPE", "fp8")
    assert EngineConfig(weight_dtype="mxfp4").resolved_weight_dtype == "mxfp4"
    with pytest.raises(ValueError):
        EngineConfig(weight_dtype="int4").resolved_weight_dtype


def test_cli_passes_weight_dtype(monkeypatch):
    from dynamo_amd.workers.main import build_parser, make_engine_from_args
    p = build_parser()
    with pytest.raises(SystemExit):
        p.parse_args(["--weight-dtype", "int4"])
    args = p.parse_args(["--model", "tiny-llama", "--device", "cpu",
                         "--weight-dtype", "mxfp4", "--kv-pool-pages", "64",
                         "--max-model-len", "256", "--page-size", "16"])
    assert args.weight_dtype == "mxfp4"
    monkeypatch.delenv("DYNAMO_WEIGHT_DTYPE", raising=False)
    eng = make_engine_from_args(args)
    assert eng.cfg.weight_dtype == "mxfp4"
    assert isinstance(eng.runner.model.layers[0].attn.wqkv, Mxfp4Weight)


@pytest.mark.parametrize("model", ["tiny-opt", "tiny-mixtral"])
def test_refuses_unsupported_arch(model):
    with pytest.raises(ValueError, match="mxfp4 weights"):
        make_engine(model, weight_dtype="mxfp4")


def test_refuses_weight_pool():
    from dynamo_amd.gms import WeightPool
    from dynamo_amd.gms.pool import estimate_pool_bytes
    mc = PRESETS["tiny-llama"]
    pool = WeightPool(estimate_pool_bytes(mc), "cpu")
    cfg = EngineConfig(model=mc, device="cpu", max_num_seqs=4,
                       max_batched_tokens=256, max_model_len=256,
                       kv_pool_pages=64, page_size=16, weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="GMS"):
        LLMEngine(cfg, seed=7, weight_pool=pool)


def test_refuses_k_not_a_multiple_of_32():
    eng = make_engine(weight_dtype="bf16")
    model = eng.runner.model
    with torch.no_grad():
        wo = model.layers[-1].attn.wo
        model.layers[-1].attn.wo = wo[:, :wo.shape[1] - 8].contiguous()
    first = model.layers[0].attn.wqkv
    with pytest.raises(ValueError, match="multiple of the 32"):
        ops.quantize_model_mxfp4(model)
    # refused before anything was replaced
    assert model.layers[0].attn.wqkv is first
    assert not hasattr(model, "weight_dtype")


def test_refuses_lora_weight_delta_and_export(tmp_path):
    eng = make_engine(weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="load_lora"):
        eng.load_lora("a", rank=4)
    with pytest.raises(ValueError, match="apply_weight_delta"):
        eng.apply_weight_delta(1, 1e-3)
    from dynamo_amd.models.loader import export_hf
    with pytest.raises(ValueError, match="export_hf"):
        export_hf(eng.runner.model, str(tmp_path / "out"))
