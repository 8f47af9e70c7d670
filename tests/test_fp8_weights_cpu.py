"""Opt-in FP8 (e4m3) weights, CPU side: the quantiser, the weight holder,
quantize_model_fp8, the weight_dtype option and what an fp8 engine refuses.

The quantiser bound is the format's: with q = e4m3_rne(w / scale) the error
of W_eff = q * scale is at most half an e4m3 ulp of the element (3 mantissa
bits: |w| * 2^-4) or, below the normal range, half a subnormal step
(2^-9 / 2 = 2^-10, times scale). The factor 1 + 1e-5 covers the fp32 divide
and multiply.
"""
import pytest
import torch

from dynamo_amd import envs, ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS
from dynamo_amd.ops import Fp8Weight, quantize_fp8_rowwise

PROJ = (("attn", "wqkv"), ("attn", "wo"), ("mlp", "w_gate_up"),
        ("mlp", "w_down"))


def w_eff(q, scale, dtype=torch.float32):
    return (q.float() * scale[:, None]).to(dtype)


@pytest.mark.parametrize("N,K", [(48, 512), (1040, 1536), (48, 28672)])
def test_quantiser_bound(N, K):
    g = torch.Generator().manual_seed(1000 * K + N)
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    w[N // 2] = 0
    q, scale = quantize_fp8_rowwise(w)
    assert q.dtype == torch.float8_e4m3fn and q.shape == (N, K)
    assert scale.dtype == torch.float32 and scale.shape == (N,)
    assert scale[N // 2] == 1.0
    eff = w_eff(q, scale)
    assert torch.isfinite(eff).all()
    wf = w.float()
    bound = torch.maximum(wf.abs() * 2.0 ** -4,
                          scale[:, None] * 2.0 ** -10) * (1 + 1e-5)
    err = (eff - wf).abs()
    ratio = (err / bound.clamp_min(1e-45)).max().item()
    print(f"N={N} K={K}: violations={(err > bound).sum().item()} "
          f"worst ratio={ratio:.7f}")
    assert (err <= bound).all()
    assert (eff[N // 2] == 0).all()


def test_quantiser_saturates_instead_of_nan():
    # the absmax element lands exactly on +-448
    w = torch.tensor([[448.0, -448.0, 1.0, 0.5],
                      [3.0, -3.0, 1.0, 0.0]])
    q, scale = quantize_fp8_rowwise(w)
    assert scale[0] == 1.0
    assert q[0].float().tolist() == [448.0, -448.0, 1.0, 0.5]
    assert q[1].float().abs().max() == 448.0
    assert torch.isfinite(q.float()).all()
    # rows whose fp32 quotient absmax / fl(absmax / 448) rounds above 448
    # before clamping: the cast alone does not saturate
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(256, 64, generator=g) * 3e4).to(torch.bfloat16)
    q, scale = quantize_fp8_rowwise(w)
    over = (w.float() / scale[:, None]).abs().amax(dim=1) > 448.0
    print(f"{int(over.sum())} of 256 rows exceed 448 before the clamp")
    assert over.any()
    assert torch.isfinite(q.float()).all()
    assert (q.float().abs().amax(dim=1) == 448.0).all()


def test_holder_is_not_a_tensor():
    h = Fp8Weight.from_tensor(torch.randn(16, 32))
    assert not isinstance(h, torch.Tensor)
    assert tuple(h.shape) == (16, 32)
    assert torch.equal(h.effective(torch.float32), w_eff(h.q, h.scale))
    x = torch.randn(3, 32)
    assert ops.fp8_linear_path(x, h) == ("torch", None)
    assert torch.equal(ops.linear(x, h),
                       torch.nn.functional.linear(x, w_eff(h.q, h.scale)))


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


@pytest.mark.parametrize("model", ["tiny-llama", "tiny-qwen"])
def test_twin_engine_equality(model):
    """An fp8 engine generates what an unquantised engine generates whose
    projections were overwritten with W_eff: catches a scale attached to the
    wrong projection or a wrong row order."""
    fp8 = make_engine(model, weight_dtype="fp8")
    twin = make_engine(model, weight_dtype="bf16")
    for lf, lt in zip(fp8.runner.model.layers, twin.runner.model.layers):
        for sub, name in PROJ:
            h = getattr(getattr(lf, sub), name)
            t = getattr(getattr(lt, sub), name)
            assert isinstance(h, Fp8Weight) and isinstance(t, torch.Tensor)
            assert tuple(h.shape) == tuple(t.shape)
            with torch.no_grad():
                t.copy_(h.effective(t.dtype))
    prompts = [list(range(3, 43)), [5, 9, 2] * 11]
    a, b = generate(fp8, prompts), generate(twin, prompts)
    assert a == b
    assert all(len(o) == 8 for o in a)


def test_storage():
    eng = make_engine(weight_dtype="fp8")
    model = eng.runner.model
    for layer in model.layers:
        for sub, name in PROJ:
            h = getattr(getattr(layer, sub), name)
            assert isinstance(h, Fp8Weight)
            assert h.q.dtype == torch.float8_e4m3fn and h.q.dim() == 2
            assert h.scale.dtype == torch.float32
            assert h.scale.shape == (h.q.shape[0],)
    # embedding, lm_head and norms keep the compute dtype
    assert model.embed.dtype == torch.bfloat16
    assert model.lm_head.dtype == torch.bfloat16
    assert model.layers[0].input_norm_w.dtype == torch.bfloat16


def test_auto_resolution(monkeypatch):
    assert "DYNAMO_WEIGHT_DTYPE" in envs.ENV_VARS
    monkeypatch.delenv("DYNAMO_WEIGHT_DTYPE", raising=False)
    assert EngineConfig().weight_dtype == "auto"
    assert EngineConfig().resolved_weight_dtype == "bf16"
    plain = make_engine()
    assert isinstance(plain.runner.model.layers[0].attn.wqkv, torch.Tensor)
    assert plain.runner.model.layers[0].attn.wqkv.dtype == torch.bfloat16
    monkeypatch.setenv("DYNAMO_WEIGHT_DTYPE", "fp8")
    assert EngineConfig().resolved_weight_dtype == "fp8"
    assert isinstance(make_engine().runner.model.layers[0].attn.wqkv,
                      Fp8Weight)
    # an explicit value wins over the environment
    assert EngineConfig(weight_dtype="bf16").resolved_weight_dtype == "bf16"
    assert isinstance(
        make_engine(weight_dtype="bf16").runner.model.layers[0].attn.wqkv,
        torch.Tensor)
    monkeypatch.setenv("DYNAMO_WEIGHT_DTYPE", "bf16")
    assert EngineConfig(weight_dtype="fp8").resolved_weight_dtype == "fp8"
    with pytest.raises(ValueError):
        EngineConfig(weight_dtype="int4").resolved_weight_dtype


def test_default_build_unchanged(monkeypatch):
    """With the option off the model holds the tensors it held before."""
    monkeypatch.delenv("DYNAMO_WEIGHT_DTYPE", raising=False)
    a, b = make_engine(), make_engine(weight_dtype="bf16")
    for la, lb in zip(a.runner.model.layers, b.runner.model.layers):
        for sub, name in PROJ:
            assert torch.equal(getattr(getattr(la, sub), name),
                               getattr(getattr(lb, sub), name))
    assert not hasattr(a.runner.model, "weight_dtype")


@pytest.mark.parametrize("model", ["tiny-opt", "tiny-mixtral"])
def test_refuses_unsupported_arch(model):
    with pytest.raises(ValueError, match="fp8 weights"):
        make_engine(model, weight_dtype="fp8")


def test_refuses_weight_pool():
    from dynamo_amd.gms import WeightPool
    from dynamo_amd.gms.pool import estimate_pool_bytes
    mc = PRESETS["tiny-llama"]
    pool = WeightPool(estimate_pool_bytes(mc), "cpu")
    cfg = EngineConfig(model=mc, device="cpu", max_num_seqs=4,
                       max_batched_tokens=256, max_model_len=256,
                       kv_pool_pages=64, page_size=16, weight_dtype="fp8")
    with pytest.raises(ValueError, match="GMS"):
        LLMEngine(cfg, seed=7, weight_pool=pool)


def test_refuses_lora_weight_delta_and_export(tmp_path):
    eng = make_engine(weight_dtype="fp8")
    with pytest.raises(ValueError, match="load_lora"):
        eng.load_lora("a", rank=4)
    with pytest.raises(ValueError, match="apply_weight_delta"):
        eng.apply_weight_delta(1, 1e-3)
    from dynamo_amd.models.loader import export_hf
    with pytest.raises(ValueError, match="export_hf"):
        export_hf(eng.runner.model, str(tmp_path / "out"))


def test_cli_passes_weight_dtype(monkeypatch):
    from dynamo_amd.workers.main import build_parser, make_engine_from_args
    p = build_parser()
    assert p.parse_args([]).weight_dtype == "auto"
    with pytest.raises(SystemExit):
        p.parse_args(["--weight-dtype", "int4"])
    args = p.parse_args(["--model", "tiny-llama", "--device", "cpu",
                         "--weight-dtype", "fp8", "--kv-pool-pages", "64",
                         "--max-model-len", "256", "--page-size", "16"])
    assert args.weight_dtype == "fp8"
    monkeypatch.delenv("DYNAMO_WEIGHT_DTYPE", raising=False)
    eng = make_engine_from_args(args)
    assert eng.cfg.weight_dtype == "fp8"
    assert isinstance(eng.runner.model.layers[0].attn.wqkv, Fp8Weight)
