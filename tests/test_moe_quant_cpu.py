"""Quantised Mixtral experts, CPU side: the [E, N, K] holders, the per-format
configuration rule of the routed GEMM, the torch path of ops.moe_decode_mlp
with holders, the model quantisers with the host-side expert loop, and what
a CPU engine refuses.

The CPU path of moe_decode_mlp rounds to bf16 where the bf16 block does (gu,
act; then fp32 to the one output rounding), so its bound is the block's:
tau_blk * S_row of tests/moe_cases.py, against the fp64 result on the exact
effective weights.
"""
import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine
from dynamo_amd.engine.config import PRESETS
from tests import moe_cases as mc

HOLDERS = {"fp8": ops.Fp8ExpertWeight, "mxfp4": ops.Mxfp4ExpertWeight}
KSTEP = {"fp8": 128, "mxfp4": 256}
FORMATS = ("fp8", "mxfp4")


@pytest.mark.parametrize("fmt", FORMATS)
def test_holder_round_trip(fmt):
    w = (torch.randn(3, 32, 256, generator=mc._gen("moe_quant_holder"))
         * 0.02).to(torch.bfloat16)
    h = HOLDERS[fmt].from_tensor(w)
    assert not isinstance(h, torch.Tensor)
    assert tuple(h.shape) == (3, 32, 256) and h.dim() == 3 and len(h) == 3
    eff = h.effective(torch.float32)
    assert eff.shape == w.shape
    two_d = type(h[0])
    for e in range(3):
        assert h[e].q.data_ptr() == h.q[e].data_ptr()          # a view
        assert tuple(h[e].shape) == (32, 256)
        assert torch.equal(h[e].effective(torch.float32), eff[e])
        # the 2-D quantiser on the expert's rows
        again = two_d.from_tensor(w[e])
        assert torch.equal(again.q.view(torch.uint8),
                           h[e].q.view(torch.uint8))
        assert torch.equal(again.scale, h[e].scale)
    assert float((eff - w.float()).abs().max()) < 0.02


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_config_covers_mixtral(fmt):
    kstep, configs, shapes = ops.MOE_DECODE_FORMATS[fmt]
    assert kstep == KSTEP[fmt] and (1, 1, 2) in configs and len(configs) <= 8
    assert all(c[2] % 2 == 0 for c in configs)
    for entry in shapes.values():
        assert all(c in configs for c in entry)
    D, I = 4096, 14336
    for tp in (1, 2, 4, 8):
        for N, K in ((2 * I // tp, D), (D, I // tp)):
            for T in (1, 16, 17, 64):
                c = ops.moe_decode_config(N, K, T, fmt)
                assert c in configs and K % (c[0] * kstep * c[1]) == 0
            assert ops.moe_decode_config(N, K, 65, fmt) is None
    assert ops.moe_decode_config(256, kstep // 2, 1, fmt) is None
    assert ops.moe_decode_config(256, 3 * kstep, 1, fmt)[:2] == (1, 1)
    # the bf16 rule is what it was
    assert ops.moe_decode_config(768, 256, 16) == (2, 2, 2)


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_mlp_cpu_path(fmt):
    x = mc.block_x(16)
    logits = mc.cpu_block_logits(x)
    _, wgu, wd = mc.block_weights()
    hgu, hd = HOLDERS[fmt].from_tensor(wgu), HOLDERS[fmt].from_tensor(wd)
    topw, topi = ops.topk_gating(logits, mc.BLK_K)
    assert not ops.moe_decode_ready(x, mc.BLK_K, hgu, hd)     # CPU tensors
    out = ops.moe_decode_mlp(x, topw, topi, hgu, hd)
    assert out.shape == x.shape and out.dtype == torch.bfloat16
    egu, ed = hgu.effective(torch.float64), hd.effective(torch.float64)
    ref = torch.zeros(16, mc.BLK_D, dtype=torch.float64)
    for t in range(16):
        for j in range(mc.BLK_K):
            e = int(topi[t, j])
            gu = egu[e] @ x[t].double()
            g, u = gu[:mc.BLK_I], gu[mc.BLK_I:]
            ref[t] += topw[t, j].double() * (ed[e] @ (g * torch.sigmoid(g) * u))
    assert float(mc.block_ratio(out, ref).max()) <= mc.tau_blk()


@pytest.mark.parametrize("fmt", FORMATS)
def test_quantise_model_and_host_loop(fmt):
    """quantize_model_* on a Mixtral model, and the CPU forward of a quantised
    MoEMLP (the per-expert loop): the same F.linear calls as a bf16 twin
    holding effective(bf16), so the same bits."""
    from dynamo_amd.models.mixtral import MixtralForCausalLM
    model, twin = (MixtralForCausalLM(PRESETS["tiny-mixtral"]) for _ in "ab")
    assert getattr(ops, "quantize_model_" + fmt)(model) == 8
    assert model.weight_dtype == fmt
    x = torch.randn(70, 128, generator=mc._gen("moe_quant_loop")).bfloat16()
    for lq, lt in zip(model.layers, twin.layers):
        assert isinstance(lq.attn.wqkv, type(lq.moe.w_down[0]))
        assert isinstance(lq.moe.router, torch.Tensor)
        for name in ("w_gate_up", "w_down"):
            h = getattr(lq.moe, name)
            assert isinstance(h, HOLDERS[fmt])
            getattr(lt.moe, name).copy_(h.effective(torch.bfloat16))
        assert torch.equal(lq.moe.forward(x), lt.moe.forward(x))


@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_refusals(fmt):
    def engine(model):
        cfg = EngineConfig(model=PRESETS[model], device="cpu", max_num_seqs=4, kv_pool_pages=64,
                           max_batched_tokens=256, max_model_len=256,
                           page_size=16, weight_dtype=fmt)
        return LLMEngine(cfg, seed=7)
    for model, what in (("tiny-mixtral", "GPU engine"),
                        ("tiny-opt", f"{fmt} weights")):
        with pytest.raises(ValueError, match=what):
            engine(model)
