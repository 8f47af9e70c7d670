"""CPU side of the routed MoE decode route: the torch reference of
ops.moe_decode_mlp against the fp64 block reference of tests/moe_cases.py,
and the route's registration."""
import torch

from dynamo_amd import envs, ops
from tests import moe_cases as mc


def test_decode_mlp_reference_matches_block():
    x = mc.block_x(16)
    logits = mc.cpu_block_logits(x)
    _, wgu, wd = mc.block_weights()
    topw, topi = ops.topk_gating(logits, mc.BLK_K)
    out = ops.moe_decode_mlp(x, topw, topi, wgu, wd)
    assert out.shape == x.shape and out.dtype == torch.bfloat16
    mc.assert_block_close(out, mc.block_reference(x, logits), "torch_ref")


def test_registered():
    assert "DYNAMO_MOE_FUSED" in envs.ENV_VARS
    assert ops.MOE_DECODE_CONFIGS[0] == (1, 1, 2)
    for (N, K), entry in ops.MOE_DECODE_SHAPES.items():
        for cfg in entry:
            assert cfg in ops.MOE_DECODE_CONFIGS
            assert K % (cfg[0] * 64 * cfg[1]) == 0 and N % 32 == 0
    # no table entry: the deepest point that divides K; none below 64-k steps
    assert ops.moe_decode_config(768, 256, 16) == (2, 2, 2)
    assert ops.moe_decode_config(256, 384, 64) == (1, 2, 2)
    assert ops.moe_decode_config(256, 96, 1) is None
