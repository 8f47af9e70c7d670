"""Host side of the multi-query attention route: what the kernel takes, the
per-row causal limits it is given, and the switch's default."""
import pytest
import torch

from dynamo_amd import envs, ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn


@pytest.mark.parametrize("q_lens,Hq,Hkv,hd,ps,vt,dtype,want", [
    ([8, 3], 64, 8, 128, 64, True, BF16, True),
    ([8], 64, 8, 128, 32, True, FP8, True),
    ([9], 64, 8, 128, 64, True, BF16, False),        # q_len 9
    ([8, 2], 18, 2, 128, 64, True, BF16, False),     # q_len * G = 72
    ([4], 64, 8, 128, 64, False, BF16, False),       # token-major V
    ([4], 64, 8, 64, 64, True, BF16, False),         # head_dim 64
    ([4], 64, 8, 128, 16, True, BF16, False),        # page 16
    ([4], 64, 8, 128, 64, True, torch.float32, False),
    ([4], 8, 8, 128, 64, True, BF16, False),         # G = 1 has no d-major V
    ([], 64, 8, 128, 64, True, BF16, False),
])
def test_multiquery_ready(q_lens, Hq, Hkv, hd, ps, vt, dtype, want):
    assert ops.multiquery_ready(q_lens, Hq, Hkv, hd, ps, vt, dtype) is want


def test_row_ctx():
    i32 = dict(dtype=torch.int32)
    q_len = torch.tensor([3, 0, 1, 4], **i32)
    q_start = torch.tensor([0, 3, 3, 4], **i32)
    ctx = torch.tensor([3, 17, 600, 513], **i32)
    got = ops.multiquery_row_ctx(q_start, q_len, ctx, 8)
    assert got.dtype == torch.int32
    assert got.tolist() == [1, 2, 3, 600, 510, 511, 512, 513]


def test_switch_defaults_off_and_prepare_ignores_short_chunks(monkeypatch):
    assert "DYNAMO_MQ_ATTN" in envs.ENV_VARS
    monkeypatch.delenv("DYNAMO_MQ_ATTN", raising=False)
    monkeypatch.setattr(ops, "_multiquery_override", None)
    assert not ops.multiquery_attn_enabled()
    monkeypatch.setenv("DYNAMO_MQ_ATTN", "1")
    assert ops.multiquery_attn_enabled()
    ops.set_multiquery_attn(False)
    assert not ops.multiquery_attn_enabled()

    cfg = EngineConfig(model=PRESETS["tiny-llama"], device="cpu",
                       dtype="float32", max_num_seqs=4, max_batched_tokens=64,
                       max_model_len=256, kv_pool_pages=32, page_size=16)
    e = LLMEngine(cfg, seed=1)
    assert e.runner.multiquery_scratch is None
    e.add_request("short", list(range(5)), SamplingParams(max_tokens=2))
    _, meta = e.runner.prepare(e.scheduler.schedule())
    assert meta.num_prefill_tokens == 5 and meta.prefill_multiquery is None
