"""Rope + KV append folded into decode attention == the two kernels, bit for
bit.

ops.paged_attention_decode_rope (paged_decode_mfma_swapped_dmajor_rope) is
held against the pair it replaces, ops.rope_append_qkv followed by
ops.paged_attention_decode, on cloned caches: torch.equal on the attention
output and on the WHOLE K and V caches, so a misplaced, missing or doubled
append and any write outside the slot show. The slot of the new token starts
as NaN in both caches: a kernel that read the token back stale instead of
using what it just computed would put NaN in the output.

Chunk 512 (what DecodeScratch picks below 2048 tokens), so a wave's slab is
128 tokens. The contexts put the new token (ctx - 1) at: the only token (1),
last / first of an 8-token run (8 / 9), of a 32-token K group (32 / 33), of a
64-token tile and page (64 / 65), of a slab (128 / 129), of a chunk (512 /
513, 1025), and mid-run (2).
"""
from types import SimpleNamespace

import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.models import layers
from dynamo_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HD, PS, MAX_CTX = 128, 64, 1536
CTX_ROWS = [(1, 2, 8), (9, 32, 33), (64, 65, 128), (129, 512, 513),
            (1025, 33, 1)]


def _case(Hq, Hkv, ctxs, bias, neg_rows=(), seed=0):
    """Seeded inputs of one decode step: row b has ctxs[b] tokens including
    the new one; rows in neg_rows carry slot -1."""
    B = len(ctxs)
    g = torch.Generator(device=DEV)
    g.manual_seed(seed * 7919 + Hq * 31 + sum(ctxs) + 2 * bias)
    maxp = MAX_CTX // PS
    P = B * maxp + 3
    width = (Hq + 2 * Hkv) * HD

    def randn(*shape, shift=0.0):
        # asymmetric: a sign or operand mix-up does not cancel
        return (torch.randn(*shape, generator=g, device=DEV) + shift).to(
            torch.bfloat16)

    # a wider buffer sliced down: the kernels read qkv through its row stride
    qkv = randn(B, width + 64, shift=0.25)[:, :width]
    b = randn(width, shift=-0.125) if bias else None
    kc = randn(P, Hkv, PS, HD, shift=0.125)
    vc = randn(P, Hkv, HD, PS, shift=-0.25)
    pt = torch.randperm(P, generator=g, device=DEV)[:B * maxp].view(
        B, maxp).to(torch.int32)
    ctx = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    pos = (ctx - 1).clamp(min=0)
    slots = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    for r, c in enumerate(ctxs):
        if r in neg_rows or c == 0:
            continue
        page, off = int(pt[r, (c - 1) // PS]), (c - 1) % PS
        slots[r] = page * PS + off
        kc[page, :, off, :] = float("nan")
        vc[page, :, :, off] = float("nan")
    cos_sin = torch_ref.make_cos_sin_cache(MAX_CTX, HD, 10000.0, device=DEV)
    return SimpleNamespace(qkv=qkv, bias=b, kc=kc, vc=vc, pt=pt, ctx=ctx,
                           pos=pos, slots=slots, cos_sin=cos_sin, Hq=Hq,
                           Hkv=Hkv, B=B, scale=HD ** -0.5)


def _pair(c, scratch):
    kc, vc = c.kc.clone(), c.vc.clone()
    q = ops.rope_append_qkv(c.qkv, c.bias, c.pos, c.slots, c.cos_sin, kc, vc,
                            c.Hq, c.Hkv, HD, v_transposed=True)
    out = ops.paged_attention_decode(q.view(c.B, c.Hq, HD), kc, vc, c.pt,
                                     c.ctx, c.scale, scratch,
                                     v_transposed=True)
    return out, kc, vc


def _fused(c, scratch):
    kc, vc = c.kc.clone(), c.vc.clone()
    out = ops.paged_attention_decode_rope(
        c.qkv, c.bias, c.pos, c.slots, c.cos_sin, kc, vc, c.pt, c.ctx,
        c.scale, scratch, c.Hq, c.Hkv, HD)
    return out, kc, vc


def _assert_same(got, ref):
    for a, b in zip(got, ref):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("ctxs", CTX_ROWS)
@pytest.mark.parametrize("Hq,Hkv", [(64, 8), (32, 8)])
def test_fused_matches_rope_append_then_decode(Hq, Hkv, ctxs, bias):
    c = _case(Hq, Hkv, ctxs, bias)
    scratch = ops.DecodeScratch(c.B, Hq, HD, MAX_CTX, DEV)
    assert scratch.chunk_tokens == 512 and scratch.chunks == 3
    ref = _pair(c, scratch)
    got = _fused(c, scratch)
    assert not torch.isnan(ref[0].float()).any()
    _assert_same(got, ref)
    # the append happened: no NaN marker is left in either cache
    assert not torch.isnan(got[1].float()).any()
    assert not torch.isnan(got[2].float()).any()


@pytest.mark.parametrize("bias", [False, True])
def test_negative_slot_appends_nothing(bias):
    """Row 1 is a live context whose slot is -1, row 2 a padded graph row
    (ctx 0, slot -1): neither may touch a cache, row 1 attends over what the
    pages hold and row 2 comes out as zeros."""
    c = _case(64, 8, (65, 33, 0), bias, neg_rows=(1, 2), seed=1)
    scratch = ops.DecodeScratch(c.B, 64, HD, MAX_CTX, DEV)
    ref = _pair(c, scratch)
    got = _fused(c, scratch)
    _assert_same(got, ref)
    assert not got[0][2].any()
    # only row 0's slot changed, in either cache
    page, off = divmod(int(c.slots[0]), PS)
    kc0, vc0 = c.kc.clone(), c.vc.clone()
    kc0[page, :, off, :] = got[1][page, :, off, :]
    vc0[page, :, :, off] = got[2][page, :, :, off]
    _assert_same((got[1], got[2]), (kc0, vc0))


def test_layer_takes_the_switch(monkeypatch):
    """Attention.forward of a decode step: the fused op with the switch on,
    rope_append_qkv + paged_attention_decode with it off; equal bits."""
    Hq, Hkv, D = 32, 8, 256
    c = _case(Hq, Hkv, (129, 64, 513), False, seed=2)
    cfg = SimpleNamespace(num_q_heads=Hq, num_kv_heads=Hkv, head_dim=HD,
                          hidden_size=D, attn_bias=True)
    torch.manual_seed(3)
    attn = layers.Attention(cfg, 0, layers.TPContext(), DEV, torch.bfloat16)
    x = torch.randn(c.B, D, dtype=torch.bfloat16, device=DEV)
    scratch = ops.DecodeScratch(c.B, Hq, HD, MAX_CTX, DEV)
    calls = []
    for name in ("rope_append_qkv", "paged_attention_decode",
                 "paged_attention_decode_rope"):
        real = getattr(ops, name)
        monkeypatch.setattr(
            ops, name,
            lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])

    def run(on):
        ops.set_fused_rope_attn(on)
        del calls[:]
        kc, vc = c.kc.clone(), c.vc.clone()
        meta = layers.AttnMetadata(
            slot_mapping=c.slots, positions=c.pos, num_decode=c.B,
            decode_page_table=c.pt, decode_ctx_lens=c.ctx,
            decode_scratch=scratch, v_transposed=True, decode_step=True)
        with torch.inference_mode():
            o = attn(x, c.cos_sin, kc, vc, meta)
        return (o, kc, vc), list(calls)

    try:
        off, off_calls = run(False)
        on, on_calls = run(True)
    finally:
        ops.set_fused_rope_attn(None)
    assert off_calls == ["rope_append_qkv", "paged_attention_decode"]
    assert on_calls == ["paged_attention_decode_rope"]
    _assert_same(on, off)
