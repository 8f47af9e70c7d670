"""Decode-step tail kernels: fast path == general path, bit for bit.

rmsnorm / fused_add_rmsnorm, rope_append_qkv and the argmax samplers each
have a latency-oriented kernel next to the general one. Every case runs the
op twice on cloned inputs, allow_fast=False then True, and requires
torch.equal on every output tensor (the flagship's logits are nearly flat,
so a last-ulp change anywhere can flip a token); the fast result is also
held against the torch reference at the tolerance tests/test_gpu_kernels.py
uses for that op.
"""
import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def assert_close(a, b, rtol=2e-2, atol=2e-2):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(),
                               rtol=rtol, atol=atol)


# D 2048 / 4096 / 8192: register kernel with 1 / 2 / 4 vectors per thread;
# 1024 and 5120 are no multiple of 8 * 256 and stay on the general kernel
NORM_D = [2048, 4096, 8192, 1024, 5120]


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("rows", [1, 16, 17])
def test_rmsnorm_fast_matches_general(rows, D):
    torch.manual_seed(rows * 10007 + D)
    x = torch.randn(rows, D, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(D, dtype=torch.bfloat16, device=DEV)
    slow = ops.rmsnorm(x.clone(), w, 1e-5, allow_fast=False)
    fast = ops.rmsnorm(x.clone(), w, 1e-5, allow_fast=True)
    assert torch.equal(fast, slow)
    assert_close(fast, torch_ref.rmsnorm(x, w, 1e-5))


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("rows", [1, 16, 17])
def test_fused_add_rmsnorm_fast_matches_general(rows, D):
    torch.manual_seed(rows * 10007 + D + 1)
    x = torch.randn(rows, D, dtype=torch.bfloat16, device=DEV)
    res = torch.randn(rows, D, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(D, dtype=torch.bfloat16, device=DEV)
    xs, rs = x.clone(), res.clone()
    xf, rf = x.clone(), res.clone()
    slow = ops.fused_add_rmsnorm(xs, rs, w, 1e-5, allow_fast=False)
    fast = ops.fused_add_rmsnorm(xf, rf, w, 1e-5, allow_fast=True)
    assert torch.equal(fast, slow)
    assert torch.equal(rf, rs)          # the written-back residual
    xr, rr = x.clone(), res.clone()
    ref = torch_ref.fused_add_rmsnorm(xr, rr, w, 1e-5)
    assert_close(rf, rr)
    assert_close(fast, ref)


# ---------------------------------------------------------------------------
def _rope_append_case(T, Hq, Hkv, hd, bias, vt, neg_row, fp8=False):
    ps, P = 64, 4
    torch.manual_seed(T * 131 + Hq * 7 + hd + 2 * bias + vt)
    width = (Hq + 2 * Hkv) * hd
    # a wider buffer sliced down: the op reads qkv through its row stride
    qkv = torch.randn(T, width + 64, dtype=torch.bfloat16,
                      device=DEV)[:, :width]
    b = (torch.randn(width, dtype=torch.bfloat16, device=DEV)
         if bias else None)
    pos = torch.randint(0, 500, (T,), dtype=torch.int32, device=DEV)
    slots = torch.randperm(P * ps, device=DEV)[:T].to(torch.int64)
    if neg_row is not None:
        slots[neg_row] = -1
    cos_sin = torch_ref.make_cos_sin_cache(512, hd, 10000.0, device=DEV)
    kc0 = torch.randn(P, Hkv, ps, hd, dtype=torch.bfloat16, device=DEV)
    vc0 = torch.randn((P, Hkv, hd, ps) if vt else (P, Hkv, ps, hd),
                      dtype=torch.bfloat16, device=DEV)
    cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16

    def run(allow_fast):
        kc, vc = kc0.to(cdt), vc0.to(cdt)
        q = ops.rope_append_qkv(qkv, b, pos, slots, cos_sin, kc, vc, Hq, Hkv,
                                hd, v_transposed=vt, allow_fast=allow_fast)
        return q, kc, vc

    qs, ks, vs = run(False)
    qf, kf, vf = run(True)
    # whole caches, as raw bytes: a stray write anywhere shows
    raw = torch.uint8 if fp8 else torch.int16
    assert torch.equal(qf, qs)
    assert torch.equal(kf.view(raw), ks.view(raw))
    assert torch.equal(vf.view(raw), vs.view(raw))

    # torch reference: the unfused CPU sequence, on bf16 caches that start
    # from what the GPU caches started from
    kr, vr = kc0.to(cdt).cpu().to(torch.bfloat16), \
        vc0.to(cdt).cpu().to(torch.bfloat16)
    qr = ops.rope_append_qkv(qkv.cpu(), None if b is None else b.cpu(),
                             pos.cpu(), slots.cpu(), cos_sin.cpu(), kr, vr,
                             Hq, Hkv, hd, v_transposed=vt)
    assert_close(qf, qr)
    # e4m3 keeps 3 mantissa bits; 0.12 is the fp8-cache tolerance of
    # tests/test_gpu_kernels.py
    tol = dict(rtol=0.12, atol=0.12) if fp8 else {}
    assert_close(kf, kr, **tol)
    assert_close(vf, vr, **tol)


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("Hq,Hkv,hd", [(64, 8, 128), (8, 1, 128), (12, 12, 64)])
@pytest.mark.parametrize("T", [1, 16, 19])
def test_rope_append_fast_matches_general(T, Hq, Hkv, hd, bias, vt):
    if T == 1:
        # a single row cannot both write the cache and be skipped
        _rope_append_case(T, Hq, Hkv, hd, bias, vt, neg_row=None)
        _rope_append_case(T, Hq, Hkv, hd, bias, vt, neg_row=0)
    else:
        _rope_append_case(T, Hq, Hkv, hd, bias, vt, neg_row=T // 2)


@pytest.mark.parametrize("vt", [False, True])
def test_rope_append_fast_matches_general_fp8_kv(vt):
    _rope_append_case(19, 64, 8, 128, True, vt, neg_row=5, fp8=True)


# ---------------------------------------------------------------------------
def _sampling_logits(B, V):
    """[(logits, {row: index the greedy winner must have})]: one row whose
    maximum is duplicated (the lower index wins), one whose maximum is the
    last element (the scalar tail), and at B > 1 one whose maximum is element
    0 of a row that starts off a 16-byte boundary when V % 4 != 0."""
    g = torch.Generator().manual_seed(B * 1000003 + V)
    base = torch.randn(B, V, generator=g)
    lo, hi = V // 3, V - 7
    if B == 1:
        dup, tail = base.clone(), base.clone()
        dup[0, lo] = dup[0, hi] = 9.0
        tail[0, V - 1] = 9.0
        return [(dup.to(DEV), {0: lo}), (tail.to(DEV), {0: V - 1})]
    base[0, lo] = base[0, hi] = 9.0
    base[B - 1, V - 1] = 9.0
    base[3, 0] = 9.0
    return [(base.to(DEV), {0: lo, B - 1: V - 1, 3: 0})]


@pytest.mark.parametrize("V", [128256, 32000, 1001])
@pytest.mark.parametrize("B", [1, 16])
def test_greedy_fast_matches_general(B, V):
    for logits, winners in _sampling_logits(B, V):
        slow = ops.greedy_sample(logits.clone(), allow_fast=False)
        fast = ops.greedy_sample(logits.clone(), allow_fast=True)
        assert torch.equal(fast, slow)
        assert torch.equal(fast.cpu(), torch_ref.greedy_sample(logits.cpu()))
        for row, idx in winners.items():
            assert int(fast[row]) == idx


@pytest.mark.parametrize("V", [128256, 32000, 1001])
@pytest.mark.parametrize("B", [1, 16])
def test_gumbel_fast_matches_general(B, V):
    seeds = torch.tensor([(b * 2654435761 + 12345) ^ (b << 40) for b in range(B)],
                         dtype=torch.int64)
    inv_t = torch.linspace(0.5, 1.5, B)
    for logits, _ in _sampling_logits(B, V):
        slow = ops.gumbel_sample(logits.clone(), inv_t.to(DEV), 0,
                                 seeds.to(DEV), allow_fast=False)
        fast = ops.gumbel_sample(logits.clone(), inv_t.to(DEV), 0,
                                 seeds.to(DEV), allow_fast=True)
        assert torch.equal(fast, slow)
        # the CPU path is the same splitmix64 Gumbel stream
        ref = ops.gumbel_sample(logits.cpu(), inv_t, 0, seeds)
        assert torch.equal(fast.cpu(), ref)
