"""csrc/logprobs.hip on the GPU against torch_ref.top_logprobs (float64), and
compute_logprobs with the kernel switched on against the torch path."""
import functools
import types

import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.engine import SamplingParams
from dynamo_amd.engine.sampling import compute_logprobs
from dynamo_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ("normal", "ascending", "equal", "ties", "masked")
# 5: below nmax; 1021: unaligned rows, V % 4 != 0, one slice; 16387: several
# slices with head and tail; 128256: the flagship vocabulary (B = 2 only)
SHAPES = [(V, B) for V in (5, 1021, 16387) for B in (1, 3, 64)] + [(128256, 2)]
# slices = 1 at 16387: one block takes the whole row in several steps and
# flushes its queue between them (at every step on the ascending row)
CASES = [(V, B, None) for V, B in SHAPES] + [(16387, 3, 1)]
SENTINEL = 777.0


def _rows(kind, B, V, g):
    if kind == "normal":
        return torch.randn(B, V, generator=g) * 3
    if kind == "ascending":     # every element passes the queue's threshold
        return (torch.arange(V, dtype=torch.float32) / 1024).repeat(B, 1)
    if kind == "equal":
        return torch.full((B, V), 1.5)
    if kind == "ties":
        # eight levels: runs of equal logits straddle the n-th place and
        # every slice boundary
        return torch.randint(0, 8, (B, V), generator=g).float()
    x = torch.full((B, V), float("-inf"))
    for b in range(B):
        x[b, torch.randperm(V, generator=g)[:3]] = torch.randn(3, generator=g)
    return x


@functools.lru_cache(maxsize=None)
def _inputs(kind, V, B):
    """(logits, sampled, float64 logprobs, error of fp32 torch.log_softmax)"""
    g = torch.Generator().manual_seed(V * 131 + B)
    x = _rows(kind, B, V, g)
    sampled = torch.randint(0, V, (B,), generator=g).to(torch.int32)
    ref = torch.log_softmax(x.double(), -1)
    old = torch.log_softmax(x.to(DEV), -1).cpu().double()
    fin = torch.isfinite(ref)
    return x, sampled, ref, float((old - ref)[fin].abs().max())


@functools.lru_cache(maxsize=None)
def _bound(V):
    """4 e, e = the largest error of fp32 torch.log_softmax, the path the
    kernel replaces, against float64 over every input of this file at V; the
    factor is for another, equally valid fp32 summation order. Measured on
    MI355X, e / the kernel's own worst error: V = 5: 7.97e-07 / 4.82e-07,
    1021: 1.96e-06 / 7.04e-07, 16387: 2.17e-06 / 9.75e-07, 128256: 1.90e-06 /
    1.01e-06 (profiles/README.md, "Fused logprobs")."""
    return 4 * max(_inputs(k, v, b)[3] for k in KINDS for v, b in SHAPES
                   if v == V)


@pytest.mark.parametrize("nmax", [1, 5, 20])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,B,slices", CASES)
def test_top_logprobs_kernel(V, B, slices, kind, nmax):
    x, sampled, ref, _ = _inputs(kind, V, B)
    want = torch.tensor([(nmax, 0, max(1, nmax // 2))[b % 3]
                         for b in range(B)], dtype=torch.int32)

    def filled(dev):
        return (torch.full((B,), SENTINEL, device=dev),
                torch.full((B, nmax), SENTINEL, device=dev),
                torch.full((B, nmax), -7, dtype=torch.int32, device=dev))
    token_lp, top_lp, top_ids = (t.cpu() for t in ops.top_logprobs(
        x.to(DEV), sampled.to(DEV), want.to(DEV), nmax, filled(DEV),
        slices=slices))
    r_token, r_lp, r_ids = torch_ref.top_logprobs(x, sampled, want, nmax,
                                                  filled("cpu"))
    # ids exactly; the sentinel and -inf exactly where the reference has them
    assert torch.equal(top_ids, r_ids)
    assert torch.equal(top_lp == SENTINEL, r_lp == SENTINEL)
    assert torch.equal(token_lp == SENTINEL, r_token == SENTINEL)
    inf = torch.isinf(r_lp)
    assert torch.equal(top_lp[inf], r_lp[inf])
    assert torch.equal(torch.isinf(token_lp), torch.isinf(r_token))
    # finite values against float64
    exact = ref.gather(1, r_ids.clamp(min=0).long())
    exact_tok = ref.gather(1, sampled.long().unsqueeze(1)).squeeze(1)
    fin = torch.isfinite(top_lp) & (r_lp != SENTINEL)
    fin_tok = torch.isfinite(token_lp) & (r_token != SENTINEL)
    err = max((top_lp.double() - exact)[fin].abs().max().item(),
              (token_lp.double() - exact_tok)[fin_tok].abs().max().item()
              if fin_tok.any() else 0.0)
    print(f"V={V} B={B} {kind} nmax={nmax}: kernel error {err:.3e}, "
          f"bound {_bound(V):.3e}")
    assert err <= _bound(V)


def test_compute_logprobs_kernel_path():
    B, V = 16, 16387
    logits = _inputs("normal", V, 64)[0][:B].to(DEV).contiguous()
    sampled = ops.greedy_sample(logits)
    want = [(5, 0, 2, 20)[b % 4] for b in range(B)]
    reqs = [types.SimpleNamespace(sampling=SamplingParams(logprobs=n))
            for n in want]
    try:
        ops.set_logprobs_kernel(False)
        off = compute_logprobs(logits, sampled, reqs)
        ops.set_logprobs_kernel(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        on = compute_logprobs(logits, sampled, reqs)
        peak = torch.cuda.max_memory_allocated() - before
    finally:
        ops.set_logprobs_kernel(None)
    assert peak < B * V * 4, f"{peak} bytes allocated: a [B, V] temporary?"
    for a, b, n in zip(on, off, want):
        if not n:
            assert a is None and b is None
            continue
        assert [t for t, _ in a["top"]] == [t for t, _ in b["top"]]
        assert len(a["top"]) == n
        for u, v in zip([a["token_logprob"]] + [p for _, p in a["top"]],
                        [b["token_logprob"]] + [p for _, p in b["top"]]):
            assert abs(u - v) <= _bound(V)
