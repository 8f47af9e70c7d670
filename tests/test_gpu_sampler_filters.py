"""The fused top-k / top-p sampler (`topkp_sample_kernel`) against the exact
keep set of `torch_ref.topkp_keep_mask`, on the cases of
tests/sampler_cases.py (margins asserted on the CPU by
tests/test_sampler_cases_cpu.py).

* exact distribution: `topkp_sample(logits, ...)` equals
  `gumbel_sample(masked, ...)` token for token, where `masked` is `logits`
  with -inf outside the reference mask. Both kernels draw from the same
  splitmix64 stream and `gumbel_sample` is held bit-for-bit to the CPU stream
  elsewhere, so this pins the keep set and the sampling inside it. 16 seeds
  through the scalar `seed` path and one pass of `row_seeds` with negative
  and repeated seeds; the inverse temperatures 0.5, 1 and 4 rotate over the
  rows with the seed, so every row is sampled at each of them and the keep
  set may not depend on temperature. A last pass at an inverse temperature
  of -1e6 returns the kept token with the lowest logit (see _sample), so a
  set that is one token too large or too small fails for certain and not
  only when a seed happens to draw that token.
* membership: every sample is in the reference mask, with no widening.
* top_k = 1 on ladder and ties rows returns the argmax for every seed.
* range: top_p in {0, 1e-6, 0.999999} and k above the number of finite
  entries. No equality; every sample lies in [0, V), indexes a finite logit,
  and is the argmax for top_p <= 1e-6.

Each vocabulary size is sampled once per session and shared by its tests.
"""
import functools

import pytest
import torch

from dynamo_amd import ops
from tests import sampler_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = tuple(s * 7919 + 13 for s in range(16))
FLOOR_SEED = 20240229
ALL_V = sc.VOCABS + (sc.BIG_V,)


def _inv_temp(B: int, shift: int) -> torch.Tensor:
    return torch.tensor([sc.INV_TEMPS[(b + shift) % 3] for b in range(B)],
                        dtype=torch.float32, device=DEV)


def _row_seeds(B: int) -> torch.Tensor:
    base = [11, -5, 1 << 62, 0, 42, 42, 7, -(1 << 60), -1, 42]
    return torch.tensor([base[b % len(base)] for b in range(B)],
                        dtype=torch.int64, device=DEV)


def _sample(g: sc.Group, masked: bool, floor: bool = True):
    """-> int64 [17 or 18, B] on the CPU: one row per scalar seed, then the
    row_seeds pass, then the floor pass. `masked` runs gumbel_sample on the
    reference's set.

    The floor pass makes the edge of the keep set deterministic: at an
    inverse temperature of -1e6 the Gumbel noise (17 at the most) is small
    against the scaled logit gap at a top-k boundary or on the ladder
    (>= 50), so the sample is the kept token with the *lowest* logit. One
    token too many or too few in the set changes it, where a random draw
    would have to hit that token. Its reference masks with +inf, and rows
    with -inf entries sit the pass out (both sides report the argmax): a
    -inf logit that top-k alone lets through is never drawn at a positive
    temperature but would win this one."""
    logits = g.logits.to(DEV)
    mask = g.mask.to(DEV)
    tk, tp = g.top_k.to(DEV), g.top_p.to(DEV)
    outs = []
    for i, seed in enumerate(SEEDS + (None,)):
        inv_t = _inv_temp(g.B, i)
        rows = _row_seeds(g.B) if seed is None else None
        if masked:
            outs.append(ops.gumbel_sample(
                logits.masked_fill(~mask, float("-inf")), inv_t, seed or 0,
                rows))
        else:
            outs.append(ops.topkp_sample(logits, inv_t, tk, tp, seed or 0,
                                         rows))
    if floor:
        inv_t = torch.full((g.B,), -1e6, device=DEV)
        if masked:
            out = ops.gumbel_sample(logits.masked_fill(~mask, float("inf")),
                                    inv_t, FLOOR_SEED)
        else:
            out = ops.topkp_sample(logits, inv_t, tk, tp, FLOOR_SEED)
        outs.append(torch.where(torch.isinf(logits).any(-1),
                                g.argmax.to(DEV, torch.int32), out))
    return torch.stack(outs).long().cpu()


@functools.lru_cache(maxsize=None)
def _exact(V: int):
    """[(group, topkp_sample's tokens, gumbel_sample's on the masked row)]"""
    return [(g, _sample(g, False), _sample(g, True))
            for g in sc.exact_groups(V)]


@functools.lru_cache(maxsize=None)
def _ranges(V: int):
    return [(g, _sample(g, False, floor=False)) for g in sc.range_groups(V)]


def _report(bad):
    return f"{len(bad)} rows, first: " + "; ".join(bad[:40])


@pytest.mark.parametrize("V", ALL_V)
def test_equals_gumbel_on_the_reference_set(V):
    bad = []
    for g, got, want in _exact(V):
        for b in (got != want).any(0).nonzero().flatten().tolist():
            s = int((got[:, b] != want[:, b]).nonzero()[0])
            bad.append(f"{g.labels[b]} keeps {int(g.mask[b].sum())}: pass {s}"
                       f" gave {int(got[s, b])}, reference {int(want[s, b])}")
    assert not bad, _report(bad)


@pytest.mark.parametrize("V", ALL_V)
def test_every_sample_is_in_the_reference_set(V):
    bad = []
    for g, got, _ in _exact(V):
        inside = (got >= 0) & (got < V)
        inside &= g.mask.gather(1, got.clamp(0, V - 1).T).T
        for b in (~inside).any(0).nonzero().flatten().tolist():
            s = int((~inside[:, b]).nonzero()[0])
            bad.append(f"{g.labels[b]} keeps {int(g.mask[b].sum())}: pass {s}"
                       f" gave {int(got[s, b])}")
    assert not bad, _report(bad)


@pytest.mark.parametrize("V", sc.VOCABS)
def test_top_k_1_is_the_argmax(V):
    bad, n = [], 0
    for g, got, _ in _exact(V):
        for b in sc.topk1_rows(g):
            n += 1
            if not bool((got[:, b] == g.argmax[b]).all()):
                bad.append(f"{g.labels[b]}: {sorted(set(got[:, b].tolist()))}"
                           f", argmax {int(g.argmax[b])}")
    assert n >= 4
    assert not bad, _report(bad)


@pytest.mark.parametrize("V", sc.VOCABS)
def test_out_of_range_parameters(V):
    bad = []
    for g, got in _ranges(V):
        inside = (got >= 0) & (got < V)
        finite = torch.isfinite(g.logits).gather(1, got.clamp(0, V - 1).T).T
        ok = inside & finite
        greedy = (g.top_p <= 1e-6)[None, :]
        ok &= ~greedy | (got == g.argmax[None, :])
        for b in (~ok).any(0).nonzero().flatten().tolist():
            s = int((~ok[:, b]).nonzero()[0])
            bad.append(f"{g.labels[b]}: pass {s} gave {int(got[s, b])}, "
                       f"argmax {int(g.argmax[b])}")
    assert not bad, _report(bad)
