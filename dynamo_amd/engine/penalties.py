"""Per-request logit processors between the model's logits and sampling:
repetition / presence / frequency penalties, logit_bias and min_p
(SamplingParams; kernels in csrc/logits_process.hip, semantics at
ops/torch_ref.apply_logit_processors).

The penalties need, per request, which tokens its prompt holds and how often
each token occurs in its output. PenaltyBank keeps that on the device as one
int32 per (slot, token), allocated on the first request that needs it. The
counts are a function of the request's tokens alone: each request has a
cursor into all_tokens, and whatever lies past it is folded in before the
request is sampled - one token per step in steady state, everything at once
for a new request, one that returns from preemption or one whose prefill ran
on another worker. There is no other way to restore a row.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from dynamo_amd import ops
from .scheduler import Request


class PenaltyBank:
    def __init__(self, num_slots: int):
        self.num_slots = num_slots
        self.counts: Optional[torch.Tensor] = None   # [num_slots, V] int32
        self._free = list(range(num_slots - 1, -1, -1))

    def release(self, req: Request):
        """The request finished, was aborted or was preempted: its row goes
        back to the pool (and is zeroed when it is handed out again)."""
        if req.penalty_slot >= 0:
            self._free.append(req.penalty_slot)
            req.penalty_slot = -1
            req.penalty_cursor = 0

    def _fold(self, reqs: List[Request], V: int, device):
        """Give every request that needs counts a row and bring the rows up
        to date with all_tokens, in one launch."""
        slots: List[int] = []
        tokens: List[int] = []
        flags: List[int] = []
        for r in reqs:
            if not r.sampling.needs_counts:
                continue
            if r.penalty_slot < 0:
                if self.counts is None:
                    self.counts = torch.zeros(self.num_slots, V,
                                              dtype=torch.int32, device=device)
                if not self._free:
                    raise RuntimeError(
                        "no free penalty slot: more penalised requests are "
                        f"live than max_num_seqs = {self.num_slots}")
                r.penalty_slot = self._free.pop()
                r.penalty_cursor = 0
                self.counts[r.penalty_slot].zero_()
            new = r.all_tokens[r.penalty_cursor:]
            if new:
                n_prompt = len(r.prompt_tokens) - r.penalty_cursor
                slots.extend([r.penalty_slot] * len(new))
                tokens.extend(new)
                flags.extend(1 if i < n_prompt else 0
                             for i in range(len(new)))
                r.penalty_cursor += len(new)
        if tokens:
            e = torch.tensor([slots, tokens, flags],
                             dtype=torch.int32).to(device)
            ops.penalty_fold(self.counts, e[0], e[1], e[2])

    def process(self, logits: torch.Tensor, reqs: List[Request]):
        """Apply the rows' logit processors to logits [n, V] (fp32,
        contiguous) in place; reqs[i] is sampled from row i next. This check
        is all that happens when every row's parameters are neutral."""
        if any(r.sampling.has_logit_processors for r in reqs):
            self._process(logits, reqs)

    @torch.inference_mode()   # both callers' tensors, one mode for the bank
    def _process(self, logits: torch.Tensor, reqs: List[Request]):
        V = logits.shape[1]
        dev = logits.device
        self._fold(reqs, V, dev)
        params, slots = [], []
        off, ids, vals = [0], [], []
        for r in reqs:
            sp = r.sampling
            params.append((sp.repetition_penalty, sp.presence_penalty,
                           sp.frequency_penalty, sp.min_p, sp.temperature))
            slots.append(r.penalty_slot)
            ids.extend(sp.logit_bias.keys())
            vals.extend(sp.logit_bias.values())
            off.append(len(ids))
        bias = None
        if ids:
            bias = (torch.tensor(off, dtype=torch.int32).to(dev),
                    torch.tensor(ids, dtype=torch.int32).to(dev),
                    torch.tensor(vals, dtype=torch.float32).to(dev))
        ops.apply_logit_processors(
            logits, self.counts,
            torch.tensor(slots, dtype=torch.int32).to(dev),
            torch.tensor(params, dtype=torch.float32).to(dev), bias)


def validate_request(sp, prompt_tokens: List[int], vocab_size: int):
    """ValueError for token ids the kernels would have to skip: a logit_bias
    key, or a prompt token of a penalised request, outside the vocabulary."""
    bad = [k for k in sp.logit_bias if not 0 <= k < vocab_size]
    if bad:
        raise ValueError(
            f"logit_bias names token id {bad[0]}, which is outside the "
            f"vocabulary [0, {vocab_size})")
    if sp.needs_counts:
        bad = [t for t in prompt_tokens if not 0 <= t < vocab_size]
        if bad:
            raise ValueError(
                f"prompt token id {bad[0]} is outside the vocabulary "
                f"[0, {vocab_size}): a request with repetition, presence or "
                "frequency penalties needs valid ids")
