"""csrc/logits_process.hip on the GPU against ops/torch_ref.py: the fold
kernel against a Counter, the apply kernel row by row (vector path and scalar
path, aligned and unaligned rows), and the engine's two call sites."""
import collections
import math

import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS
from dynamo_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# 1003: V % 4 != 0, so every row after the first starts off a 16-byte
# boundary; 16389: one element past four full 512 x 8 x 4 sweeps, plus a
# scalar tail
VOCABS = [1024, 1003, 16389]
# seeds at which the min_p and top-2 margins asserted below hold (found on
# the CPU, on the reference)
SEEDS = {1024: 2, 1003: 2, 16389: 0}
S = 7                      # bank slots
REP, PRES, FREQ = 1.3, 0.4, 0.7
MIN_P, TEMP = 0.1, 0.7
NEUTRAL = (1.0, 0.0, 0.0, 0.0, 0.0)
EPS = 2.0 ** -23


def _entries(V, g):
    """{slot: (prompt tokens, output tokens)}: duplicates in both, counts of
    0, 1 and many, and the first and last ids of the row (the scalar head and
    tail of the vector path)."""
    def draw(n, pool=None):
        if pool is None:
            return torch.randint(0, V, (n,), generator=g).tolist()
        return [pool[i] for i in
                torch.randint(0, len(pool), (n,), generator=g).tolist()]
    edges = [0, 1, 2, 3, V - 4, V - 3, V - 2, V - 1]
    out = {}
    for slot in (0, 1, 2, 3, 5):
        pool = draw(12) + edges[slot % 2::2]
        prompt = draw(50) + draw(10, pool) + edges[::3]
        output = draw(60, pool) + [pool[0]] * 40 + draw(5)
        out[slot] = (prompt, output)
    return out


def _fold_tensors(entries, device):
    rows = [(s, t, 1) for s, (p, _) in entries.items() for t in p]
    rows += [(s, t, 0) for s, (_, o) in entries.items() for t in o]
    e = torch.tensor(rows, dtype=torch.int32).t().contiguous()
    return [x.to(device) for x in e]


class Case:
    """The seven rows of the issue plus a guard row, for one V."""

    def __init__(self, V):
        self.V = V
        g = torch.Generator().manual_seed(SEEDS[V])
        self.entries = _entries(V, g)
        # slot 4 held another request (slot 5's tokens), was cleared and now
        # holds what slot 1 holds; slot 6 is never used
        self.cpu_bank = torch.zeros(S, V, dtype=torch.int32)
        torch_ref.penalty_fold(self.cpu_bank,
                               *_fold_tensors(self.entries, "cpu"))
        self.cpu_bank[4] = self.cpu_bank[1]
        lg = torch.randn(8, V, generator=g) * 3.0 + 0.7
        lg[6] = lg[2]
        self.logits = lg
        #                 rep  pres  freq  min_p temp
        self.params = torch.tensor([
            NEUTRAL,                          # 0 neutral, on a used slot
            NEUTRAL,                          # 1 bias only, no slot
            (REP, 0.0, 0.0, 0.0, 0.0),        # 2 repetition only
            (1.0, PRES, FREQ, 0.0, 1.0),      # 3 frequency and presence
            (REP, -PRES, FREQ, MIN_P, TEMP),  # 4 everything
            (1.0, 0.0, 0.0, MIN_P, TEMP),     # 5 min_p, no slot
            (REP, 0.0, 0.0, 0.0, 0.0),        # 6 = row 2 on the cleared slot
            NEUTRAL,                          # 7 guard
        ], dtype=torch.float32)
        self.slots = torch.tensor([0, -1, 1, 2, 3, -1, 4, -1],
                                  dtype=torch.int32)
        ids1 = torch.randperm(V, generator=g)[:37].tolist() + [0, V - 1]
        ids4 = self.entries[3][1][:20] + [1, V - 2]
        bias = {1: {t: 5.0 - 0.37 * i for i, t in enumerate(dict.fromkeys(ids1))},
                4: {t: -3.0 + 0.27 * i for i, t in enumerate(dict.fromkeys(ids4))}}
        off, ids, vals = [0], [], []
        for b in range(8):
            ids += list(bias.get(b, {}))
            vals += list(bias.get(b, {}).values())
            off.append(len(ids))
        self.bias = (torch.tensor(off, dtype=torch.int32),
                     torch.tensor(ids, dtype=torch.int32),
                     torch.tensor(vals, dtype=torch.float32))
        self.bias_dense = torch.zeros(8, V)
        for b, d in bias.items():
            for t, v in d.items():
                self.bias_dense[b, t] = v
        # the reference, once; and the same without min_p (the values the
        # threshold is taken on)
        self.ref = torch_ref.apply_logit_processors(
            self.logits.clone(), self.cpu_bank, self.slots, self.params,
            self.bias)
        p0 = self.params.clone()
        p0[:, 3] = 0.0
        self.ref_unmasked = torch_ref.apply_logit_processors(
            self.logits.clone(), self.cpu_bank, self.slots, p0, self.bias)

    def tolerance(self):
        """4 * 2^-23 * (|l| + |freq| * cnt + |pres| + |bias|) per element."""
        cnt = torch.zeros(8, self.V)
        for b, s in enumerate(self.slots.tolist()):
            if s >= 0:
                cnt[b] = (self.cpu_bank[s] >> 1).float()
        freq = self.params[:, 2:3].abs()
        pres = self.params[:, 1:2].abs()
        return 4 * EPS * (self.logits.abs() + freq * cnt + pres
                          + self.bias_dense.abs())


_cases = {}


def case(V) -> Case:
    if V not in _cases:
        _cases[V] = Case(V)
    return _cases[V]


def gpu_bank(c: Case):
    """The bank as the engine would have built it: folds, a cleared slot, a
    second fold into it."""
    bank = torch.zeros(S, c.V, dtype=torch.int32, device=DEV)
    ops.penalty_fold(bank, *_fold_tensors(c.entries, DEV))
    ops.penalty_fold(bank, *_fold_tensors({4: c.entries[5]}, DEV))
    bank[4].zero_()
    ops.penalty_fold(bank, *_fold_tensors({4: c.entries[1]}, DEV))
    return bank


@pytest.mark.parametrize("V", VOCABS)
def test_reference_margins(V):
    """What the GPU comparisons below rely on, asserted on the reference."""
    c = case(V)
    thr = math.log(MIN_P)
    for b in (4, 5):
        u = c.ref_unmasked[b]
        z = (u - u.max()) / TEMP
        assert (z - thr).abs().min() > 1e-3
        masked = torch.isinf(c.ref[b])
        assert masked.any() and (~masked).sum() >= 2
        assert torch.equal(masked, z < thr)
    for b in range(8):
        top2 = torch.topk(c.ref[b], 2).values
        assert top2[0] - top2[1] > 1e-3
    cnt = c.cpu_bank[2] >> 1
    assert (cnt == 0).any() and (cnt == 1).any() and cnt.max() >= 40
    assert not torch.equal(c.ref[2], c.logits[2])


@pytest.mark.parametrize("V", VOCABS)
def test_fold_matches_counter(V):
    c = case(V)
    two = {s: c.entries[s] for s in (1, 3)}
    bank = torch.zeros(S, V, dtype=torch.int32, device=DEV)
    ops.penalty_fold(bank, *_fold_tensors(two, DEV))
    # ids outside the bank are skipped, not folded elsewhere
    bad = torch.tensor([[1, 1, S, -1], [V, -1, 0, 0], [0, 1, 0, 1]],
                       dtype=torch.int32, device=DEV)
    ops.penalty_fold(bank, bad[0], bad[1], bad[2])
    got = bank.cpu()
    for s in range(S):
        if s not in two:
            assert not got[s].any()
            continue
        prompt, output = two[s]
        cnt = collections.Counter(output)
        assert len(prompt) > len(set(prompt)) and max(cnt.values()) >= 40
        want = torch.zeros(V, dtype=torch.int32)
        for t in set(prompt):
            want[t] |= 1
        for t, n in cnt.items():
            want[t] += 2 * n
        assert torch.equal(got[s], want)


@pytest.mark.parametrize("fast", [True, False], ids=["vector", "scalar"])
@pytest.mark.parametrize("V", VOCABS)
def test_apply_matches_reference(V, fast):
    c = case(V)
    bank = gpu_bank(c)
    assert torch.equal(bank.cpu(), c.cpu_bank)
    bank_before = bank.clone()
    logits = c.logits.to(DEV)
    out = ops.apply_logit_processors(
        logits, bank, c.slots.to(DEV), c.params.to(DEV),
        tuple(t.to(DEV) for t in c.bias), allow_fast=fast)
    assert out is logits
    got = logits.cpu()
    assert torch.equal(bank, bank_before)
    # untouched rows: bit for bit
    for b in (0, 7):
        assert torch.equal(got[b].view(torch.int32),
                           c.logits[b].view(torch.int32))
    # the -inf mask is the reference's, exactly
    assert torch.equal(torch.isinf(got), torch.isinf(c.ref))
    keep = ~torch.isinf(c.ref)
    err = (got - c.ref).abs()
    tol = c.tolerance()
    worst = (err[keep] / tol[keep]).max().item()
    print(f"V={V} fast={fast}: worst |err| / bound = {worst:.3f}")
    assert (err[keep] <= tol[keep]).all()
    # the cleared slot shows no trace of its previous owner
    assert torch.equal(got[6].view(torch.int32), got[2].view(torch.int32))
    # greedy on the processed logits
    assert torch.equal(ops.greedy_sample(logits).cpu().long(),
                       c.ref.argmax(-1))


def test_bias_and_min_p_without_a_bank():
    c = case(1003)
    rows = [1, 5, 7]
    logits = c.logits[rows].to(DEV)
    off = c.bias[0]
    n1 = int(off[2] - off[1])
    bias = (torch.tensor([0, n1, n1, n1], dtype=torch.int32),
            c.bias[1][off[1]:off[2]], c.bias[2][off[1]:off[2]])
    ops.apply_logit_processors(
        logits, None, torch.full((3,), -1, dtype=torch.int32, device=DEV),
        c.params[rows].to(DEV), tuple(t.to(DEV) for t in bias))
    got = logits.cpu()
    assert torch.equal(torch.isinf(got), torch.isinf(c.ref[rows]))
    keep = ~torch.isinf(got)
    assert ((got - c.ref[rows]).abs()[keep] <= c.tolerance()[rows][keep]).all()
    assert torch.equal(got[2], c.logits[7])


# ------------------------------------------------------------------- engine
def make_engine(**kw):
    cfg = EngineConfig(model=PRESETS["tiny-llama-gpu"], device=DEV,
                       max_num_seqs=8, max_batched_tokens=512,
                       max_model_len=2048, page_size=64, kv_pool_pages=256,
                       **kw)
    return LLMEngine(cfg, seed=7)


FORCED = 77


def _mixed(engine):
    reqs = [("pen", list(range(10, 45)),
             SamplingParams(max_tokens=16, presence_penalty=1e4)),
            ("bias", [7] * 29,
             SamplingParams(max_tokens=16, logit_bias={FORCED: 100.0})),
            ("dflt", list(range(10, 45)), SamplingParams(max_tokens=16))]
    outs = {}
    for rid, p, sp in reqs:
        engine.add_request(rid, p, sp)
        outs[rid] = []
    steps = 0
    while engine.has_work():
        for so in engine.step():
            outs[so.req_id].append(so.new_token)
        steps += 1
        assert steps < 200
    return outs


def test_engine_graphs_and_eager_agree():
    fast_engine = make_engine(enable_hip_graphs=True)
    assert fast_engine.graph_runner is not None
    fast = _mixed(fast_engine)
    eager = _mixed(make_engine(enable_hip_graphs=False))
    print("fast path:", fast)
    assert fast == eager
    assert fast["bias"] == [FORCED] * 16
    assert len(set(fast["pen"])) == 16, "presence_penalty=1e4 must not repeat"
    alone = make_engine(enable_hip_graphs=True)
    alone.add_request("dflt", list(range(10, 45)),
                      SamplingParams(max_tokens=16))
    toks = []
    while alone.has_work():
        toks += [so.new_token for so in alone.step()]
    assert toks == fast["dflt"], "a default request is untouched by neighbours"
    assert alone.penalties.counts is None
    assert fast_engine.penalties.counts is not None
