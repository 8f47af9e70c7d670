"""Top-k / top-p sampler test cases with teeth (plain helper, not a conftest).

The sampler tests of tests/test_gpu_kernels.py run one shape of `randn * 3`
rows and check membership in a keep set. On such rows a keep set a few
tokens too large on a flat row, a nucleus taken over the wrong distribution
or a token id of -1 for top_p = 0 all pass. This module builds rows and parameters whose keep set under
`torch_ref.topkp_keep_mask` is unambiguous, so that a kernel can be held to
it exactly, and asserts that on the CPU while it builds them. It is shared by
tests/test_sampler_cases_cpu.py and tests/test_gpu_sampler_filters.py.

Rows (values are laid out by rank, then scattered through one fixed
permutation per V, so rank r sits at index perm[r]):
    ladder      -1e-4 * rank: probabilities closer together than any
                absolute resolution on [0, 1] can tell apart
    peaked      randn * 3
    ties        randn * 3 with the value of rank kt copied to the ranks
                kt-1 .. kt+2 (ranks counted from 1): a four-way tie across
                the top-k boundary. kt is the row's own k for k in
                {5, 50, V-1} (clipped to the row) and 5 otherwise, so the
                maximum stays unique and top_k = 1 has one right answer
    masked      randn * 3 with -inf on a random 70 % of entries, as min_p
                leaves a row
    masked_few  three finite entries: fewer than k = 5, 50, V-1
    onehot      randn with one logit 100 above the rest
    max_first   peaked, the maximum moved to index 0
    max_last    peaked, the maximum moved to index V-1

Parameters, all crossed with every row kind:
    k in {-3, 0, 1, 5, 50, V-1, V, V+5} at top_p = 1
    top_p at a shallow, a middle and a deep rank with k = 0
    k in {1, 5, 50} with a top_p on the renormalised survivors

Margins, asserted here and never skipped at run time (a draw that misses one
is redrawn from the next seed):
    * at a top-k boundary the k-th and (k+1)-th probabilities are exactly
      tied or differ by a relative 5e-5 (__expf is good to ~1e-6: 50x)
    * a top_p is the midpoint (cum[j-1] + cum[j]) / 2 of the reference's
      cumulative mass over the top-k survivors at a rank j (cum[-1] = 0), so
      ranks 0 .. j are kept; both neighbours are >= 1e-5 away (an fp32 mass
      carries ~2e-6: __expf plus a tree sum of terms totalling <= 1), and
      ranks j and j+1 are not tied, so the sort in _filter_topk_topp and the
      tie rule of the reference agree
    * for k in {5, 50} crossed with top_p on the ORDER_KINDS rows, top-k
      followed by the nucleus of the survivors differs from top-k
      intersected with the nucleus of the full row. For k = 1 both are the
      argmax, whatever the row; there top_p is half the survivor's mass.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from dynamo_amd.ops import torch_ref

NEG_INF = float("-inf")
VOCABS = (511, 1000, 8192)      # < one block; not a multiple of 4; a ladder
#                                 the old 6e-8 resolution cannot resolve
BIG_V = 128256                  # one peaked group at the flagship vocabulary
MAX_ROWS = 16                   # rows per launch
KIND_NAMES = ("ladder", "peaked", "ties", "masked", "masked_few", "onehot",
              "max_first", "max_last")
# kinds on which k in {5, 50} crossed with top_p must tell the two orders of
# the filters apart (masked_few: top-k keeps every finite entry; onehot: the
# nucleus is the one token either way)
ORDER_KINDS = ("ladder", "peaked", "ties", "masked", "max_first", "max_last")
INV_TEMPS = (0.5, 1.0, 4.0)
K_GAP = 5e-5                    # relative, between the k-th and (k+1)-th prob
P_MARGIN = 1e-5                 # absolute, from top_p to either neighbour
FEW = 3                         # finite entries of a masked_few row
P_DEPTHS = ("shallow", "middle", "deep")
RANGE_PS = (0.0, 1e-6, 0.999999)


def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(_seed(*key))


@functools.lru_cache(maxsize=None)
def perm(V: int) -> torch.Tensor:
    return torch.randperm(V, generator=_gen("sampler_perm", V))


def param_list(V: int) -> List[Tuple[int, Optional[str]]]:
    """(k, depth): depth None is top_p = 1, one of P_DEPTHS is the rank the
    midpoint aims for, and "cross" is the first of middle, deep and shallow
    at which the two orders of the filters give different sets."""
    out = [(k, None) for k in (-3, 0, 1, 5, 50, V - 1, V, V + 5)]
    out += [(0, d) for d in P_DEPTHS]
    out += [(k, "cross") for k in (1, 5, 50)]
    return out


# --------------------------------------------------------------------------
# rows
# --------------------------------------------------------------------------
def _by_rank(V: int, gen, scale: float = 3.0) -> torch.Tensor:
    return (torch.randn(V, generator=gen) * scale).sort(
        descending=True).values


def tie_rank(k: int, V: int) -> int:
    return k if k in (5, 50, V - 1) else 5


def build_row(kind: str, V: int, k: int, attempt: int) -> torch.Tensor:
    """One fp32 row of `kind`; `k` only places the tie of a "ties" row."""
    gen = _gen("sampler_row", kind, V, k if kind == "ties" else 0, attempt)
    if kind == "ladder":
        vals = -1e-4 * torch.arange(V, dtype=torch.float32)
    elif kind == "ties":
        vals = _by_rank(V, gen)
        kt = tie_rank(k, V)
        vals[max(0, kt - 2):min(V, kt + 2)] = vals[kt - 1]
    elif kind == "masked":
        vals = torch.randn(V, generator=gen) * 3
        drop = torch.randperm(V, generator=gen)[:int(0.7 * V)]
        vals[drop] = NEG_INF
        vals = vals.sort(descending=True).values
    elif kind == "masked_few":
        vals = torch.full((V,), NEG_INF)
        vals[:FEW] = _by_rank(FEW, gen)
    elif kind == "onehot":
        vals = _by_rank(V, gen, 1.0)
        vals[0] = vals[1] + 100.0
    else:
        vals = _by_rank(V, gen)
    row = torch.empty(V, dtype=torch.float32)
    row[perm(V)] = vals.float()
    if kind in ("max_first", "max_last"):
        at = 0 if kind == "max_first" else V - 1
        top = int(row.argmax())
        row[[at, top]] = row[[top, at]]
    return row


# --------------------------------------------------------------------------
# margins
# --------------------------------------------------------------------------
def _sorted_probs(row: torch.Tensor, k: int):
    """-> (logits sorted descending, their float64 softmax over the top-k
    survivors, the number of survivors)."""
    V = row.numel()
    srt = row.double().sort(descending=True).values
    n = int(torch.isfinite(srt).sum())
    if 0 < k < V:
        n = min(n, int((srt >= srt[k - 1]).sum()))
    surv = srt.clone()
    surv[n:] = NEG_INF
    return srt, torch.softmax(surv, -1), n


def k_boundary_ok(row: torch.Tensor, k: int) -> bool:
    """k-th and (k+1)-th probabilities exactly tied, or K_GAP apart."""
    V = row.numel()
    if not 0 < k < V:
        return True
    srt = row.double().sort(descending=True).values
    a, b = float(srt[k - 1]), float(srt[k])
    if a == b or b == NEG_INF:
        return True
    return 1.0 - float(torch.exp(torch.tensor(b - a, dtype=torch.float64))) \
        >= K_GAP


def pick_top_p(row: torch.Tensor, k: int, depth: str) -> Optional[float]:
    """The midpoint top_p (as the float32 the kernel is given) at the
    feasible rank nearest the one `depth` aims for, or None if no rank of
    this row is feasible."""
    srt, prob, n = _sorted_probs(row, k)
    cum = prob.cumsum(-1)
    before = cum - prob
    mid = (before + cum) / 2
    ok = prob / 2 >= 2 * P_MARGIN           # twice the margin asked for
    ok[:-1] &= srt[:-1] != srt[1:]          # ranks j and j+1 not tied
    ok[n - 1:] = False                      # something must be dropped
    if not bool(ok.any()):
        return None
    want = {"shallow": min(2, n - 2),
            "middle": int((cum < 0.5).sum()),
            "deep": int((cum < 0.95).sum())}[depth]
    cand = ok.nonzero().flatten()
    j = int(cand[(cand - want).abs().argmin()])
    p = float(torch.tensor(float(mid[j]), dtype=torch.float32))
    assert p - float(before[j]) >= P_MARGIN, (p, j)
    assert float(cum[j]) - p >= P_MARGIN, (p, j)
    return p


def sequential_and_intersected(row, k: int, p: float):
    """The keep set of top-k followed by the nucleus of the survivors, and
    of top-k intersected with the nucleus of the full row."""
    row = row[None]
    seq = torch_ref.topkp_keep_mask(row, k, p)[0]
    both = (torch_ref.topkp_keep_mask(row, k, 1.0)[0]
            & torch_ref.topkp_keep_mask(row, 0, p)[0])
    return seq, both


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
@dataclass
class Group:
    """At most MAX_ROWS rows that go through the kernel in one launch."""
    V: int
    labels: List[str]            # "kind k=.. p=.."
    kinds: List[str]
    logits: torch.Tensor         # [B, V] fp32
    top_k: torch.Tensor          # [B] int32
    top_p: torch.Tensor          # [B] fp32
    mask: torch.Tensor           # [B, V] bool, torch_ref.topkp_keep_mask
    argmax: torch.Tensor         # [B] int64, lowest index of the maximum

    @property
    def B(self) -> int:
        return len(self.labels)


def _one_case(kind: str, V: int, k: int, depth: Optional[str]):
    """-> (row, top_p) from the first draw that meets every margin."""
    for attempt in range(64):
        row = build_row(kind, V, k, attempt)
        if not k_boundary_ok(row, k):
            continue
        if depth is None:
            return row, 1.0
        if depth != "cross":
            p = pick_top_p(row, k, depth)
            if p is not None:
                return row, p
        else:
            must_differ = k in (5, 50) and kind in ORDER_KINDS
            for d in ("middle", "deep", "shallow"):
                p = pick_top_p(row, k, d)
                if p is None:
                    continue
                if must_differ:
                    seq, both = sequential_and_intersected(row, k, p)
                    if bool((seq == both).all()):
                        continue
                return row, p
        if kind in ("ladder", "masked_few") or k == 1:
            break                    # no other draw will differ
    assert not (k in (5, 50) and kind in ORDER_KINDS), (kind, V, k)
    # one survivor (k = 1), or nothing droppable at the margin: the midpoint
    # below the first token, which keeps the argmax alone
    row = build_row(kind, V, k, 0)
    assert k_boundary_ok(row, k)
    _, prob, _ = _sorted_probs(row, k)
    assert float(prob[0]) / 2 >= P_MARGIN
    return row, float(torch.tensor(float(prob[0]) / 2, dtype=torch.float32))


def _group(V: int, rows, labels, kinds, ks, ps) -> Group:
    logits = torch.stack(rows)
    assert not bool(logits.isnan().any())
    top_k = torch.tensor(ks, dtype=torch.int32)
    top_p = torch.tensor(ps, dtype=torch.float32)
    return Group(V, labels, kinds, logits, top_k, top_p,
                 torch_ref.topkp_keep_mask(logits, top_k, top_p),
                 logits.argmax(-1))


def _groups(V: int, specs) -> List[Group]:
    """specs: (kind, k, row, p) in order; cut into launches of MAX_ROWS."""
    out = []
    for i in range(0, len(specs), MAX_ROWS):
        part = specs[i:i + MAX_ROWS]
        out.append(_group(
            V, [s[2] for s in part],
            [f"{s[0]} k={s[1]} p={s[3]:.9g}" for s in part],
            [s[0] for s in part], [s[1] for s in part],
            [s[3] for s in part]))
    return out


@functools.lru_cache(maxsize=None)
def exact_groups(V: int) -> Tuple[Group, ...]:
    """The cases a kernel must match exactly. BIG_V holds peaked rows only."""
    kinds = ("peaked",) if V == BIG_V else KIND_NAMES
    specs = []
    for kind in kinds:
        for k, depth in param_list(V):
            row, p = _one_case(kind, V, k, depth)
            specs.append((kind, k, row, p))
    return tuple(_groups(V, specs))


@functools.lru_cache(maxsize=None)
def range_groups(V: int) -> Tuple[Group, ...]:
    """Out-of-range parameters: top_p in RANGE_PS on every kind, and k above
    the number of finite entries. A sample must index a finite logit, and
    for top_p <= 1e-6 it must be the argmax, which these rows keep unique
    and more likely than 2e-6."""
    specs = []
    for kind in KIND_NAMES:
        row = build_row(kind, V, 0, 0)
        _, prob, _ = _sorted_probs(row, 0)
        assert float(prob[0]) > 2e-6 and float(prob[0]) > float(prob[1])
        specs += [(kind, 0, row, p) for p in RANGE_PS]
    few = build_row("masked_few", V, 0, 0)
    specs += [("masked_few", k, few, p) for k in (5, 50, V - 1)
              for p in (1.0, 0.0)]
    return tuple(_groups(V, specs))


def topk1_rows(g: Group) -> List[int]:
    """Rows of a group with top_k = 1 on a ladder or ties row."""
    return [b for b in range(g.B)
            if int(g.top_k[b]) == 1 and g.kinds[b] in ("ladder", "ties")]
