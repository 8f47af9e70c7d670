"""MoE test cases with teeth (plain helper, not a conftest).

The older MoE tests run one grouped-GEMM shape at rtol = atol = 2e-2 and one
random gating case against `torch.topk`; the only test of `MoEMLP.forward`
counts generated tokens. A token sent to the wrong expert, a gate weight
paired with the wrong row, a row that is never written or a dropped k chunk
all pass. This module holds the cases, the fp64 references, the bounds and
the reference mutations shared by tests/test_moe_reference_cpu.py (which shows
on the CPU that each bound rejects each mutation) and tests/test_gpu_moe.py.

Grouped GEMM
    x [T, D] bf16 gathered by expert, w [E, N, D] bf16, counts [E];
    ref[r, n] = sum_d x[r, d] w[e(r), n, d] and A[r, n] = sum_d |x| |w|, fp64.
    x and w are randn, so outputs are O(sqrt(D)) and an all-zero row fails.
    Bound, per element: |out - ref| <= 2^-8 |ref| + 2^-12 A. One bf16 output
    rounding is <= 2^-9 relative; fp32 accumulation in any order is
    <= D 2^-24 A <= 2^-13 A for D <= 2048 (every case keeps D <= 2048); both
    terms are doubled for margin. The bound is never tuned to a kernel.

Gating
    Logits live on a grid of multiples of 1/8, so equal values are exactly
    equal and unequal ones are at least e^(1/8) apart in probability: the
    kernel's fp32 __expf cannot reorder them. The reference is the fp64
    softmax, a stable sort on (-p, index) -- the kernel's documented tie
    rule, "first lane holding best wins" -- and a renormalisation over the K
    picked. `torch.topk` leaves tie order unspecified and is not the oracle.
    The "spread" rows put every low logit at exactly -200: their fp32
    probabilities are exactly 0, their fp64 ones are equal, so both orders
    fall back to the index. No NaN logits: the kernel's answer for NaN is an
    index of -1, and nothing may index with that.

Block (`MoEMLP.forward`)
    hidden 256, intermediate 384, E = 8, K = 2, weights randn / sqrt(fan_in),
    router rows randn / 8 (logits ~ N(0, 2^2): both picked experts carry
    weight, and the K-th / (K+1)-th logit gap is asserted > 1e-3 in every
    row). The fp64 reference routes the block's own fp32 router logits with
    the gating reference and sums w_k down_e(silu(gate_e x) up_e x).
    Bound, per row: |out - ref| <= tau_blk * max_n |ref[row]|, where tau_blk
    is BLK_FACTOR = 4 times the worst ratio a second reference shows that
    rounds to bf16 where the block does (gu, act, yg, the gate weight, yg * w,
    each index_add_ accumulation). The factor covers the different summation
    orders of the library GEMMs and the HIP kernels; the block mutations, not
    the factor, decide whether it is small enough.
"""
from __future__ import annotations

import functools
import itertools
import zlib
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

NAN = float("nan")
GEMM_REL = 2.0 ** -8
GEMM_ABS = 2.0 ** -12
GEMM_MAX_D = 2048
TILE_M = 16                      # rows per m-tile of the grouped GEMM


def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(_seed(*key))


# --------------------------------------------------------------------------
# grouped GEMM: cases
# --------------------------------------------------------------------------
COUNTS = (
    (3, 0, 17, 5),          # empty expert inside, a 16 + 1 split
    (0, 17, 16),            # first expert empty, a segment of exactly 16
    (16, 0, 0, 32),         # exactly 16 and exactly 32 rows
    (1,),
    (0, 0, 1, 0),           # first and last expert empty
    (33, 1),                # three m-tiles, then a single row
    (16,) * 8,
    (0, 40, 0),
)
# (D, N) the <2> instantiation serves (N < 16384): D > 512 runs the X-staging
# loop more than once, 640 / 1792 end in a 128 / 256-wide tail chunk, 136 and
# 144 are no multiple of the 128-column block
DN_NT2 = ((128, 128), (128, 136), (512, 144), (640, 256), (1024, 128),
          (1792, 384), (2048, 128))
# (D, N) the <4> instantiation serves (N >= 16384); 16400 is no multiple of
# its 256-column block. The wide one only with E <= 2 (42 MB of weights).
DN_NT4 = ((128, 16384), (640, 16400))


def gemm_params() -> List[Tuple[str, Tuple[int, ...], int, int]]:
    """(kind, counts, D, N); kind is "nt2" or "nt4" after the MFMA kernel
    instantiation that N selects."""
    out = [("nt2", c, D, N) for c, (D, N) in itertools.product(COUNTS, DN_NT2)]
    out += [("nt4", c, *DN_NT4[0]) for c in COUNTS]
    out += [("nt4", c, *DN_NT4[1]) for c in COUNTS if len(c) <= 2]
    return out


def gemm_id(p) -> str:
    kind, counts, D, N = p
    return f"{kind}_c{'-'.join(map(str, counts))}_D{D}_N{N}"


@dataclass
class GemmCase:
    counts: Tuple[int, ...]
    D: int
    N: int
    x: torch.Tensor          # [T, D] bf16
    w: torch.Tensor          # [E, N, D] bf16
    ref: torch.Tensor        # [T, N] f64
    A: torch.Tensor          # [T, N] f64

    @property
    def E(self) -> int:
        return len(self.counts)

    @property
    def T(self) -> int:
        return sum(self.counts)

    @property
    def seg_start(self) -> List[int]:
        return [0] + list(itertools.accumulate(self.counts))

    @property
    def expert_of_row(self) -> List[int]:
        return [e for e, n in enumerate(self.counts) for _ in range(n)]


def gemm_reference(x, w, counts) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (ref, A), both [T, N] float64, written out per segment."""
    T, N = x.shape[0], w.shape[1]
    ref = torch.zeros(T, N, dtype=torch.float64)
    A = torch.zeros(T, N, dtype=torch.float64)
    s = 0
    for e, n in enumerate(counts):
        if n:
            xs, we = x[s:s + n].double(), w[e].double()
            ref[s:s + n] = xs @ we.T
            A[s:s + n] = xs.abs() @ we.abs().T
        s += n
    return ref, A


def build_gemm_case(counts: Sequence[int], D: int, N: int) -> GemmCase:
    counts = tuple(int(c) for c in counts)
    assert D <= GEMM_MAX_D and D % 128 == 0
    gen = _gen("moe_gemm", counts, D, N)
    x = torch.randn(sum(counts), D, generator=gen).to(torch.bfloat16)
    w = torch.randn(len(counts), N, D, generator=gen).to(torch.bfloat16)
    ref, A = gemm_reference(x, w, counts)
    return GemmCase(counts, D, N, x, w, ref, A)


# --------------------------------------------------------------------------
# grouped GEMM: comparison
# --------------------------------------------------------------------------
def gemm_ratio(out, ref, A) -> torch.Tensor:
    """Per element |out - ref| / (2^-8 |ref| + 2^-12 A); inf where the output
    is not finite, or differs where the bound is 0."""
    out = out.detach().to("cpu", torch.float64)
    err = (out - ref).abs()
    bound = GEMM_REL * ref.abs() + GEMM_ABS * A
    inf = torch.full_like(err, float("inf"))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, inf, torch.zeros_like(err)))
    return torch.where(torch.isfinite(out), ratio, inf)


def gemm_violates(out, ref, A) -> bool:
    """Would `assert_gemm_close` reject `out`?"""
    r = gemm_ratio(out, ref, A)
    return bool((~(r <= 1.0)).any())


def assert_gemm_close(out, ref, A, what: str = "") -> float:
    """Every element finite and within the bound; returns the worst ratio."""
    if ref.numel() == 0:
        return 0.0
    finite = torch.isfinite(out.detach().float().cpu())
    assert bool(finite.all()), (
        f"{what}: non-finite output in rows "
        f"{(~finite.all(dim=-1)).nonzero().flatten().tolist()[:8]}")
    ratio = gemm_ratio(out, ref, A)
    worst = float(ratio.max())
    assert worst <= 1.0, (
        f"{what}: max err/bound = {worst:.3f} at (row, col) "
        f"{(ratio == ratio.max()).nonzero()[0].tolist()}")
    return worst


# --------------------------------------------------------------------------
# grouped GEMM: mutations of the reference. Each returns the mutated
# reference, or None where it does not apply to the case.
# --------------------------------------------------------------------------
def _row(case: GemmCase, r: int, e: int) -> torch.Tensor:
    return case.w[e].double() @ case.x[r].double()


def _mut_k_tail(case: GemmCase, n: int):
    """The last n elements of k never summed."""
    if case.T == 0:
        return None
    out = case.ref.clone()
    s = 0
    for e, c in enumerate(case.counts):
        if c:
            out[s:s + c] -= (case.x[s:s + c, -n:].double()
                             @ case.w[e, :, -n:].double().T)
        s += c
    return out


def mut_k_drop8(case):
    return _mut_k_tail(case, 8)


def mut_k_drop_chunk(case):
    return _mut_k_tail(case, 128) if case.D > 128 else None


def mut_first_row_prev_expert(case):
    """The first row of every segment computed with expert e - 1."""
    out, hit = case.ref.clone(), False
    for e, c in enumerate(case.counts):
        if c and e > 0:
            out[case.seg_start[e]] = _row(case, case.seg_start[e], e - 1)
            hit = True
    return out if hit else None


def mut_last_row_next_expert(case):
    """The last row of every segment computed with expert e + 1."""
    out, hit = case.ref.clone(), False
    for e, c in enumerate(case.counts):
        if c and e + 1 < case.E:
            r = case.seg_start[e + 1] - 1
            out[r] = _row(case, r, e + 1)
            hit = True
    return out if hit else None


def mut_last_col_zero(case):
    if case.T == 0:
        return None
    out = case.ref.clone()
    out[:, -1] = 0.0
    return out


def mut_swap_cols01(case):
    if case.T == 0:
        return None
    out = case.ref.clone()
    out[:, [0, 1]] = out[:, [1, 0]]
    return out


def mut_row16_unwritten(case):
    """Row r0 + 16 of every segment with more than 16 rows stays NaN."""
    out, hit = case.ref.clone(), False
    for e, c in enumerate(case.counts):
        if c > TILE_M:
            out[case.seg_start[e] + TILE_M] = NAN
            hit = True
    return out if hit else None


def mut_seg_start_shift(case):
    """Every segment offset one too large: row 0 is never written and the
    first row after every expert change uses the previous rows' expert."""
    if case.T == 0:
        return None
    out = case.ref.clone()
    owner = case.expert_of_row
    out[0] = NAN
    for r in range(1, case.T):
        if owner[r - 1] != owner[r]:
            out[r] = _row(case, r, owner[r - 1])
    return out


GEMM_MUTATIONS: Dict[str, Callable[[GemmCase], Optional[torch.Tensor]]] = {
    "k_drop8": mut_k_drop8,
    "k_drop_chunk": mut_k_drop_chunk,
    "first_row_prev_expert": mut_first_row_prev_expert,
    "last_row_next_expert": mut_last_row_next_expert,
    "last_col_zero": mut_last_col_zero,
    "swap_cols01": mut_swap_cols01,
    "row16_unwritten": mut_row16_unwritten,
    "seg_start_shift": mut_seg_start_shift,
}


# --------------------------------------------------------------------------
# gating
# --------------------------------------------------------------------------
GATING_E = (1, 4, 8, 60, 64)
GATING_K = (1, 2, 8)
GATING_T = (1, 4, 5, 33)         # a block holds 4 waves: 5 and 33 leave a tail
ROW_KINDS = ("grid", "equal", "dupmax", "ktie", "spread", "offset", "neginf")


def gating_params() -> List[Tuple[int, int, int]]:
    return [(E, K, T) for E in GATING_E for K in GATING_K if K <= E
            for T in GATING_T]


def _grid(gen, n: int) -> torch.Tensor:
    return torch.randint(-32, 33, (n,), generator=gen).float() / 8


def _gating_row(kind: str, E: int, K: int, gen) -> Tuple[torch.Tensor, str]:
    """One row of logits of the kind asked for, or a plain grid row where
    the kind does not fit (E, K)."""
    row = _grid(gen, E)
    if kind == "equal":
        row = row[:1].repeat(E)
    elif kind == "dupmax" and E >= 2:
        i = torch.randperm(E, generator=gen)[:2]
        row[i] = float(row.max()) + 1.0
    elif kind == "ktie" and E > K:
        # distinct values by rank, then rank K takes rank K-1's value: the
        # tie sits across the K / K+1 boundary and the lower index wins
        perm = torch.randperm(E, generator=gen)
        row[perm] = 4.0 - torch.arange(E).float() / 8
        row[perm[K]] = row[perm[K - 1]]
    elif kind == "spread" and E >= 2:
        perm = torch.randperm(E, generator=gen)
        nhigh = max(1, E // 4)
        row[perm[:nhigh]] = 200.0 + row[perm[:nhigh]]
        row[perm[nhigh:]] = -200.0
    elif kind == "offset":
        row = row + 1.0e4
    elif kind == "neginf" and E > K:
        ninf = min(E - K, max(1, E // 3))
        row[torch.randperm(E, generator=gen)[:ninf]] = float("-inf")
    elif kind != "grid":
        kind = "grid"
    return row, kind


def gating_logits(E: int, K: int, T: int) -> Tuple[torch.Tensor, List[str]]:
    """-> (logits [T, E] fp32, the kind of every row). The kinds rotate from
    a per-case start, so the short T also reach every kind across (E, K)."""
    gen = _gen("moe_gating", E, K, T)
    start = _seed("moe_gating_start", E, K, T) % len(ROW_KINDS)
    rows, kinds = [], []
    for t in range(T):
        row, kind = _gating_row(ROW_KINDS[(start + t) % len(ROW_KINDS)], E, K,
                                gen)
        rows.append(row)
        kinds.append(kind)
    logits = torch.stack(rows).float()
    assert not bool(logits.isnan().any())
    assert bool((torch.isfinite(logits).sum(-1) >= K).all())
    return logits, kinds


def gating_reference(logits: torch.Tensor, K: int):
    """-> (topi [T, K] int64, topw [T, K] f64, p [T, E] f64): fp64 softmax,
    stable sort on (-p, index), weights renormalised over the K picked."""
    p = torch.softmax(logits.detach().cpu().double(), dim=-1)
    order = torch.sort(-p, dim=-1, stable=True).indices
    topi = order[:, :K]
    picked = p.gather(1, topi)
    return topi, picked / picked.sum(-1, keepdim=True), p


def assert_gating_matches(topw, topi, logits, K: int, what: str = ""):
    """All the gating assertions: indices equal the reference, distinct and
    in [0, E) per row; weights descending, summing to 1 within 1e-5 and equal
    to the reference at rtol 1e-4 / atol 1e-5."""
    T, E = logits.shape
    ri, rw, _ = gating_reference(logits, K)
    gi = topi.detach().cpu().long()
    gw = topw.detach().cpu().double()
    assert gi.shape == (T, K) and gw.shape == (T, K), what
    assert bool(((gi >= 0) & (gi < E)).all()), f"{what}: index out of [0, E)"
    srt = gi.sort(dim=-1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), f"{what}: repeated expert"
    bad = (gi != ri).any(dim=-1).nonzero().flatten().tolist()
    assert not bad, (f"{what}: rows {bad[:8]} pick {gi[bad[0]].tolist()}, "
                     f"reference {ri[bad[0]].tolist()}")
    assert bool((gw[:, :-1] >= gw[:, 1:]).all()), f"{what}: not descending"
    assert float((gw.sum(-1) - 1.0).abs().max()) <= 1e-5, f"{what}: sum != 1"
    torch.testing.assert_close(gw, rw, rtol=1e-4, atol=1e-5)


# --------------------------------------------------------------------------
# block: MoEMLP.forward
# --------------------------------------------------------------------------
BLK_D, BLK_I, BLK_E, BLK_K = 256, 384, 8, 2
BLK_TS = (1, 5, 16, 64, 65, 256, 257)    # every T a block test runs
BLK_FACTOR = 4.0
BLK_MIN_GAP = 1e-3


def block_config(moe_ep: bool = False):
    from dynamo_amd.engine.config import ModelConfig
    return ModelConfig(name="moe-block-test", arch="mixtral",
                       hidden_size=BLK_D, intermediate_size=BLK_I,
                       num_experts=BLK_E, num_experts_per_tok=BLK_K,
                       moe_ep=moe_ep)


@functools.lru_cache(maxsize=None)
def block_weights():
    """One full set: (router [E, D], w_gate_up [E, 2I, D], w_down [E, D, I]),
    bf16. Outputs are O(1) and both picked experts carry weight."""
    gen = _gen("moe_block_weights")
    bf = torch.bfloat16
    router = (torch.randn(BLK_E, BLK_D, generator=gen) / 8).to(bf)
    wgu = (torch.randn(BLK_E, 2 * BLK_I, BLK_D, generator=gen)
           / BLK_D ** 0.5).to(bf)
    wd = (torch.randn(BLK_E, BLK_D, BLK_I, generator=gen)
          / BLK_I ** 0.5).to(bf)
    return router, wgu, wd


def _logit_gap(logits: torch.Tensor) -> float:
    """Smallest K-th / (K+1)-th logit distance over the rows."""
    srt = logits.detach().cpu().float().sort(dim=-1, descending=True).values
    return float((srt[:, BLK_K - 1] - srt[:, BLK_K]).min())


@functools.lru_cache(maxsize=None)
def block_x(T: int, variant: int = 0) -> torch.Tensor:
    """[T, D] bf16 randn; `variant` picks another draw (other routings).
    The router logits are bf16 values, so two of them tie now and then: the
    seed is the first of (T, variant, 0), (T, variant, 1), ... whose K-th and
    (K+1)-th logits are more than BLK_MIN_GAP apart in every row."""
    for attempt in range(64):
        x = torch.randn(T, BLK_D, generator=_gen("moe_block_x", T, variant,
                                                 attempt)).to(torch.bfloat16)
        if _logit_gap(cpu_block_logits(x)) > BLK_MIN_GAP:
            return x
    raise AssertionError(f"no decisive seed for T={T}")


def load_block_weights(moe, lo: int = 0, hi: int = BLK_E) -> None:
    """Overwrite a MoEMLP's weights with experts [lo, hi) of the full set
    (the router is never sliced)."""
    router, wgu, wd = block_weights()
    with torch.no_grad():
        moe.router.copy_(router)
        moe.w_gate_up.copy_(wgu[lo:hi])
        moe.w_down.copy_(wd[lo:hi])


def _bf(t: torch.Tensor) -> torch.Tensor:
    """fp64 -> fp32 accumulator -> bf16 store, back in fp64."""
    return t.float().to(torch.bfloat16).double()


def _route(logits: torch.Tensor):
    """Gating reference on the block's logits, with the decisiveness
    condition of the case: K-th and (K+1)-th logit more than 1e-3 apart."""
    logits = logits.detach().cpu().float()
    gap = _logit_gap(logits)
    assert gap > BLK_MIN_GAP, f"K / K+1 logit gap {gap:.2e}: pick another seed"
    return gating_reference(logits, BLK_K)


def _expert_outputs(x, emulate: bool):
    """down_e(silu(gate_e x) * up_e x) of every token under every expert,
    [E, T, D] fp64; with `emulate`, gu, act and yg are rounded to bf16."""
    _, wgu, wd = block_weights()
    rnd = _bf if emulate else (lambda t: t)
    gu = rnd(torch.einsum("td,end->etn", x.double(), wgu.double()))
    g, u = gu[..., :BLK_I], gu[..., BLK_I:]
    act = rnd(g * torch.sigmoid(g) * u)
    return rnd(torch.einsum("eti,edi->etd", act, wd.double())), gu


def block_reference(x: torch.Tensor, logits: torch.Tensor,
                    mutation: Optional[str] = None) -> Optional[torch.Tensor]:
    """-> ref [T, D] fp64 (None for a mutation that does not apply). `logits` are the fp32 router logits of the block's
    own `linear(x, router).float()`. `mutation` names a BLOCK_MUTATIONS
    fault to build into the result."""
    T = x.shape[0]
    topi, topw, p = _route(logits)
    Y, gu = _expert_outputs(x, emulate=False)
    if mutation == "gate_up_swapped":
        _, _, wd = block_weights()
        g, u = gu[..., BLK_I:], gu[..., :BLK_I]
        Y = torch.einsum("eti,edi->etd", g * torch.sigmoid(g) * u, wd.double())
    topi, topw = topi.clone(), topw.clone()
    if mutation == "experts_swapped":
        # the token whose two weights differ most (equal weights would make
        # the swap the same sum)
        t = int((topw[:, 0] - topw[:, 1]).argmax())
        topi[t] = topi[t].flip(0)
    elif mutation == "unrenormalised":
        topw = p.gather(1, topi)
    elif mutation == "second_expert_dropped":
        t = int(topw[:, 1].argmax())
        topw[t, 1] = 0.0
    tok = torch.arange(T).repeat_interleave(BLK_K)
    flat_e, flat_w = topi.reshape(-1), topw.reshape(-1)
    if mutation == "weights_unsorted":
        # rows sorted by expert, weights left in token order
        order = torch.argsort(flat_e, stable=True)
        if bool((order == torch.arange(order.numel())).all()):
            return None                  # already sorted: nothing to misplace
        flat_e, tok = flat_e[order], tok[order]
    out = torch.zeros(T, BLK_D, dtype=torch.float64)
    out.index_add_(0, tok, Y[flat_e, tok] * flat_w.unsqueeze(-1))
    return out


BLOCK_MUTATIONS = ("experts_swapped", "unrenormalised", "weights_unsorted",
                   "second_expert_dropped", "gate_up_swapped")


def block_emulated(x: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """The block in exact arithmetic except that it rounds to bf16 where
    MoEMLP.forward does: gu, act, yg, the gate weight, yg * w, and each
    index_add_ accumulation (rows arrive sorted by expert)."""
    T = x.shape[0]
    topi, topw, _ = _route(logits)
    Y, _ = _expert_outputs(x, emulate=True)
    w = _bf(topw)
    out = torch.zeros(T, BLK_D, dtype=torch.float64)
    t = torch.arange(T)
    srt = topi.sort(dim=-1)
    for k in range(BLK_K):
        e = srt.values[:, k]
        wk = w.gather(1, srt.indices[:, k:k + 1])
        out = _bf(out + _bf(Y[e, t] * wk))
    return out


def block_ratio(out, ref) -> torch.Tensor:
    """Per row max_n |out - ref| / max_n |ref|; inf for a non-finite row."""
    out = out.detach().to("cpu", torch.float64)
    s_row = ref.abs().amax(dim=-1)
    ratio = (out - ref).abs().amax(dim=-1) / s_row.clamp_min(1e-300)
    bad = ~torch.isfinite(out).all(dim=-1)
    return torch.where(bad, torch.full_like(ratio, float("inf")), ratio)


def cpu_block_logits(x: torch.Tensor) -> torch.Tensor:
    """The router logits of a bf16 block on the CPU."""
    router, _, _ = block_weights()
    return torch.nn.functional.linear(x, router).float()


@functools.lru_cache(maxsize=None)
def emulated_worst_ratio() -> float:
    """Worst ratio of the bf16-emulating reference against the fp64 one over
    all block cases."""
    worst = 0.0
    for T in BLK_TS:
        x = block_x(T)
        logits = cpu_block_logits(x)
        r = block_ratio(block_emulated(x, logits), block_reference(x, logits))
        worst = max(worst, float(r.max()))
    return worst


def tau_blk() -> float:
    return BLK_FACTOR * emulated_worst_ratio()


def assert_block_close(out, ref, what: str = "", scale: float = 1.0) -> float:
    """Every row finite and within scale * tau_blk * S_row; returns the worst
    err / (tau_blk * S_row)."""
    ratio = block_ratio(out, ref) / tau_blk()
    worst = float(ratio.max())
    assert worst <= scale, (
        f"{what}: max err/(tau_blk*S_row) = {worst:.3f} at row "
        f"{int(ratio.argmax())} (tau_blk = {tau_blk():.5f})")
    return worst
