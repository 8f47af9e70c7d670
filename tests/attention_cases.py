"""Paged-attention test cases with teeth (plain helper, not a conftest).

The older attention tests feed `randn` q/k/v to the kernels and compare with
a fixed `atol`.  A softmax over random scores averages V down to an rms of a
few hundredths, so that `atol` is about the size of the signal: a dropped
token, a leaked token or two swapped pages all pass.  This module builds
cases where such bugs are O(1) errors, and a comparison whose bound scales
with the row.

Case builder
    * page ids come from `randperm`; page 0 is a reserved null page
    * the page table is 2 columns wider than the longest row needs and its
      unused entries are 0 (the null page)
    * the null page, the spare pages nobody owns and every slot >= ctx of a
      row's last page hold NaN in K and V (NaN survives float8_e4m3fn), so
      any read past `ctx` or through an unused table entry poisons the row
    * fp8 caches are quantised first; the reference reads the dequantised
      values, so quantisation error is not part of the comparison

Structured queries (decode): the query heads of a batch row cycle through
three kinds (with G == 1 the kinds rotate over batch rows instead):
    tail needle   q = k[ctx-1] of the head's kv head
    edge needle   q = k[n]; n rotates over token 0, the tokens either side
                  of every page / 32-token tile / slab (chunk/4) / chunk edge
                  inside ctx (categories round-robin, each shuffled per case)
    diffuse       plain randn
A needle puts a softmax weight >= 0.5 on its token at these lengths
(|k|^2/sqrt(128) ~ 11.3 against N(0,1) scores), so losing, duplicating or
misplacing that one token moves the output by O(|v|).

Structured queries (prefill): query row j at absolute position p alternates
    diagonal needle  q = k[p]    fails if the mask excludes the diagonal
    future lure      q = k[p+1]  (when p+1 < ctx) an O(1) error if the mask
                                 leaks one token, a diffuse row if it holds

Comparison: out must be finite and |out - ref| <= TAU * A[row] with
A = max_d sum_t p_t |v_t,d| and TAU = 2^-7: P is rounded to bf16 before the
PV MFMA (<= 2^-9 relative per term), l is accumulated from the unrounded P
(another 2^-9), the bf16 output adds 2^-9 and one more 2^-9 is slack for
__expf / v_exp.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

HD = 128
SCALE = HD ** -0.5
TAU = 2.0 ** -7
TILE = 32
SPARE_PAGES = 3
NAN = float("nan")


# --------------------------------------------------------------------------
# case containers
# --------------------------------------------------------------------------
@dataclass
class DecodeCase:
    q: torch.Tensor            # [B, Hq, hd] bf16
    kcache: torch.Tensor       # [P, Hkv, ps, hd] bf16 | e4m3
    vcache: torch.Tensor       # same, or [P, Hkv, hd, ps] when v_transposed
    page_table: torch.Tensor   # [B, max_pages + 2] int32, unused entries 0
    ctx_lens: torch.Tensor     # [B] int32
    G: int
    Hkv: int
    ps: int
    chunk: int
    v_transposed: bool
    fp8: bool
    # dequantised caches (fp32 is exact for bf16 and e4m3), token-major
    k_f32: torch.Tensor = field(repr=False, default=None)
    v_f32: torch.Tensor = field(repr=False, default=None)
    needles: List[Tuple[int, int, int, str]] = field(default_factory=list)
    # (b, q head, token, "tail" | "edge")

    @property
    def scale(self) -> float:
        return SCALE

    @property
    def ctxs(self) -> List[int]:
        return [int(c) for c in self.ctx_lens]

    def npages(self, b: int) -> int:
        return (self.ctxs[b] + self.ps - 1) // self.ps

    def device_args(self, device):
        """(q, kcache, vcache, page_table, ctx_lens) on `device`."""
        return tuple(t.to(device) for t in (self.q, self.kcache, self.vcache,
                                            self.page_table, self.ctx_lens))


@dataclass
class PrefillCase:
    q: torch.Tensor            # [Tq, Hq, hd] bf16
    kcache: torch.Tensor
    vcache: torch.Tensor
    page_table: torch.Tensor   # [nseq, max_pages + 2] int32
    seq_q_start: torch.Tensor  # [nseq] int32
    seq_q_len: torch.Tensor
    seq_ctx_len: torch.Tensor
    spec: Tuple[Tuple[int, int], ...]
    G: int
    Hkv: int
    ps: int
    v_transposed: bool
    fp8: bool
    k_f32: torch.Tensor = field(repr=False, default=None)
    v_f32: torch.Tensor = field(repr=False, default=None)
    n_lures: int = 0

    @property
    def scale(self) -> float:
        return SCALE

    def device_args(self, device):
        return tuple(t.to(device) for t in (
            self.q, self.kcache, self.vcache, self.page_table,
            self.seq_q_start, self.seq_q_len, self.seq_ctx_len))


# --------------------------------------------------------------------------
# cache construction
# --------------------------------------------------------------------------
def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _build_cache(gen, ctxs: Sequence[int], Hkv: int, ps: int, fp8: bool,
                 v_transposed: bool):
    """-> (kcache, vcache, page_table, k_f32, v_f32); *_f32 are token-major
    [P, Hkv, ps, hd] dequantised copies, NaN where the cache holds NaN."""
    npages = [(c + ps - 1) // ps for c in ctxs]
    P = 1 + sum(npages) + SPARE_PAGES
    store = torch.float8_e4m3fn if fp8 else torch.bfloat16
    k = torch.randn(P, Hkv, ps, HD, generator=gen).to(store).float()
    v = torch.randn(P, Hkv, ps, HD, generator=gen).to(store).float()
    ids = (torch.randperm(P - 1, generator=gen) + 1).tolist()
    table = torch.zeros(len(ctxs), max(npages + [0]) + 2, dtype=torch.int32)
    owned = 0
    for b, (c, n) in enumerate(zip(ctxs, npages)):
        row = ids[owned:owned + n]
        owned += n
        table[b, :n] = torch.tensor(row, dtype=torch.int32)
        if c % ps:
            k[row[-1], :, c % ps:] = NAN
            v[row[-1], :, c % ps:] = NAN
    for page in [0] + ids[owned:]:          # null page + spare pages
        k[page] = NAN
        v[page] = NAN
    kcache = k.to(store)
    vcache = (v.transpose(2, 3).contiguous() if v_transposed else v).to(store)
    # the quantised round trip must be the identity (values were quantised
    # first) and NaN must survive the storage type
    assert torch.equal(kcache.float().nan_to_num(7.0), k.nan_to_num(7.0))
    assert bool(kcache[0].float().isnan().all())
    assert bool(vcache[0].float().isnan().all())
    return kcache, vcache, table, k, v


def _token(cache_f32, table_row, t: int, ps: int):
    """[Hkv, hd] of logical token t of one sequence."""
    return cache_f32[int(table_row[t // ps]), :, t % ps]


def needle_candidates(ctx: int, ps: int, chunk: int, gen) -> List[int]:
    """Edge positions of one row, categories round-robin (page, tile, slab,
    chunk), each category shuffled; token 0 always comes first."""
    def edges(step):
        out = []
        for e in range(step, ctx, step):
            out += [e - 1, e]
        return out
    cats = [edges(ps) + [((ctx - 1) // ps) * ps], edges(TILE),
            edges(chunk // 4), edges(chunk)]
    cats = [[c[i] for i in torch.randperm(len(c), generator=gen).tolist()]
            for c in cats if c]
    order = [0]
    while any(cats):
        for c in cats:
            if c:
                order.append(c.pop())
    seen, uniq = set(), []
    for t in order:
        if 0 <= t < ctx and t not in seen:
            seen.add(t)
            uniq.append(t)
    return uniq


def build_decode_case(G: int, Hkv: int, ps: int, ctxs: Sequence[int], *,
                      chunk: int = 512, v_transposed: bool = False,
                      fp8: bool = False) -> DecodeCase:
    ctxs = [int(c) for c in ctxs]
    gen = torch.Generator().manual_seed(
        _seed("decode", G, Hkv, ps, ctxs, chunk, v_transposed, fp8))
    kcache, vcache, table, k32, v32 = _build_cache(gen, ctxs, Hkv, ps, fp8,
                                                   v_transposed)
    B, Hq = len(ctxs), G * Hkv
    q = torch.randn(B, Hq, HD, generator=gen)
    needles = []
    turn = 0                                  # edge-needle rotation, per case
    for b, ctx in enumerate(ctxs):
        if ctx == 0:
            continue
        cand = needle_candidates(ctx, ps, chunk, gen)
        for h in range(Hq):
            kind = (b if G == 1 else h % G) % 3
            if kind == 2:
                continue
            if kind == 0:
                t, name = ctx - 1, "tail"
            else:
                t, name = cand[turn % len(cand)], "edge"
                turn += 1
            q[b, h] = _token(k32, table[b], t, ps)[h // G]
            needles.append((b, h, t, name))
    return DecodeCase(q=q.to(torch.bfloat16), kcache=kcache, vcache=vcache,
                      page_table=table,
                      ctx_lens=torch.tensor(ctxs, dtype=torch.int32),
                      G=G, Hkv=Hkv, ps=ps, chunk=chunk,
                      v_transposed=v_transposed, fp8=fp8, k_f32=k32,
                      v_f32=v32, needles=needles)


def build_prefill_case(G: int, Hkv: int, ps: int,
                       spec: Sequence[Tuple[int, int]], *,
                       v_transposed: bool = False,
                       fp8: bool = False) -> PrefillCase:
    spec = tuple((int(a), int(b)) for a, b in spec)
    gen = torch.Generator().manual_seed(
        _seed("prefill", G, Hkv, ps, spec, v_transposed, fp8))
    ctxs = [c for _, c in spec]
    qlens = [ql for ql, _ in spec]
    kcache, vcache, table, k32, v32 = _build_cache(gen, ctxs, Hkv, ps, fp8,
                                                   v_transposed)
    Hq = G * Hkv
    starts = [0]
    for ql in qlens[:-1]:
        starts.append(starts[-1] + ql)
    q = torch.randn(sum(qlens), Hq, HD, generator=gen)
    lures = 0
    for s, (ql, ctx) in enumerate(spec):
        for j in range(ql):
            p = ctx - ql + j
            for h in range(Hq):
                if (j + h) % 2 == 0:
                    t = p                       # diagonal needle
                elif p + 1 < ctx:
                    t = p + 1                   # future lure
                    lures += 1
                else:
                    continue                    # no future token: diffuse
                q[starts[s] + j, h] = _token(k32, table[s], t, ps)[h // G]
    i32 = dict(dtype=torch.int32)
    return PrefillCase(q=q.to(torch.bfloat16), kcache=kcache, vcache=vcache,
                       page_table=table,
                       seq_q_start=torch.tensor(starts, **i32),
                       seq_q_len=torch.tensor(qlens, **i32),
                       seq_ctx_len=torch.tensor(ctxs, **i32), spec=spec, G=G,
                       Hkv=Hkv, ps=ps, v_transposed=v_transposed, fp8=fp8,
                       k_f32=k32, v_f32=v32, n_lures=lures)


# --------------------------------------------------------------------------
# fp64 references (written out here; independent of ops.torch_ref)
# --------------------------------------------------------------------------
def _gather(cache_f32, table_row, n: int, ps: int) -> torch.Tensor:
    """Logical tokens 0..n-1 of one sequence -> [n, Hkv, hd] float64."""
    t = torch.arange(n)
    pages = table_row[t // ps].long()
    return cache_f32[pages, :, t % ps].to(torch.float64)


def _attend(qrow, K, V, G: int, allowed=None):
    """qrow [..., Hq, hd] f64, K/V [n, Hkv, hd] f64 -> (out, A)."""
    K = K.repeat_interleave(G, dim=1)
    V = V.repeat_interleave(G, dim=1)
    s = torch.einsum("...hd,thd->...ht", qrow, K) * SCALE
    if allowed is not None:                     # [rows, n] bool
        s = s.masked_fill(~allowed[:, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.where(s == float("-inf"), torch.zeros_like(p), p)
    out = torch.einsum("...ht,thd->...hd", p, V)
    A = torch.einsum("...ht,thd->...hd", p, V.abs()).amax(dim=-1)
    return out, A, p


def decode_reference(case: DecodeCase, *, ctx_lens=None, k_table=None,
                     v_table=None, v_reversed: Optional[Dict[int, int]] = None,
                     return_weights: bool = False):
    """-> (ref [B, Hq, hd] f64, A [B, Hq] f64).

    The keyword arguments exist for the teeth checks, which mutate this
    reference: other context lengths, another page table for K and/or V,
    and `v_reversed[b] = j` token-reverses logical V page j of row b."""
    ctxs = case.ctxs if ctx_lens is None else [int(c) for c in ctx_lens]
    kt = case.page_table if k_table is None else k_table
    vt = case.page_table if v_table is None else v_table
    B, Hq = case.q.shape[:2]
    ref = torch.zeros(B, Hq, HD, dtype=torch.float64)
    A = torch.zeros(B, Hq, dtype=torch.float64)
    weights = {}
    for b, n in enumerate(ctxs):
        if n == 0:
            continue
        K = _gather(case.k_f32, kt[b], n, case.ps)
        full = ((n + case.ps - 1) // case.ps) * case.ps
        V = _gather(case.v_f32, vt[b], full, case.ps)
        if v_reversed is not None and b in v_reversed:
            lo = v_reversed[b] * case.ps
            V[lo:lo + case.ps] = V[lo:lo + case.ps].flip(0)
        ref[b], A[b], p = _attend(case.q[b].double(), K, V[:n], case.G)
        weights[b] = p
    if return_weights:
        return ref, A, weights
    return ref, A


def prefill_reference(case: PrefillCase, *, mask_shift: int = 0):
    """-> (ref [Tq, Hq, hd] f64, A [Tq, Hq] f64). Query row at absolute
    position p attends kv positions t <= p + mask_shift (t < ctx)."""
    Tq, Hq = case.q.shape[:2]
    ref = torch.zeros(Tq, Hq, HD, dtype=torch.float64)
    A = torch.zeros(Tq, Hq, dtype=torch.float64)
    for s, (ql, ctx) in enumerate(case.spec):
        if ql == 0:
            continue
        qs = int(case.seq_q_start[s])
        K = _gather(case.k_f32, case.page_table[s], ctx, case.ps)
        V = _gather(case.v_f32, case.page_table[s], ctx, case.ps)
        qpos = torch.arange(ctx - ql, ctx)
        allowed = torch.arange(ctx)[None, :] <= (qpos[:, None] + mask_shift)
        o, a, _ = _attend(case.q[qs:qs + ql].double(), K, V, case.G, allowed)
        dead = ~allowed.any(dim=1)              # rows that attend nothing
        o[dead] = 0.0
        a[dead] = 0.0
        ref[qs:qs + ql], A[qs:qs + ql] = o, a
    return ref, A


# --------------------------------------------------------------------------
# comparison
# --------------------------------------------------------------------------
def error_ratio(out, ref, A, tau: float = TAU) -> torch.Tensor:
    """Per (row, head): max_d |out - ref| / (tau * A); inf where the bound
    is violated with A == 0 or the output is not finite."""
    out = out.detach().to("cpu", torch.float64)
    err = (out - ref).abs().amax(dim=-1)
    bound = tau * A
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    bad = ~torch.isfinite(out).all(dim=-1)
    return torch.where(bad, torch.full_like(ratio, float("inf")), ratio)


def violates(out, ref, A, tau: float = TAU) -> torch.Tensor:
    """Per (row, head) bool: would `assert_attention_close` reject it?"""
    return ~(error_ratio(out, ref, A, tau) <= 1.0)


def assert_attention_close(out, ref, A, tau: float = TAU, what: str = ""):
    """Finite first, then |out - ref| <= tau * A per row. Returns the worst
    err / (tau * A) so callers can record it."""
    finite = torch.isfinite(out.detach().float().cpu())
    assert bool(finite.all()), (
        f"{what}: non-finite output in rows "
        f"{(~finite.all(dim=-1)).nonzero().tolist()[:8]}")
    ratio = error_ratio(out, ref, A, tau)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert worst <= 1.0, (
        f"{what}: max err/(tau*A) = {worst:.3f} at row/head "
        f"{(ratio == ratio.max()).nonzero()[0].tolist()}")
    return worst


# --------------------------------------------------------------------------
# case lists shared by the CPU reference module and the GPU edge module
# --------------------------------------------------------------------------
CTX_LISTS = (
    (1, 31, 32, 33),
    (63, 64, 65, 0),
    (127, 128, 129),
    (0, 511, 512, 513),
    (1100, 1, 640),
)
# Hkv spread over the G values (not the full product)
HKV_OF_G = {1: 3, 2: 2, 3: 1, 4: 3, 5: 2, 6: 1, 7: 2, 8: 1, 16: 1}


def decode_token_major_params():
    """(G, Hkv, ps, ctx-list index) of the token-major bf16 sweep."""
    out = []
    for G, Hkv in HKV_OF_G.items():
        sizes = (32, 64, 128, 256) + ((16,) if G in (1, 2, 4, 8) else ())
        for ps in sizes:
            for ci in range(len(CTX_LISTS)):
                out.append((G, Hkv, ps, ci))
    return out


# (max_ctx of the scratch, chunk it implies, context lengths)
OVERSIZED = (
    (2048, 1024, (1023, 1024, 1025, 300)),
    (8192, 2048, (2047, 2049, 5)),
)

# d-major V: Hkv and context list spread over (G, ps)
def decode_d_major_params():
    out = []
    for gi, G in enumerate((2, 3, 8, 16)):
        for pi, ps in enumerate((32, 64, 128)):
            Hkv = (1, 2, 3)[(gi + pi) % 3] if G < 16 else 1
            for fp8 in (False, True):
                out.append((G, Hkv, ps, (gi + pi) % len(CTX_LISTS),
                            (gi + pi + 3) % len(CTX_LISTS), fp8))
    return out


def decode_fp8_token_major_params():
    out = []
    for gi, G in enumerate((1, 4, 7, 16)):
        for pi, ps in enumerate((32, 64)):
            Hkv = {1: 2, 4: 1, 7: 3, 16: 1}[G]
            out.append((G, Hkv, ps, (2 * gi + pi) % len(CTX_LISTS),
                        (2 * gi + pi + 2) % len(CTX_LISTS)))
    return out


# prefill: (q_len, ctx_len) lists. Tile heights are (8/G)*32 = 32/64/128
# rows for G = 8/4/2 and 64 for the 16x16 fallback (G = 1, 7).
PREFILL_SPECS = (
    ((31, 31), (1, 1), (33, 33)),
    ((65, 130), (5, 200)),
    ((129, 129), (3, 67)),
    ((1, 1), (63, 64), (64, 257)),
)
PREFILL_G_HKV = ((1, 2), (2, 1), (4, 2), (8, 1), (7, 1))
PREFILL_PS = (16, 32, 64, 128)


def prefill_params():
    """(G, Hkv, ps, spec index, v_transposed): both layouts for every
    (G, ps); the spec list rotates so each (G, layout) sees all of them."""
    out = []
    for gi, (G, Hkv) in enumerate(PREFILL_G_HKV):
        for pi, ps in enumerate(PREFILL_PS):
            for vt in (False, True):
                for k in range(2):
                    si = (gi + pi + 2 * k + vt) % len(PREFILL_SPECS)
                    out.append((G, Hkv, ps, si, vt))
    return out


def prefill_fp8_params():
    out = []
    for gi, (G, Hkv) in enumerate(((2, 2), (4, 1), (8, 2))):
        for pi, ps in enumerate(PREFILL_PS):
            for vt in (False, True):
                out.append((G, Hkv, ps,
                            (gi + pi + vt) % len(PREFILL_SPECS), vt))
    return out
