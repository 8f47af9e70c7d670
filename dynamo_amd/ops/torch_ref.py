"""Plain-PyTorch fp32 reference implementations of every native op.

These serve two roles:
  1. the CPU execution path (config #1: OPT-125m aggregated on CPU), and
  2. the numerics oracle the HIP kernels are tested against
     (tests/test_gpu_kernels.py compares each kernel to these in fp32).
"""
from __future__ import annotations

import torch


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    return ((xf * torch.rsqrt(var + eps)) * weight.float()).to(x.dtype)


def fused_add_rmsnorm(x, residual, weight, eps):
    """residual <- x + residual ; returns rmsnorm(residual) (matches the HIP
    kernel's bf16 residual-stream rounding: the sum is stored in the stream
    dtype before normalizing)."""
    summed = (x.float() + residual.float()).to(residual.dtype)
    residual.copy_(summed)
    return rmsnorm(summed, weight, eps)


def make_cos_sin_cache(max_pos: int, head_dim: int, theta: float,
                       device="cpu", scaling=None) -> torch.Tensor:
    """[max_pos, head_dim] fp32: first half cos, second half sin."""
    half = head_dim // 2
    inv_freq = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64) / half))
    if scaling is not None:
        inv_freq = apply_llama3_scaling(inv_freq, **scaling)
    t = torch.arange(max_pos, dtype=torch.float64)
    freqs = torch.outer(t, inv_freq)
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).float().to(device)


def apply_llama3_scaling(inv_freq, factor=8.0, low_freq_factor=1.0,
                         high_freq_factor=4.0, original_max_position=8192):
    import math
    low_wavelen = original_max_position / low_freq_factor
    high_wavelen = original_max_position / high_freq_factor
    new = []
    for f in inv_freq:
        wavelen = 2 * math.pi / f
        if wavelen < high_wavelen:
            new.append(f)
        elif wavelen > low_wavelen:
            new.append(f / factor)
        else:
            smooth = (original_max_position / wavelen - low_freq_factor) / (
                high_freq_factor - low_freq_factor)
            new.append((1 - smooth) * f / factor + smooth * f)
    return torch.tensor(new, dtype=inv_freq.dtype)


def rope(q, k, positions, cos_sin, num_q_heads, num_k_heads, head_dim):
    """NeoX-style rotary, in-place semantics (returns new tensors)."""
    half = head_dim // 2
    cs = cos_sin[positions.long()]          # [T, hd]
    cos = cs[:, :half].unsqueeze(1).float()  # [T, 1, half]
    sin = cs[:, half:].unsqueeze(1).float()

    def rot(x, H):
        x = x.view(-1, H, head_dim).float()
        x1, x2 = x[..., :half], x[..., half:]
        o1 = x1 * cos - x2 * sin
        o2 = x2 * cos + x1 * sin
        return torch.cat([o1, o2], dim=-1)

    qo = rot(q, num_q_heads).to(q.dtype).view(q.shape)
    ko = rot(k, num_k_heads).to(k.dtype).view(k.shape)
    return qo, ko


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    d = gate_up.shape[-1] // 2
    g, u = gate_up[..., :d].float(), gate_up[..., d:].float()
    return (torch.nn.functional.silu(g) * u).to(gate_up.dtype)


def gelu(x: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.gelu(x.float(), approximate="tanh").to(x.dtype)


def kv_cache_append(kcache, vcache, k, v, slot_mapping,
                    v_transposed=False):
    """kcache: [P, Hkv, ps, hd]; k/v: [T, Hkv, hd]; slots: [T] int64.
    v_transposed: vcache is d-major [P, Hkv, hd, ps] (the MI355X decode
    layout — PV fragments read as contiguous token runs)."""
    P, Hkv, ps, hd = kcache.shape
    valid = slot_mapping >= 0
    slots = slot_mapping[valid]
    pages = (slots // ps).long()
    offs = (slots % ps).long()
    kcache[pages, :, offs] = k[valid].to(kcache.dtype)
    if v_transposed:
        vcache[pages, :, :, offs] = v[valid].to(vcache.dtype)
    else:
        vcache[pages, :, offs] = v[valid].to(vcache.dtype)


def _gather_kv(kcache, page_table, ctx_len, v_transposed=False):
    """-> [ctx_len, Hkv, hd] for one sequence."""
    if v_transposed:
        P, Hkv, hd, ps = kcache.shape
    else:
        P, Hkv, ps, hd = kcache.shape
    npages = (ctx_len + ps - 1) // ps
    pages = page_table[:npages].long()
    kv = kcache[pages]
    if v_transposed:                        # [np, Hkv, hd, ps]
        kv = kv.permute(0, 3, 1, 2).reshape(npages * ps, Hkv, hd)
    else:                                   # [np, Hkv, ps, hd]
        kv = kv.permute(0, 2, 1, 3).reshape(npages * ps, Hkv, hd)
    return kv[:ctx_len]


def paged_attention_decode(q, kcache, vcache, page_table, ctx_lens, scale,
                           v_transposed=False):
    """q: [B, Hq, hd] -> out [B, Hq, hd]."""
    B, Hq, hd = q.shape
    Hkv = kcache.shape[1]
    G = Hq // Hkv
    outs = []
    for b in range(B):
        ctx = int(ctx_lens[b])
        kk = _gather_kv(kcache, page_table[b], ctx).float()  # [ctx, Hkv, hd]
        vv = _gather_kv(vcache, page_table[b], ctx, v_transposed).float()
        qq = q[b].float()                                    # [Hq, hd]
        kk = kk.repeat_interleave(G, dim=1)                  # [ctx, Hq, hd]
        vv = vv.repeat_interleave(G, dim=1)
        s = torch.einsum("hd,thd->ht", qq, kk) * scale       # [Hq, ctx]
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("ht,thd->hd", p, vv)
        outs.append(o)
    return torch.stack(outs).to(q.dtype)


def attention_prefill_paged(q, kcache, vcache, page_table, seq_q_start,
                            seq_q_len, seq_ctx_len, scale,
                            v_transposed=False):
    """Varlen causal attention where K/V come from the paged cache.

    q: [Tq, Hq, hd]; query token j of seq s sits at absolute position
    ctx_len - q_len + j and attends kv positions <= its own.
    """
    Tq, Hq, hd = q.shape
    Hkv = kcache.shape[1]
    G = Hq // Hkv
    out = torch.zeros_like(q)
    nseq = len(seq_q_len)
    for s in range(nseq):
        qs, ql, ctx = int(seq_q_start[s]), int(seq_q_len[s]), int(seq_ctx_len[s])
        if ql == 0:
            continue
        kk = _gather_kv(kcache, page_table[s], ctx).float()
        vv = _gather_kv(vcache, page_table[s], ctx, v_transposed).float()
        qq = q[qs:qs + ql].float()                           # [ql, Hq, hd]
        kk = kk.repeat_interleave(G, dim=1)
        vv = vv.repeat_interleave(G, dim=1)
        sc = torch.einsum("qhd,thd->hqt", qq, kk) * scale    # [Hq, ql, ctx]
        qpos = torch.arange(ctx - ql, ctx, device=q.device)
        tpos = torch.arange(ctx, device=q.device)
        mask = tpos[None, :] > qpos[:, None]                 # [ql, ctx]
        sc = sc.masked_fill(mask[None], float("-inf"))
        p = torch.softmax(sc, dim=-1)
        o = torch.einsum("hqt,thd->qhd", p, vv)
        out[qs:qs + ql] = o.to(q.dtype)
    return out


def greedy_sample(logits: torch.Tensor) -> torch.Tensor:
    return logits.argmax(dim=-1).to(torch.int32)


def topkp_keep_mask(logits: torch.Tensor, top_k, top_p) -> torch.Tensor:
    """The set a top-k / top-p filtered sampler may draw from: bool [B, V],
    computed per row in float64. `top_k` and `top_p` are scalars or [B].

    top-k first (off for k <= 0 or k >= V): every entry >= the k-th largest
    logit survives, so a tie at the boundary is kept whole. Then top-p (off
    for p >= 1) on the softmax over the survivors only: a token is kept iff
    the mass of the tokens strictly above it is <= top_p. Tokens with equal
    logits stand or fall together (a sort would split them by its own
    order), and the argmax is always kept, whatever top_p is. -inf entries
    are never kept unless the whole row is -inf. This is the keep set of
    engine/sampling.py::_filter_topk_topp wherever no tie straddles the
    nucleus boundary, and the contract of the HIP topkp_sample kernel."""
    x = logits.detach().cpu().double()
    B, V = x.shape
    ks = torch.as_tensor(top_k).reshape(-1).expand(B).tolist()
    ps = torch.as_tensor(top_p).double().reshape(-1).expand(B).tolist()
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b in range(B):
        row, k, p = x[b], int(ks[b]), ps[b]
        keep = row > float("-inf")
        if not bool(keep.any()):
            keep = torch.ones(V, dtype=torch.bool)
        if 0 < k < V:
            keep &= row >= torch.topk(row, k).values[-1]
        if p < 1.0:
            srt, idx = torch.sort(row.masked_fill(~keep, float("-inf")),
                                  descending=True, stable=True)
            prob = torch.softmax(srt, dim=-1)
            above = prob.cumsum(-1) - prob      # mass before each position
            # every member of a run of equal logits takes the run's first
            _, run, counts = torch.unique_consecutive(
                srt, return_inverse=True, return_counts=True)
            above = above[(counts.cumsum(0) - counts)[run]]
            nucleus = (above <= p) | (run == 0)
            keep &= torch.zeros(V, dtype=torch.bool).scatter(0, idx, nucleus)
        mask[b] = keep
    return mask


# --------------------------------------------------------------------------
# batched LoRA: every row picks its adapter from a bank by slot
def lora_shrink(t, x, A_bank, slots, ranks):
    """t[i, r] = sum_k x[i, k] * A_bank[slots[i], r, k] for r < ranks[slots[i]],
    in fp32. Rows with slots[i] < 0, and columns at r >= the rank, are not
    written. A per-row gather: nothing of the bank outside the named slot's
    first `rank` rows is read."""
    sl = slots.tolist()
    rk = ranks.tolist()
    for i, s in enumerate(sl):
        if s < 0 or rk[s] <= 0:
            continue
        r = rk[s]
        t[i, :r] = A_bank[s, :r].float() @ x[i].float()
    return t


def lora_expand_add(y, t, B_bank, slots, ranks, scales):
    """In place: y[i] = dtype(float(y[i]) + scales[s] * B_bank[s, :, :rank] @
    t[i, :rank]) with s = slots[i]: fp32 math, one rounding to y's dtype. Rows
    with slots[i] < 0 or rank 0 are left bit-untouched."""
    sl = slots.tolist()
    rk = ranks.tolist()
    sc = scales.tolist()
    for i, s in enumerate(sl):
        if s < 0 or rk[s] <= 0:
            continue
        r = rk[s]
        d = B_bank[s, :, :r].float() @ t[i, :r].float()
        y[i] = (y[i].float() + sc[s] * d).to(y.dtype)
    return y


# --------------------------------------------------------------------------
# Per-request logit processors: the contract of csrc/logits_process.hip.
# The bank `counts` is int32 [slots, V]: bit 0 of a word says the token occurs
# in the request's prompt, bits 1.. count its occurrences in the output.
PENALTY_PROMPT_BIT = 1
PENALTY_COUNT_ONE = 2


def penalty_fold(counts, slots, tokens, is_prompt):
    """Add entry i = (slots[i], tokens[i], is_prompt[i]) to the bank: set the
    prompt bit or add one to the output count. Entries that name a slot or a
    token outside the bank are skipped."""
    S, V = counts.shape
    for s, t, p in zip(slots.tolist(), tokens.tolist(), is_prompt.tolist()):
        if 0 <= s < S and 0 <= t < V:
            if p:
                counts[s, t] |= PENALTY_PROMPT_BIT
            else:
                counts[s, t] += PENALTY_COUNT_ONE
    return counts


def apply_logit_processors(logits, counts, slots, params, bias=None):
    """In place on fp32 logits [B, V], row b with params[b] = (repetition r,
    presence, frequency, min_p, temperature T), bank row slots[b] (-1: none)
    and bias = (offsets [B + 1], ids, vals) in CSR form or None, in this
    order, all in fp32:
      1. r != 1: l = l / r if l > 0 else l * r for every token in the prompt
         or the output
      2. l -= frequency * cnt + presence for every token with output count
         cnt > 0
      3. l[id] += val for the row's bias entries
      4. min_p > 0 and T > 0: l = -inf where (l - max l) / T < ln(min_p)
    A row with neutral parameters is not written."""
    B, V = logits.shape
    sl = slots.tolist()
    off = bias[0].tolist() if bias is not None else None
    for b in range(B):
        rep, pres, freq, min_p, temp = params[b].unbind()
        row = logits[b]
        s = sl[b]
        if (counts is not None and 0 <= s < counts.shape[0]
                and (rep != 1 or pres != 0 or freq != 0)):
            w = counts[s]
            cnt = w >> 1
            if rep != 1:
                pen = torch.where(row > 0, row / rep, row * rep)
                row.copy_(torch.where(w != 0, pen, row))
            row.copy_(torch.where(
                cnt > 0, row - (freq * cnt.float() + pres), row))
        if off is not None and off[b + 1] > off[b]:
            ids = bias[1][off[b]:off[b + 1]].long()
            ok = (ids >= 0) & (ids < V)
            row[ids[ok]] += bias[2][off[b]:off[b + 1]][ok]
        if min_p > 0 and temp > 0:
            drop = (row - row.max()) / temp < torch.log(min_p)
            row.masked_fill_(drop, float("-inf"))
    return logits
