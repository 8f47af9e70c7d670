"""CPU checks of the attention test machinery in tests/attention_cases.py.

1. `torch_ref` (the CPU engine path and the oracle of every older attention
   test) meets the row-scaled bound against the independent fp64 reference
   on the same cases the GPU edge module runs, d-major V and ctx_len == 0
   rows included.
2. Teeth: the comparison must REJECT a reference that drops the last token,
   reads one token past ctx, drops the last 32-token tile, swaps two
   page-table entries, token-reverses a V page or follows an unused
   page-table entry; for prefill, a causal mask shifted by +1 or -1. The
   fixed-atol comparison of the older tests accepts most of these.

Page swap: attention is invariant under a permutation of whole (K, V) token
pairs, so swapping two full pages for K and V together computes the same
output and no comparison can see it. The mutation therefore swaps the
entries in the table the K gather uses (a kernel that resolves K and V
pages differently, or a page in the wrong order for one of them).
"""
import pytest
import torch

from tests import attention_cases as ac
from dynamo_amd.ops import torch_ref


def _decode_keys():
    keys = []
    for G, Hkv, ps, ci in ac.decode_token_major_params():
        keys.append((G, Hkv, ps, ac.CTX_LISTS[ci], 512, False, False))
    for _, chunk, ctxs in ac.OVERSIZED:
        for G in (4, 8):
            for vt in (False, True):
                keys.append((G, 2 if G == 4 else 1, 64, ctxs, chunk, vt,
                             False))
    for G, Hkv, ps, c0, c1, fp8 in ac.decode_d_major_params():
        for ci in (c0, c1):
            keys.append((G, Hkv, ps, ac.CTX_LISTS[ci], 512, True, fp8))
    for G, Hkv, ps, c0, c1 in ac.decode_fp8_token_major_params():
        for ci in (c0, c1):
            keys.append((G, Hkv, ps, ac.CTX_LISTS[ci], 512, False, True))
    return sorted(set(keys))


def _prefill_keys():
    keys = [(G, Hkv, ps, ac.PREFILL_SPECS[si], vt, False)
            for G, Hkv, ps, si, vt in ac.prefill_params()]
    keys += [(G, Hkv, ps, ac.PREFILL_SPECS[si], vt, True)
             for G, Hkv, ps, si, vt in ac.prefill_fp8_params()]
    return sorted(set(keys))


def _did(k):
    G, Hkv, ps, ctxs, chunk, vt, fp8 = k
    return (f"G{G}_hkv{Hkv}_ps{ps}_ctx{'-'.join(map(str, ctxs))}_ck{chunk}"
            f"_{'dm' if vt else 'tm'}_{'fp8' if fp8 else 'bf16'}")


def _pid(k):
    G, Hkv, ps, spec, vt, fp8 = k
    return (f"G{G}_hkv{Hkv}_ps{ps}_"
            + "-".join(f"{a}x{b}" for a, b in spec)
            + f"_{'dm' if vt else 'tm'}_{'fp8' if fp8 else 'bf16'}")


DECODE_KEYS = _decode_keys()
PREFILL_KEYS = _prefill_keys()


def _decode_case(k):
    G, Hkv, ps, ctxs, chunk, vt, fp8 = k
    return ac.build_decode_case(G, Hkv, ps, ctxs, chunk=chunk,
                                v_transposed=vt, fp8=fp8)


def _prefill_case(k):
    G, Hkv, ps, spec, vt, fp8 = k
    return ac.build_prefill_case(G, Hkv, ps, spec, v_transposed=vt, fp8=fp8)


def _ref_caches(case):
    """torch_ref indexes the caches on the CPU, where float8 tensors cannot
    be indexed; the dequantised bf16 copy holds the same values exactly."""
    if case.fp8:
        return case.kcache.to(torch.bfloat16), case.vcache.to(torch.bfloat16)
    return case.kcache, case.vcache


@pytest.mark.parametrize("key", DECODE_KEYS, ids=_did)
def test_decode_reference_and_teeth(key):
    case = _decode_case(key)
    ref, A, weights = ac.decode_reference(case, return_weights=True)
    assert bool(torch.isfinite(ref).all())
    ctxs, ps, G = case.ctxs, case.ps, case.G
    live = [b for b, c in enumerate(ctxs) if c > 0]

    # every needle really dominates its row
    for b, h, t, _ in case.needles:
        w = float(weights[b][h, t])
        assert w >= 0.5, (b, h, t, w)

    # --- torch_ref meets the bound; ctx_len == 0 rows are zeros
    kc, vc = _ref_caches(case)
    got = torch_ref.paged_attention_decode(
        case.q, kc, vc, case.page_table, case.ctx_lens, case.scale,
        v_transposed=case.v_transposed)
    ac.assert_attention_close(got, ref, A, what="torch_ref decode")
    for b, c in enumerate(ctxs):
        if c == 0:
            assert bool((got[b] == 0).all())

    def rows_caught(mut):
        return ac.violates(mut, ref, A).any(dim=1)

    def expect(mut, name, rows):
        caught = rows_caught(mut)
        assert bool(caught.any()), f"{name}: not caught"
        for b in rows:
            assert bool(caught[b]), f"{name}: row {b} (ctx {ctxs[b]}) passes"

    # rows that carry a tail needle must each see the three length bugs
    tail_rows = sorted({b for b, _, _, kind in case.needles if kind == "tail"})
    mut, _ = ac.decode_reference(case, ctx_lens=[max(c - 1, 0) for c in ctxs])
    expect(mut, "ctx-1", tail_rows)
    mut, _ = ac.decode_reference(case, ctx_lens=[c + 1 for c in ctxs])
    assert not bool(torch.isfinite(mut).all())
    expect(mut, "ctx+1", range(len(ctxs)))
    mut, _ = ac.decode_reference(
        case, ctx_lens=[((c - 1) // ac.TILE) * ac.TILE if c else 0
                        for c in ctxs])
    expect(mut, "last tile dropped", tail_rows)

    # two page-table entries swapped (K side, see the module docstring):
    # every multi-page row must be caught
    multi = [b for b in live if case.npages(b) > 1]
    if multi:
        kt = case.page_table.clone()
        for b in multi:
            last = case.npages(b) - 1
            kt[b, 0], kt[b, last] = case.page_table[b, last], case.page_table[b, 0]
        mut, _ = ac.decode_reference(case, k_table=kt)
        expect(mut, "page swap", multi)

    # one V page token-reversed: the page of the row's first needle
    first = {}
    for b, _, t, _ in case.needles:
        first.setdefault(b, t // ps)
    mut, _ = ac.decode_reference(
        case, v_reversed={b: first.get(b, 0) for b in live})
    expect(mut, "V page reversed", sorted(first))

    # one unused page-table entry used: reads the null page
    bad = case.page_table.clone()
    for b in live:
        bad[b, 0] = case.page_table[b, case.npages(b)]
    mut, _ = ac.decode_reference(case, k_table=bad, v_table=bad)
    expect(mut, "unused page-table entry", live)


@pytest.mark.parametrize("key", PREFILL_KEYS, ids=_pid)
def test_prefill_reference_and_teeth(key):
    case = _prefill_case(key)
    assert case.n_lures > 0
    ref, A = ac.prefill_reference(case)
    assert bool(torch.isfinite(ref).all())
    kc, vc = _ref_caches(case)
    got = torch_ref.attention_prefill_paged(
        case.q, kc, vc, case.page_table, case.seq_q_start, case.seq_q_len,
        case.seq_ctx_len, case.scale, v_transposed=case.v_transposed)
    ac.assert_attention_close(got, ref, A, what="torch_ref prefill")
    for shift in (+1, -1):
        mut, _ = ac.prefill_reference(case, mask_shift=shift)
        caught = ac.violates(mut, ref, A).any(dim=1)
        # every sequence of the case must see the shifted mask, except that
        # a leak cannot show where no future token exists (a (1, 1) row)
        for s, (ql, ctx) in enumerate(case.spec):
            if shift == +1 and ctx == 1:
                continue
            qs = int(case.seq_q_start[s])
            assert bool(caught[qs:qs + ql].any()), (shift, s, ql, ctx)


def test_old_comparison_is_blind_where_the_new_one_is_not():
    """Why the new comparison exists: on randn data at ctx 2048 the fixed
    rtol=atol=2e-2 comparison of test_gpu_kernels.py accepts a dropped last
    token; the row-scaled bound on a needle case rejects it."""
    torch.manual_seed(0)
    ctx, Hq = 2048, 8
    q = torch.randn(Hq, ac.HD).bfloat16().double()
    k = torch.randn(ctx, 1, ac.HD).bfloat16().double()
    v = torch.randn(ctx, 1, ac.HD).bfloat16().double()
    full, _, _ = ac._attend(q, k, v, Hq)
    cut, _, _ = ac._attend(q, k[:-1], v[:-1], Hq)
    assert torch.allclose(cut, full, rtol=2e-2, atol=2e-2)
    case = ac.build_decode_case(8, 1, 64, [ctx], chunk=1024)
    ref, A = ac.decode_reference(case)
    mut, _ = ac.decode_reference(case, ctx_lens=[ctx - 1])
    assert bool(ac.violates(mut, ref, A).any())
