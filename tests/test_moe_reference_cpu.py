"""CPU checks of the MoE test machinery in tests/moe_cases.py.

1. Grouped GEMM: an fp32-accumulate, bf16-output stand-in meets the derived
   bound |out - ref| <= 2^-8 |ref| + 2^-12 A on every case the GPU module
   runs (worst ratio 0.87 here), and the bound REJECTS every
   mutation of the reference: the last 8 or the last 128 elements of k
   dropped, the first / last row of a segment computed with the neighbouring
   expert's weights, the last column zeroed, columns 0 and 1 swapped, row
   r0 + 16 of a long segment never written, every segment offset shifted by
   one.
2. `build_moe_tiles` partitions [0, sum) exactly and in order with
   1 <= m <= 16, every tile inside its expert's rows, none for an empty expert.
3. Gating: the CPU route of `ops.topk_gating` meets the gating reference on
   every case, ties included. `torch.topk` ordered ties differently from the
   kernel's "first lane holding best wins", so the CPU branch is a stable
   descending sort now and the CPU and GPU engines route alike.
4. Block: `MoEMLP.forward` on the CPU (fp32, per-expert loop route) meets the
   block bound at T in {1, 5, 64}, and the bound rejects every block mutation
   (two experts of a token swapped, weights unrenormalised, weights in
   unsorted order on sorted rows, a second expert dropped, gate and up halves
   swapped) at every T the GPU module runs.

tau_blk: the bf16-emulating reference is at most 0.01239 * S_row from the
fp64 one over T in {1, 5, 16, 64, 65, 256, 257}; tau_blk = 4 x that =
0.04958. Every block mutation is rejected at the factor of 4: the mildest is
the dropped second expert at T = 1, at 1.3 tau_blk (its weight is the largest
second weight of the case; test_block_mutations_rejected prints each ratio).
"weights in unsorted order" does not apply to a single token whose two
picks are already in expert order.
"""
import random

import pytest
import torch

from dynamo_amd import ops
from tests import moe_cases as mc

GEMM_PARAMS = mc.gemm_params()
GEMM_IDS = [mc.gemm_id(p) for p in GEMM_PARAMS]


# --------------------------------------------------------------------------
# grouped GEMM
# --------------------------------------------------------------------------
def _stand_in(case):
    """fp32 accumulation, one bf16 rounding."""
    out = torch.empty(case.T, case.N, dtype=torch.bfloat16)
    s = 0
    for e, n in enumerate(case.counts):
        if n:
            out[s:s + n] = (case.x[s:s + n].float()
                            @ case.w[e].float().T).to(torch.bfloat16)
        s += n
    return out


@pytest.mark.parametrize("p", GEMM_PARAMS, ids=GEMM_IDS)
def test_gemm_bound_and_mutations(p):
    _, counts, D, N = p
    case = mc.build_gemm_case(counts, D, N)
    worst = mc.assert_gemm_close(_stand_in(case), case.ref, case.A,
                                 what="fp32 stand-in")
    print(f"MOE_RATIO standin {worst:.4f}")
    # the reference itself passes, each mutation of it does not
    assert not mc.gemm_violates(case.ref, case.ref, case.A)
    applied = []
    for name, mutate in mc.GEMM_MUTATIONS.items():
        bad = mutate(case)
        if bad is None:
            continue
        applied.append(name)
        assert mc.gemm_violates(bad, case.ref, case.A), (
            f"{name} passes the bound on {mc.gemm_id(p)}")
    always = {"k_drop8", "last_col_zero", "swap_cols01", "seg_start_shift"}
    assert always <= set(applied)
    assert ("k_drop_chunk" in applied) == (D > 128)
    assert ("row16_unwritten" in applied) == (max(counts) > mc.TILE_M)


def test_gemm_params_coverage():
    kinds = {(k, D, N) for k, _, D, N in GEMM_PARAMS}
    assert {(k, D, N) for k, D, N in kinds if k == "nt2"} == {
        ("nt2", D, N) for D, N in mc.DN_NT2}
    assert all(N < 16384 for k, _, N in kinds if k == "nt2")
    assert all(N >= 16384 for k, _, N in kinds if k == "nt4")
    assert all(D <= mc.GEMM_MAX_D for _, D, _ in kinds)
    for c in mc.COUNTS:
        assert ("nt4", c, 128, 16384) in GEMM_PARAMS
    assert [c for k, c, D, N in GEMM_PARAMS if N == 16400] == [(1,), (33, 1)]


# --------------------------------------------------------------------------
# build_moe_tiles
# --------------------------------------------------------------------------
def _random_counts():
    rng = random.Random(7)
    return [tuple(rng.choice((0, 0, 1, 15, 16, 17, rng.randrange(71)))
                  for _ in range(rng.randrange(1, 10))) for _ in range(40)]


@pytest.mark.parametrize("counts", list(mc.COUNTS) + [(), (0,), (70, 0, 70)]
                         + _random_counts())
def test_build_moe_tiles(counts):
    tiles = ops.build_moe_tiles(list(counts))
    seg = [0]
    for c in counts:
        seg.append(seg[-1] + c)
    nxt = 0
    for e, r0, m in tiles:
        assert r0 == nxt, "tiles must partition [0, sum) in order"
        assert 1 <= m <= 16
        assert 0 <= e < len(counts)
        assert seg[e] <= r0 and r0 + m <= seg[e + 1], "tile leaves its expert"
        nxt = r0 + m
    assert nxt == sum(counts)
    assert {e for e, _, _ in tiles} == {e for e, c in enumerate(counts) if c}
    assert len(tiles) == sum((c + 15) // 16 for c in counts)


# --------------------------------------------------------------------------
# gating
# --------------------------------------------------------------------------
@pytest.mark.parametrize("E,K,T", mc.gating_params())
def test_gating_cpu_route(E, K, T):
    logits, kinds = mc.gating_logits(E, K, T)
    topw, topi = ops.topk_gating(logits, K)
    assert topw.dtype == torch.float32 and topi.dtype == torch.int32
    mc.assert_gating_matches(topw, topi, logits, K, what=f"cpu {kinds}")


def test_gating_cases_reach_every_kind():
    seen = set()
    for E, K, T in mc.gating_params():
        logits, kinds = mc.gating_logits(E, K, T)
        assert bool((logits * 8 == (logits * 8).round()).logical_or(
            logits.isinf()).all()), "logits must lie on the 1/8 grid"
        if T == 33:
            want = set(mc.ROW_KINDS)
            if E < 2:
                want = {"grid", "equal", "offset"}
            elif E <= K:
                want -= {"ktie", "neginf"}
            assert set(kinds) == want
        seen |= {(E, k) for k in kinds}
    for E in (4, 8, 60, 64):
        assert {k for e, k in seen if e == E} == set(mc.ROW_KINDS)


def test_gating_reference_rejects_wrong_tie_order():
    """The assertions see a tie resolved towards the higher index."""
    logits = torch.tensor([[1.0, 2.0, 2.0, 0.5]])
    ri, rw, _ = mc.gating_reference(logits, 1)
    assert ri.tolist() == [[1]]
    mc.assert_gating_matches(rw, ri, logits, 1)
    with pytest.raises(AssertionError):
        mc.assert_gating_matches(rw, torch.tensor([[2]]), logits, 1)
    with pytest.raises(AssertionError):          # repeated expert
        mc.assert_gating_matches(torch.tensor([[0.5, 0.5]]),
                                 torch.tensor([[1, 1]]), logits, 2)


# --------------------------------------------------------------------------
# block
# --------------------------------------------------------------------------
def test_tau_blk():
    worst = mc.emulated_worst_ratio()
    print(f"MOE_TAU_BLK emulated_worst {worst:.5f} factor {mc.BLK_FACTOR} "
          f"tau_blk {mc.tau_blk():.5f}")
    # bf16 roundings of O(1) values: a few 2^-9, far from a routing error
    assert 2.0 ** -11 < worst < 2.0 ** -6


@pytest.mark.parametrize("T", mc.BLK_TS)
def test_block_mutations_rejected(T):
    x = mc.block_x(T)
    logits = mc.cpu_block_logits(x)
    ref = mc.block_reference(x, logits)
    assert float(mc.block_ratio(ref, ref).max()) == 0.0
    for name in mc.BLOCK_MUTATIONS:
        bad = mc.block_reference(x, logits, mutation=name)
        if bad is None:                  # one token whose picks are in order
            assert name == "weights_unsorted" and T == 1
            continue
        ratio = float(mc.block_ratio(bad, ref).max())
        print(f"MOE_BLOCK_MUTATION T{T} {name} {ratio / mc.tau_blk():.1f}")
        with pytest.raises(AssertionError):
            mc.assert_block_close(bad, ref, what=name)


@pytest.mark.parametrize("T", (1, 5, 64))
def test_block_cpu_route(T):
    from dynamo_amd.models.layers import TPContext
    from dynamo_amd.models.mixtral import MoEMLP
    moe = MoEMLP(mc.block_config(), TPContext(), "cpu", torch.float32)
    mc.load_block_weights(moe)
    x = mc.block_x(T).float()
    logits = torch.nn.functional.linear(x, moe.router).float()
    with torch.no_grad():
        out = moe.forward(x)
    ref = mc.block_reference(x, logits)
    worst = mc.assert_block_close(out, ref, what=f"cpu loop T={T}")
    print(f"MOE_BLOCK_RATIO cpu_loop T{T} {worst:.4f}")
