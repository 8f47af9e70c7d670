"""Paged decode / prefill attention kernels against an fp64 reference, on
cases where a dropped, leaked or misplaced token is an O(1) error.

Cases, structured queries, the reference and the row-scaled comparison
(|out - ref| <= TAU * A[row], TAU = 2^-7, never tuned per path) live in
tests/attention_cases.py; tests/test_attention_reference_cpu.py shows on
the CPU that the comparison rejects each of those bugs. Here every kernel
path runs with scattered page ids, a page table wider than needed, NaN in
the null page / spare pages / page tails, ctx_len == 0 rows inside the
batch, a NaN-prefilled `out`, and (decode) a scratch larger than the batch.

Measured max err / (TAU * A) per kernel path on MI355X (worst case of this
module; the bound is 1.0):

    decode path (phase-1 kernel)                    chunk 512  1024  2048
    valu          paged_decode_phase1, G 1/2/4,       0.475  0.386 0.422
                  G 8 at page 16 or DYNAMO_DECODE_MFMA=0
    mfma_swapped  G 3/5/6/7/8/16, token-major bf16    0.742  0.770 0.422
    mfma_a        same cases, DYNAMO_DECODE_SWAPPED=0 0.742  0.770 0.422
    mfma_swapped  token-major fp8                     0.585
    vt4           d-major V bf16 (nt_policy 0 and 1)  0.649  0.659 0.428
    vt4           d-major V fp8  (nt_policy 0 and 1)  0.551

    prefill path           bf16   bf16 d-major   fp8    fp8 d-major
    prefill16 (G 1, 7)     0.447  0.483          -      -
    prefill32 GSPLIT 4     0.563  0.495          0.460  0.444
    prefill32 GSPLIT 2     0.567  0.451          0.438  0.487
    prefill32 GSPLIT 1     0.440  0.663          0.447  0.470

No path needed a wider TAU. The one failure these tests found on the
unchanged kernels was the pad-row contract: with one chunk (C == 1) all
three phase-1 kernels returned from `chunk_start >= ctx` without writing the
row, so a ctx_len == 0 row kept whatever `out` held (NaN here, stale memory
from `empty_like` in the engine). The early exit now stores zeros.
"""
import os
import subprocess
import sys

import pytest
import torch

from dynamo_amd import ops
from tests import attention_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flag(name):
    e = os.environ.get(name)
    return e is None or not e.startswith("0")


def _token_major_path(G, ps, fp8=False):
    """Name of the phase-1 kernel attention_decode.hip dispatches to."""
    if fp8:
        return "mfma_swapped_fp8"
    if G in (1, 2, 4):
        return "valu"
    mfma_ok = ps % 32 == 0
    if G == 8 and not (mfma_ok and _flag("DYNAMO_DECODE_MFMA")):
        return "valu"
    return "mfma_swapped" if _flag("DYNAMO_DECODE_SWAPPED") else "mfma_a"


def _record(path, worst):
    print(f"ATTN_RATIO {path} {worst:.4f}")


def _run_decode(case, scratch, *, nt_policy=-1, what=""):
    q, kc, vc, pt, ctx = case.device_args(DEV)
    out = torch.full_like(q, float("nan"))
    got = ops.paged_attention_decode(q, kc, vc, pt, ctx, case.scale, scratch,
                                     out=out, v_transposed=case.v_transposed,
                                     nt_policy=nt_policy)
    torch.cuda.synchronize()
    return got


def _scratch_for(case, max_ctx=None, extra_batch=0):
    B, Hq = case.q.shape[:2]
    return ops.DecodeScratch(B + extra_batch, Hq, ac.HD,
                             max(case.ctxs) if max_ctx is None else max_ctx,
                             DEV)


# --------------------------------------------------------------------------
# decode, token-major bf16
# --------------------------------------------------------------------------
TM_PARAMS = ac.decode_token_major_params()


@pytest.mark.parametrize(
    "G,Hkv,ps,ci", TM_PARAMS,
    ids=[f"G{G}_hkv{h}_ps{ps}_c{ci}" for G, h, ps, ci in TM_PARAMS])
def test_decode_token_major_bf16(G, Hkv, ps, ci):
    case = ac.build_decode_case(G, Hkv, ps, ac.CTX_LISTS[ci])
    ref, A = ac.decode_reference(case)
    got = _run_decode(case, _scratch_for(case))
    path = _token_major_path(G, ps)
    _record(path, ac.assert_attention_close(got, ref, A, what=path))


# --------------------------------------------------------------------------
# scratch sized for a larger engine than the batch needs
# --------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tokmajor", "dmajor"])
@pytest.mark.parametrize("G", [4, 8], ids=["G4_", "G8_"])
@pytest.mark.parametrize("max_ctx,chunk,ctxs", ac.OVERSIZED,
                         ids=[f"ck{c}" for _, c, _ in ac.OVERSIZED])
def test_decode_oversized_scratch(max_ctx, chunk, ctxs, G, layout):
    vt = layout == "dmajor"
    case = ac.build_decode_case(G, 2 if G == 4 else 1, 64, ctxs, chunk=chunk,
                                v_transposed=vt)
    scratch = _scratch_for(case, max_ctx=max_ctx, extra_batch=3)
    assert scratch.chunk_tokens == chunk
    assert scratch.chunks == max_ctx // chunk
    ref, A = ac.decode_reference(case)
    got = _run_decode(case, scratch)
    path = ("vt4_bf16" if vt else _token_major_path(G, 64)) + f"_ck{chunk}"
    _record(path, ac.assert_attention_close(got, ref, A, what=path))


# --------------------------------------------------------------------------
# decode, d-major V (v_transposed), bf16 and fp8, both K/V load policies
# --------------------------------------------------------------------------
DM_PARAMS = [(G, h, ps, ci, fp8)
             for G, h, ps, c0, c1, fp8 in ac.decode_d_major_params()
             for ci in (c0, c1)]


@pytest.mark.parametrize(
    "G,Hkv,ps,ci,fp8", DM_PARAMS,
    ids=[f"G{G}_hkv{h}_ps{ps}_c{ci}_{'fp8' if f else 'bf16'}"
         for G, h, ps, ci, f in DM_PARAMS])
def test_decode_d_major(G, Hkv, ps, ci, fp8):
    case = ac.build_decode_case(G, Hkv, ps, ac.CTX_LISTS[ci],
                                v_transposed=True, fp8=fp8)
    ref, A = ac.decode_reference(case)
    scratch = _scratch_for(case)
    outs = []
    for nt in (0, 1):
        got = _run_decode(case, scratch, nt_policy=nt)
        path = f"vt4_{'fp8' if fp8 else 'bf16'}" + ("_nt" if nt else "")
        _record(path, ac.assert_attention_close(got, ref, A, what=path))
        outs.append(got)
    # the load policy changes no arithmetic
    assert torch.equal(outs[0], outs[1])


# --------------------------------------------------------------------------
# decode, fp8 token-major
# --------------------------------------------------------------------------
F8_PARAMS = [(G, h, ps, ci)
             for G, h, ps, c0, c1 in ac.decode_fp8_token_major_params()
             for ci in (c0, c1)]


@pytest.mark.parametrize(
    "G,Hkv,ps,ci", F8_PARAMS,
    ids=[f"G{G}_hkv{h}_ps{ps}_c{ci}" for G, h, ps, ci in F8_PARAMS])
def test_decode_fp8_token_major(G, Hkv, ps, ci):
    case = ac.build_decode_case(G, Hkv, ps, ac.CTX_LISTS[ci], fp8=True)
    ref, A = ac.decode_reference(case)
    got = _run_decode(case, _scratch_for(case))
    path = _token_major_path(G, ps, fp8=True)
    _record(path, ac.assert_attention_close(got, ref, A, what=path))


# --------------------------------------------------------------------------
# pad rows: graphs.py pads captured batches with ctx_len == 0 rows; their
# outputs feed the o-projection, so they must be zeros, not stale memory
# --------------------------------------------------------------------------
PAD_PATHS = {
    # name: (G, Hkv, v_transposed, fp8)
    "G2_tokmajor": (2, 2, False, False),    # VALU, one token-group merge
    "G4_tokmajor": (4, 1, False, False),    # VALU, production G=4
    "G8_tokmajor": (8, 1, False, False),    # MFMA (swapped / A / VALU by env)
    "G7_tokmajor_fp8": (7, 1, False, True),
    "G8_dmajor": (8, 1, True, False),
    "G3_dmajor_fp8": (3, 2, True, True),
}


@pytest.mark.parametrize("ctxs", [(0, 40, 0, 7), (0, 600, 0, 7)],
                         ids=["C1", "C2"])
@pytest.mark.parametrize("name", list(PAD_PATHS))
def test_decode_pad_rows(name, ctxs):
    G, Hkv, vt, fp8 = PAD_PATHS[name]
    case = ac.build_decode_case(G, Hkv, 64, ctxs, v_transposed=vt, fp8=fp8)
    scratch = _scratch_for(case)
    assert scratch.chunks == (1 if max(ctxs) <= 512 else 2)
    got = _run_decode(case, scratch)
    for b, c in enumerate(ctxs):
        if c == 0:
            row = got[b].float().cpu()
            assert bool((row == 0).all()), (
                f"{name}: pad row {b} is not zero "
                f"({int(row.isnan().sum())} NaN of {row.numel()})")
    ref, A = ac.decode_reference(case)
    ac.assert_attention_close(got, ref, A, what=name)


# --------------------------------------------------------------------------
# prefill
# --------------------------------------------------------------------------
def _prefill_path(G, vt, fp8):
    base = f"prefill32_gsplit{8 // G}" if G in (2, 4, 8) else "prefill16"
    return base + ("_vt" if vt else "") + ("_fp8" if fp8 else "")


def _check_prefill(G, Hkv, ps, si, vt, fp8):
    case = ac.build_prefill_case(G, Hkv, ps, ac.PREFILL_SPECS[si],
                                 v_transposed=vt, fp8=fp8)
    ref, A = ac.prefill_reference(case)
    q, kc, vc, pt, st, ln, cx = case.device_args(DEV)
    got = ops.attention_prefill_paged(q, kc, vc, pt, st, ln, cx, case.scale,
                                      v_transposed=vt)
    torch.cuda.synchronize()
    path = _prefill_path(G, vt, fp8)
    _record(path, ac.assert_attention_close(got, ref, A, what=path))


def _prefill_ids(params):
    return [f"G{G}_hkv{h}_ps{ps}_s{si}_{'dmajor' if vt else 'tokmajor'}"
            for G, h, ps, si, vt in params]


@pytest.mark.parametrize("G,Hkv,ps,si,vt", ac.prefill_params(),
                         ids=_prefill_ids(ac.prefill_params()))
def test_prefill(G, Hkv, ps, si, vt):
    _check_prefill(G, Hkv, ps, si, vt, fp8=False)


@pytest.mark.parametrize("G,Hkv,ps,si,vt", ac.prefill_fp8_params(),
                         ids=_prefill_ids(ac.prefill_fp8_params()))
def test_prefill_fp8(G, Hkv, ps, si, vt):
    """fp8 caches against the reference on the DEQUANTISED cache, at the
    same TAU as bf16 (the kernel converts e4m3 -> bf16 exactly)."""
    _check_prefill(G, Hkv, ps, si, vt, fp8=True)


# --------------------------------------------------------------------------
# fallback variants: the selection flags are read once per process, so each
# variant gets a fresh child pytest over the bf16 token-major cases it serves
# --------------------------------------------------------------------------
def _run_variant(env_extra, kexpr):
    env = dict(os.environ, **env_extra)
    out = subprocess.run(
        [sys.executable, "-m", "pytest", "tests/test_gpu_attention_edges.py",
         "-q", "-s", "-k", kexpr, "-m", "gpu", "-p", "no:cacheprovider"],
        capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    for line in out.stdout.splitlines():
        if "ATTN_RATIO" in line:     # pass the child's measurements on
            print(line[line.index("ATTN_RATIO"):])
    assert out.returncode == 0, out.stdout[-3000:]
    assert " passed" in out.stdout and "no tests ran" not in out.stdout


def test_decode_valu_g8_subprocess():
    """DYNAMO_DECODE_MFMA=0 sends G=8 to the VALU kernel (G=16 and the odd
    groups have no VALU kernel and ignore the flag)."""
    _run_variant(
        {"DYNAMO_DECODE_MFMA": "0"},
        "(test_decode_token_major_bf16 and G8_) or "
        "(test_decode_oversized_scratch and G8_ and tokmajor) or "
        "(test_decode_pad_rows and G8_tokmajor)")


def test_decode_mfma_a_variant_subprocess():
    """DYNAMO_DECODE_SWAPPED=0 selects the A-operand MFMA kernel for every
    group the swapped kernel serves by default."""
    _run_variant(
        {"DYNAMO_DECODE_SWAPPED": "0"},
        "(test_decode_token_major_bf16 and not ps16 and "
        "(G3_ or G5_ or G6_ or G7_ or G8_ or G16_)) or "
        "(test_decode_oversized_scratch and G8_ and tokmajor) or "
        "(test_decode_pad_rows and G8_tokmajor)")
