"""Skinny-M decode weight GEMM (csrc/skinny_gemm_impl.h), its dispatch
(ops.linear) and the non-temporal K/V variant of the decode attention kernel.

Inputs are what the model has: x ~ N(0, 1), W ~ N(0, 0.02), bf16, seeded.
The accuracy criterion has no fixed tolerance: on the same tensors
e_new = max|kernel - ref| must not exceed 2 * e_lib = 2 * max|F.linear - ref|
with ref = x.double() @ W.double().T. Both paths round an fp32 sum to bf16; a
differently ordered fp32 sum can land across a rounding boundary, which turns
the library's half-ulp worst case into at most one ulp.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from dynamo_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (WPB, U, NT, nontemporal W loads, row-coalesced kernel)
DEFAULT_CFG = (8, 1, 2, True, True)


@functools.lru_cache(maxsize=None)
def _case(K, N):
    """Seeded (x16 [16, K], W [N, K], ref [16, N] float64); read-only."""
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 * K + N)
    x = torch.randn(16, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    return x, w, x.double() @ w.double().T


def _kernel(x, w, cfg=DEFAULT_CFG, y=None):
    if y is None:
        y = torch.empty(x.shape[0], w.shape[0], dtype=torch.bfloat16,
                        device=x.device)
    ops.hip().skinny_gemm(y, x, w, *cfg)
    return y


def _check_against_reference(M, K, N, cfg):
    x16, w, ref16 = _case(K, N)
    x, ref = x16[:M], ref16[:M]
    e_lib = (F.linear(x, w).double() - ref).abs().max().item()
    e_new = (_kernel(x, w, cfg).double() - ref).abs().max().item()
    print(f"M={M} K={K} N={N} cfg={cfg}: e_lib={e_lib:.6g} e_new={e_new:.6g}")
    assert e_new <= 2 * e_lib


SHAPES = [(K, N) for K in (2048, 3072) for N in (16, 48, 1040)] + [(28672, 48)]


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("K,N", SHAPES)
def test_matches_reference(M, K, N):
    _check_against_reference(M, K, N, DEFAULT_CFG)


SHIPPED_CFGS = sorted(set(ops.SKINNY_GEMM_SHAPES.values()) | {DEFAULT_CFG})


@pytest.mark.parametrize("cfg", SHIPPED_CFGS)
def test_shipped_configuration(cfg):
    # smallest N that fills one block (NT tiles) plus a ragged group (1 tile)
    _check_against_reference(16, 2048, cfg[2] * 16 + 16, cfg)


@pytest.mark.parametrize("cfg", SHIPPED_CFGS)
def test_batch_invariant_and_deterministic(cfg):
    x16, w, _ = _case(3072, 1040)
    y16 = _kernel(x16, w, cfg)
    assert torch.equal(y16, _kernel(x16, w, cfg))
    for m in (0, 7, 15):
        y1 = _kernel(x16[m:m + 1], w, cfg)
        assert torch.equal(y1[0], y16[m]), f"row {m} depends on M"


@pytest.mark.parametrize("M", [1, 3])
def test_writes_only_y(M):
    x16, w, _ = _case(2048, 48)
    N, pad = 48, 4096
    buf = torch.full((pad + M * N + pad,), 0x7B7B, dtype=torch.int16,
                     device=DEV)
    y = buf[pad:pad + M * N].view(torch.bfloat16).view(M, N)
    _kernel(x16[:M], w, y=y)
    torch.cuda.synchronize()
    assert (buf[:pad] == 0x7B7B).all() and (buf[pad + M * N:] == 0x7B7B).all()
    assert torch.equal(y, _kernel(x16[:M], w))


@pytest.mark.parametrize("M", [1, 3])
def test_reads_only_the_first_m_rows(M):
    x16, w, _ = _case(2048, 48)
    xbuf = torch.full_like(x16, float("nan"))
    xbuf[:M] = x16[:M]
    y = _kernel(xbuf[:M], w)
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y, _kernel(x16[:M].contiguous(), w))


def _ineligible_calls():
    g = torch.Generator(device=DEV)
    g.manual_seed(7)

    def t(*shape, dtype=torch.bfloat16, scale=1.0):
        return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)

    return {
        "M=17": (t(17, 2048), t(48, 2048, scale=0.02)),
        "K=1000": (t(16, 1000), t(48, 1000, scale=0.02)),
        "K=1024": (t(16, 1024), t(48, 1024, scale=0.02)),
        "N=40": (t(16, 2048), t(40, 2048, scale=0.02)),
        "fp16": (t(16, 2048, dtype=torch.float16),
                 t(48, 2048, dtype=torch.float16, scale=0.02)),
        "non-contiguous x": (t(16, 4096)[:, :2048], t(48, 2048, scale=0.02)),
        # contiguous, but starting 2 bytes into its buffer
        "misaligned x": (t(16 * 2048 + 8)[1:16 * 2048 + 1].view(16, 2048),
                         t(48, 2048, scale=0.02)),
    }


@pytest.fixture
def shipped_test_shapes(monkeypatch):
    """List the dispatch tests' (N, K) as shipped, so that only the
    eligibility rules and the switch decide where a call goes."""
    shapes = dict(ops.SKINNY_GEMM_SHAPES)
    for N, K in ((48, 2048), (48, 1000), (48, 1024), (40, 2048)):
        shapes[(N, K)] = DEFAULT_CFG
    monkeypatch.setattr(ops, "SKINNY_GEMM_SHAPES", shapes)
    monkeypatch.delenv("DYNAMO_SKINNY_GEMM", raising=False)
    ops.set_skinny_gemm(None)
    yield
    ops.set_skinny_gemm(None)


def test_dispatch_takes_kernel_when_eligible(shipped_test_shapes):
    x16, w, _ = _case(2048, 48)
    assert ops.skinny_gemm_config(x16, w) == DEFAULT_CFG
    assert torch.equal(ops.linear(x16, w), _kernel(x16, w))
    # a shape outside the shipped set stays on the library
    x, w2, _ = _case(2048, 1040)
    assert ops.skinny_gemm_config(x, w2) is None
    assert torch.equal(ops.linear(x, w2), F.linear(x, w2))


@pytest.mark.parametrize("case", ["M=17", "K=1000", "K=1024", "N=40", "fp16",
                                  "non-contiguous x", "misaligned x"])
def test_dispatch_ineligible_goes_to_library(shipped_test_shapes, case):
    x, w = _ineligible_calls()[case]
    if case == "misaligned x":
        assert x.is_contiguous() and x.data_ptr() % 16 == 2
    assert ops.skinny_gemm_config(x, w) is None
    assert torch.equal(ops.linear(x, w), F.linear(x, w))
    y = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=DEV)
    with pytest.raises(RuntimeError):
        ops.hip().skinny_gemm(y, x, w, *DEFAULT_CFG)


def test_dispatch_switch_off(shipped_test_shapes, monkeypatch):
    x16, w, _ = _case(2048, 48)
    lib = F.linear(x16, w)
    ops.set_skinny_gemm(False)
    assert ops.skinny_gemm_config(x16, w) is None
    assert torch.equal(ops.linear(x16, w), lib)
    ops.set_skinny_gemm(None)
    monkeypatch.setenv("DYNAMO_SKINNY_GEMM", "0")
    assert ops.skinny_gemm_config(x16, w) is None
    assert torch.equal(ops.linear(x16, w), lib)
    # the override wins over the environment
    ops.set_skinny_gemm(True)
    assert ops.skinny_gemm_config(x16, w) == DEFAULT_CFG


def test_load_pattern_and_policy_change_no_bits():
    """The row-coalesced kernel and the plain register-streaming one, with
    either W cache policy, do the same MFMAs in the same order at equal
    WPB: equal bits (N = 1040 leaves a ragged last group for NT = 2, 4)."""
    x16, w, _ = _case(3072, 1040)
    ref = _kernel(x16, w, (4, 4, 2, False, False))
    assert torch.equal(ref, _kernel(x16, w, (4, 4, 2, True, False)))
    assert torch.equal(ref, _kernel(x16, w, (4, 2, 2, False, True)))
    assert torch.equal(ref, _kernel(x16, w, (4, 2, 2, True, True)))
    ref8 = _kernel(x16, w, (8, 4, 2, False, False))
    assert torch.equal(ref8, _kernel(x16, w, (8, 1, 2, True, True)))
    assert torch.equal(ref8, _kernel(x16, w, (8, 1, 4, True, True)))
    # no K split (the shipped gate/up form): one accumulator sums K in order
    ref1 = _kernel(x16, w, (1, 8, 4, False, False))
    assert torch.equal(ref1, _kernel(x16, w, (1, 2, 2, True, True)))
    assert torch.equal(ref1, _kernel(x16, w, (1, 2, 4, True, True)))


def test_shipped_configurations_are_launchable():
    coalesced = set(ops.hip().skinny_gemm_configs()["bf16_coalesced"])
    for cfg in SHIPPED_CFGS:
        assert cfg[4] and cfg[:3] in coalesced


def test_binding_rejects_unknown_configuration():
    x16, w, _ = _case(2048, 48)
    y = torch.empty(16, 48, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.hip().skinny_gemm(y, x16, w, 3, 4, 2)
    with pytest.raises(RuntimeError):
        ops.hip().skinny_gemm(y, x16, w, 3, 1, 2, True, True)
    with pytest.raises(RuntimeError):   # K = 2048 is no multiple of 4*32*32
        ops.hip().skinny_gemm(y, x16, w, 4, 32, 2)


# ---- decode attention: non-temporal K/V loads change no arithmetic --------
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("ctxs", [(1, 33), (33, 513), (513, 1)])
def test_decode_attention_nt_bit_identical(ctxs, fp8):
    torch.manual_seed(3)
    Hkv, ps, hd, G = 8, 64, 128, 8
    Hq, B = G * Hkv, len(ctxs)
    P = sum((c + ps - 1) // ps for c in ctxs) + 1
    kc = torch.randn(P, Hkv, ps, hd, dtype=torch.bfloat16, device=DEV)
    vct = torch.randn(P, Hkv, hd, ps, dtype=torch.bfloat16, device=DEV)
    if fp8:
        kc, vct = kc.to(torch.float8_e4m3fn), vct.to(torch.float8_e4m3fn)
    pt = torch.zeros(B, (max(ctxs) + ps - 1) // ps, dtype=torch.int32,
                     device=DEV)
    nxt = 1
    for b, c in enumerate(ctxs):
        n = (c + ps - 1) // ps
        pt[b, :n] = torch.arange(nxt, nxt + n, dtype=torch.int32)
        nxt += n
    q = torch.randn(B, Hq, hd, dtype=torch.bfloat16, device=DEV)
    ctx_lens = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    scratch = ops.DecodeScratch(B, Hq, hd, max(ctxs), DEV)
    outs = [ops.paged_attention_decode(q, kc, vct, pt, ctx_lens, hd ** -0.5,
                                       scratch, v_transposed=True,
                                       nt_policy=nt).clone()
            for nt in (0, 1)]
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1])
