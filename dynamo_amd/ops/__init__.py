"""Op dispatch: native HIP kernels on GPU, torch reference on CPU.

On a GPU box the HIP extension is REQUIRED — a missing/failed extension
raises instead of silently falling back to eager PyTorch, so GPU tests can
never pass on a non-native path.
"""
from __future__ import annotations

import torch

from . import fp8_weights, mxfp4_weights, torch_ref
from .fp8_weights import (Fp8Weight, quantize_fp8_rowwise,  # re-export
                          quantize_model_fp8)
from .mxfp4_weights import (Mxfp4Weight, quantize_mxfp4,  # re-export
                            quantize_model_mxfp4)
from .torch_ref import make_cos_sin_cache  # re-export

_hip_mod = None
_hip_err: Exception | None = None


def hip():
    """The native kernel extension; raises loudly if unavailable."""
    global _hip_mod, _hip_err
    if _hip_mod is None:
        try:
            from dynamo_amd import _hip as m  # built in-tree by setup.py
            _hip_mod = m
        except Exception as e:  # pragma: no cover
            _hip_err = e
            raise RuntimeError(
                "dynamo_amd._hip native extension is not available on a GPU "
                "device path. Build it with `python setup.py build_ext "
                f"--inplace` (PYTORCH_ROCM_ARCH=gfx950). Original error: {e}"
            ) from e
    return _hip_mod


def hip_available() -> bool:
    try:
        hip()
        return True
    except RuntimeError:
        return False


# --------------------------------------------------------------------------
# Decode weight GEMMs: (N, K) -> (WPB, U, NT, non-temporal W loads,
# row-coalesced kernel) of the in-tree skinny-M kernel
# (csrc/skinny_gemm_impl.h). A shape is listed only if (a) the kernel's
# result is bit-identical to the library's for it, so the model computes
# what it computed before, and (b) its in-situ trace average beat
# hipBLASLt's in both of two paired runs (profiles/README.md, "Decode weight
# GEMMs in-tree"). Everything else stays on the library.
SKINNY_GEMM_SHAPES: dict = {
    # gate/up: hipBLASLt's kernel for it sums K in order in one accumulator
    # with the same MFMA; so does WPB = 1 (0 of 917504 outputs differ)
    (57344, 8192): (1, 2, 2, True, True),
    # qkv (10240, 8192), o (8192, 8192), down (8192, 28672): the K-split
    # configurations (8, 1, 4) / (8, 1, 2) / (4, 2, 2) are 1-18 % faster in
    # situ, but the library splits K its own way there and 0.04-0.08 % of the
    # outputs differ by a bf16 rounding flip whatever WPB is; after 40 decode
    # steps that changes the sampled tokens. Not shipped.
    # lm_head (128256, 8192): not shown faster in situ. Not shipped.
}

_skinny_override: "bool | None" = None


def set_skinny_gemm(on: "bool | None") -> None:
    """In-process override of DYNAMO_SKINNY_GEMM (None = follow the env)."""
    global _skinny_override
    _skinny_override = on


def skinny_gemm_enabled() -> bool:
    if _skinny_override is not None:
        return _skinny_override
    from dynamo_amd import envs
    return envs.get("DYNAMO_SKINNY_GEMM", True, bool)


def skinny_gemm_config(x: torch.Tensor, w: torch.Tensor):
    """The shape's SKINNY_GEMM_SHAPES entry if x @ w^T runs on the skinny-M
    kernel, else None."""
    if not (x.is_cuda and x.dim() == 2 and w.dim() == 2
            and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16):
        return None
    M, K = x.shape
    N = w.shape[0]
    cfg = SKINNY_GEMM_SHAPES.get((N, K))
    if cfg is None or not 1 <= M <= 16 or w.shape[1] != K:
        return None
    kstep = cfg[0] * cfg[1] * (64 if cfg[4] else 32)
    if N % 16 or K < 2048 or K % kstep:
        return None
    if not (x.is_contiguous() and w.is_contiguous()
            and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0):
        return None
    return cfg if skinny_gemm_enabled() else None


# --------------------------------------------------------------------------
# FP8 (e4m3) weights, W8A16 (ops/fp8_weights.py, the Fp8Coal format of
# csrc/skinny_gemm_impl.h). (WPB, U, NT) points of fp8_skinny_gemm the binding
# can launch; it needs K % (WPB * 128 * U) == 0. A copy of the header's
# FP8_GEMM_CONFIGS that tests can read without the extension; they check it
# against hip().skinny_gemm_configs(). Non-temporal W loads throughout.
FP8_GEMM_CONFIGS: tuple = (
    (1, 1, 1), (1, 1, 2), (1, 2, 2), (2, 1, 4), (2, 2, 2),
    (4, 1, 2), (4, 2, 2), (4, 1, 4), (8, 1, 2), (8, 2, 2),
)
# The default configuration: accepts every K % 128 == 0. A shape outside the
# table takes FP8_GEMM_SPLIT_K instead when K allows (its 4-wave K split was
# 1.4-1.7x the bf16 dispatch on all four 70B layer shapes at M = 16, where
# the default ranges from 0.5x to 1.6x), else the default.
FP8_GEMM_DEFAULT: tuple = (1, 1, 2)
FP8_GEMM_SPLIT_K: tuple = (4, 1, 2)
# (N, K) -> ((WPB, U, NT) for M <= 16, (WPB, U, NT) for 16 < M <= 64) for the
# llama-3-70b layer shapes: the cold-sweep winners at M = 16 and M = 64
# (kernel_bench.py --which fp8sweep; profiles/README.md, "FP8 weights")
FP8_GEMM_SHAPES: dict = {
    (10240, 8192): ((4, 1, 2), (4, 1, 4)),    # qkv
    (8192, 8192): ((8, 1, 2), (4, 1, 2)),     # o
    (57344, 8192): ((4, 1, 4), (2, 1, 4)),    # gate/up
    (8192, 28672): ((4, 2, 2), (4, 1, 2)),    # down
}
FP8_GEMM_MAX_M = 64


def _quant_gemm_config(M, N, K, kstep, max_m, shapes, split_k, default):
    """The (WPB, U, NT) of a quantised-weight GEMM whose steps are kstep k:
    the shape's table entry (first for M <= 16, second above), else split_k,
    else, where K does not allow that, default. None if the kernel does not
    take the shape."""
    if not (1 <= M <= max_m and K >= kstep and K % kstep == 0
            and N >= 16 and N % 16 == 0):
        return None
    entry = shapes.get((N, K))
    cfg = entry[0 if M <= 16 else 1] if entry else split_k
    if K % (cfg[0] * kstep * cfg[1]):
        cfg = default
    return cfg


def _quant_linear_path(x, w, dequant_k, gemm_config):
    """("kernel", cfg) | ("dequant", None) | ("torch", None) for linear(x, w)
    with a quantised weight holder w whose dequantise kernel needs
    K % dequant_k == 0."""
    N, K = w.shape
    if not x.is_cuda:
        return "torch", None
    if x.dtype != torch.bfloat16 or K % dequant_k or x.shape[-1] != K:
        return "torch", None
    if x.dim() == 2 and x.is_contiguous() and x.data_ptr() % 16 == 0:
        cfg = gemm_config(x.shape[0], N, K)
        if cfg is not None:
            return "kernel", cfg
    return "dequant", None


def _linear_quant(x, w, path, cfg, gemm: str, dequant: str, glu=False):
    """linear(x, w) on `path`; gemm and dequant name the format's bindings.
    glu (kernel path only): the fused SwiGLU form, y = [M, N / 2]."""
    if path == "kernel":
        y = torch.empty(x.shape[0], w.shape[0] // 2 if glu else w.shape[0],
                        dtype=x.dtype, device=x.device)
        getattr(hip(), gemm)(y, x, w.q, w.scale, *cfg, True, glu)
        return y
    if path == "dequant":
        w_eff = fp8_weights.scratch_view(w)
        getattr(hip(), dequant)(w_eff, w.q, w.scale)
        return torch.nn.functional.linear(x, w_eff)
    return torch.nn.functional.linear(x, w.effective(x.dtype))


def fp8_gemm_config(M: int, N: int, K: int):
    """The (WPB, U, NT) fp8_skinny_gemm runs an [M, K] x [N, K]^T call at, or
    None if the kernel does not take the shape."""
    return _quant_gemm_config(M, N, K, 128, FP8_GEMM_MAX_M, FP8_GEMM_SHAPES,
                              FP8_GEMM_SPLIT_K, FP8_GEMM_DEFAULT)


def fp8_linear_path(x: torch.Tensor, w: Fp8Weight):
    """Where linear(x, w) runs for an Fp8Weight: ("kernel", (WPB, U, NT)) for
    the in-tree W8A16 kernel, ("dequant", None) for fp8_dequant into the
    scratch buffer + the library GEMM, ("torch", None) for F.linear(x, W_eff)
    with W_eff formed by torch (CPU, or a GPU call fp8_dequant cannot
    serve)."""
    return _quant_linear_path(x, w, 16, fp8_gemm_config)


def _linear_fp8(x: torch.Tensor, w: Fp8Weight) -> torch.Tensor:
    return _linear_quant(x, w, *fp8_linear_path(x, w), "fp8_skinny_gemm",
                         "fp8_dequant")


# --------------------------------------------------------------------------
# MXFP4 (e2m1 + e8m0) weights, W4A16 (ops/mxfp4_weights.py, the Mxfp4Coal
# format of csrc/skinny_gemm_impl.h). (WPB, U, NT) points of mxfp4_skinny_gemm
# the binding can launch; it needs K % (WPB * 256 * U) == 0. A copy of the
# header's MXFP4_GEMM_CONFIGS that tests can read without the extension; they
# check it against hip().skinny_gemm_configs(). Non-temporal W loads
# throughout.
MXFP4_GEMM_CONFIGS: tuple = (
    (1, 1, 1), (1, 1, 2), (1, 2, 2), (2, 1, 2), (2, 1, 4), (4, 1, 2),
    (4, 1, 4), (4, 1, 8), (8, 1, 2), (8, 1, 4), (2, 1, 8),
)
# The default configuration accepts every K % 256 == 0; a shape outside the
# table takes the 4-wave K split when K allows, as for fp8 (1.4-2.1x the bf16
# dispatch on all four 70B layer shapes at M = 16, where the default ranges
# from 0.9x to 2.1x).
MXFP4_GEMM_DEFAULT: tuple = (1, 1, 2)
MXFP4_GEMM_SPLIT_K: tuple = (4, 1, 2)
# (N, K) -> ((WPB, U, NT) for M <= 16, (WPB, U, NT) for 16 < M <= 32) for the
# llama-3-70b layer shapes: the cold-sweep winners at M = 16 and M = 32
# (kernel_bench.py --which mxfp4sweep; profiles/README.md, "MXFP4 weights")
MXFP4_GEMM_SHAPES: dict = {
    (10240, 8192): ((4, 1, 4), (8, 1, 4)),    # qkv
    (8192, 8192): ((4, 1, 2), (4, 1, 2)),     # o
    (57344, 8192): ((2, 1, 8), (2, 1, 8)),    # gate/up
    (8192, 28672): ((4, 1, 2), (4, 1, 2)),    # down
}
# the largest M at which no shipped instantiation uses scratch memory
# (16 * MXFP4_GEMM_MAX_MT of the header); larger M takes the dequantise path
MXFP4_GEMM_MAX_M = 32


def mxfp4_gemm_config(M: int, N: int, K: int):
    """The (WPB, U, NT) mxfp4_skinny_gemm runs an [M, K] x [N, K]^T call at,
    or None if the kernel does not take the shape."""
    return _quant_gemm_config(M, N, K, 256, MXFP4_GEMM_MAX_M,
                              MXFP4_GEMM_SHAPES, MXFP4_GEMM_SPLIT_K,
                              MXFP4_GEMM_DEFAULT)


def mxfp4_linear_path(x: torch.Tensor, w: Mxfp4Weight):
    """Where linear(x, w) runs for an Mxfp4Weight: ("kernel", (WPB, U, NT))
    for the in-tree W4A16 kernel, ("dequant", None) for mxfp4_dequant into
    the scratch buffer + the library GEMM, ("torch", None) for
    F.linear(x, W_eff) with W_eff formed by torch (CPU, or x not bf16)."""
    if w.q.data_ptr() % 16 or w.scale.data_ptr() % 8:
        return _quant_linear_path(x, w, 32, lambda M, N, K: None)
    return _quant_linear_path(x, w, 32, mxfp4_gemm_config)


def _linear_mxfp4(x: torch.Tensor, w: Mxfp4Weight) -> torch.Tensor:
    return _linear_quant(x, w, *mxfp4_linear_path(x, w), "mxfp4_skinny_gemm",
                         "mxfp4_dequant")


def linear(x: torch.Tensor, w) -> torch.Tensor:
    """x @ w^T. Decode-regime calls (M <= 16) on a shipped (N, K) take the
    in-tree weight-streaming kernel; every other call is F.linear. An
    Fp8Weight goes through fp8_linear_path, an Mxfp4Weight through
    mxfp4_linear_path."""
    if isinstance(w, Fp8Weight):
        return _linear_fp8(x, w)
    if isinstance(w, Mxfp4Weight):
        return _linear_mxfp4(x, w)
    cfg = skinny_gemm_config(x, w)
    if cfg is None:
        return torch.nn.functional.linear(x, w)
    y = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
    hip().skinny_gemm(y, x, w, *cfg)
    return y


# --------------------------------------------------------------------------
# Fused SwiGLU: the in-tree GEMM's GLU epilogue (csrc/skinny_gemm_impl.h)
# computes silu(gate) * up from the accumulators, with the bits of silu_mul on
# the plain kernel's result, and saves the silu_mul launch and the read-back
# of the [M, 2I] intermediate.
# The formats whose dispatch takes it. As with SKINNY_GEMM_SHAPES, a format is
# listed only if its fused kernel beat the two kernels in situ in both of two
# paired traces and end to end, with the parent's outputs (profiles/README.md,
# "SwiGLU in the gate/up GEMM's epilogue").
FUSED_GLU_FORMATS: tuple = ("bf16_coalesced", "fp8", "mxfp4")

_fused_glu_override: "bool | None" = None


def set_fused_glu(on: "bool | None") -> None:
    """In-process override of DYNAMO_FUSED_GLU (None = follow the env)."""
    global _fused_glu_override
    _fused_glu_override = on


def fused_glu_enabled() -> bool:
    if _fused_glu_override is not None:
        return _fused_glu_override
    from dynamo_amd import envs
    return envs.get("DYNAMO_FUSED_GLU", True, bool)


def glu_capable(fmt: str, cfg) -> bool:
    """Whether point (WPB, U, NT, ...) of table `fmt` ("bf16_coalesced" |
    "fp8" | "mxfp4" | "bf16_plain") has a GLU instantiation; a copy of the
    header's skinny::glu_capable, checked against
    hip().skinny_gemm_glu_configs() by the tests. A block pairs NT / 2 gate
    tiles with NT / 2 up tiles, so NT is even; the GLU form of bf16 (8, 1, 4)
    would run 3 waves/SIMD where its plain twin runs 4 and is not built."""
    if fmt == "bf16_plain" or cfg[2] % 2:
        return False
    return not (fmt == "bf16_coalesced" and tuple(cfg[:3]) == (8, 1, 4))


def fused_glu_config(x: torch.Tensor, w):
    """(binding name, configuration) if linear_silu_mul(x, w) runs on the
    fused kernel, else None: linear(x, w) would take the in-tree kernel, its
    configuration has a GLU form, its format is in FUSED_GLU_FORMATS and
    I = N / 2 is a multiple of 16."""
    if not fused_glu_enabled() or w.shape[0] % 32:
        return None
    if isinstance(w, Fp8Weight):
        path, cfg = fp8_linear_path(x, w)
        hit = ("fp8_skinny_gemm", "fp8", cfg) if path == "kernel" else None
    elif isinstance(w, Mxfp4Weight):
        path, cfg = mxfp4_linear_path(x, w)
        hit = (("mxfp4_skinny_gemm", "mxfp4", cfg) if path == "kernel"
               else None)
    else:
        cfg = skinny_gemm_config(x, w)
        hit = None if cfg is None else (
            "skinny_gemm", "bf16_coalesced" if cfg[4] else "bf16_plain", cfg)
    if (hit is None or hit[1] not in FUSED_GLU_FORMATS
            or not glu_capable(hit[1], hit[2])):
        return None
    return hit[0], hit[2]


def linear_silu_mul(x: torch.Tensor, w_gate_up) -> torch.Tensor:
    """silu_mul(linear(x, w_gate_up)) for a gate/up weight [2I, K], gate rows
    first: one kernel where fused_glu_config allows it, else the two calls.
    Equal bits either way."""
    hit = fused_glu_config(x, w_gate_up)
    if hit is None:
        return silu_mul(linear(x, w_gate_up))
    gemm, cfg = hit
    if gemm != "skinny_gemm":
        return _linear_quant(x, w_gate_up, "kernel", cfg, gemm, None, True)
    y = torch.empty(x.shape[0], w_gate_up.shape[0] // 2, dtype=x.dtype,
                    device=x.device)
    hip().skinny_gemm(y, x, w_gate_up, *cfg, True)
    return y


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float,
            allow_fast: bool = True) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty_like(x)
        hip().rmsnorm(out, x.contiguous(), weight, eps, allow_fast)
        return out
    return torch_ref.rmsnorm(x, weight, eps)


def fused_add_rmsnorm(x, residual, weight, eps, allow_fast=True):
    """residual <- x + residual (in place); returns normalized residual."""
    if x.is_cuda:
        hip().fused_add_rmsnorm(x, residual, weight, eps, allow_fast)
        return x
    return torch_ref.fused_add_rmsnorm(x, residual, weight, eps)


def rope_inplace(q, k, positions, cos_sin, num_q_heads, num_k_heads, head_dim):
    if q.is_cuda:
        hip().rope_inplace(q, k, positions, cos_sin, num_q_heads, num_k_heads,
                           head_dim)
        return q, k
    return torch_ref.rope(q, k, positions, cos_sin, num_q_heads, num_k_heads,
                          head_dim)


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    if gate_up.is_cuda:
        d = gate_up.shape[-1] // 2
        out = torch.empty(gate_up.shape[:-1] + (d,), dtype=gate_up.dtype,
                          device=gate_up.device)
        hip().silu_mul(out, gate_up.contiguous())
        return out
    return torch_ref.silu_mul(gate_up)


def gelu(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty_like(x)
        hip().gelu(out, x.contiguous())
        return out
    return torch_ref.gelu(x)


def kv_cache_append(kcache, vcache, k, v, slot_mapping,
                    v_transposed=False):
    if kcache.is_cuda:
        hip().kv_cache_append(kcache, vcache, k.contiguous(), v.contiguous(),
                              slot_mapping, v_transposed)
    else:
        torch_ref.kv_cache_append(kcache, vcache, k, v, slot_mapping,
                                  v_transposed)


def rope_append_qkv(qkv, bias, positions, slot_mapping, cos_sin,
                    kcache, vcache, num_q_heads, num_kv_heads, head_dim,
                    v_transposed=False, allow_fast=True):
    """Fused QKV epilogue: strided qkv read (+bias) -> rope(q,k) ->
    q contiguous out, k/v scattered into the paged cache. One kernel
    instead of {q copy, k copy, rope, kv_append}. Returns q [T, Hq*hd]."""
    T = qkv.shape[0]
    if qkv.is_cuda:
        q_out = torch.empty(T, num_q_heads * head_dim, dtype=qkv.dtype,
                            device=qkv.device)
        hip().rope_append_qkv(q_out, kcache, vcache, qkv, bias, positions,
                              slot_mapping, cos_sin, v_transposed, allow_fast)
        return q_out
    # CPU reference: the unfused sequence
    if bias is not None:
        qkv = qkv + bias
    q, k, v = qkv.split([num_q_heads * head_dim, num_kv_heads * head_dim,
                         num_kv_heads * head_dim], dim=-1)
    q = q.contiguous()
    k = k.contiguous()
    q, k = torch_ref.rope(q, k, positions, cos_sin, num_q_heads,
                          num_kv_heads, head_dim)
    torch_ref.kv_cache_append(kcache, vcache, k.view(T, num_kv_heads, head_dim),
                              v.view(T, num_kv_heads, head_dim), slot_mapping,
                              v_transposed)
    return q


class DecodeScratch:
    """Reusable scratch for two-phase flash-decode (sized once per engine)."""

    def __init__(self, max_batch: int, num_q_heads: int, head_dim: int,
                 max_ctx: int, device):
        self.chunks = int(hip().paged_decode_num_chunks(max_ctx))
        self.chunk_tokens = int(hip().decode_chunk_tokens(max_ctx))
        self.partial = torch.empty(max_batch, num_q_heads, self.chunks, head_dim,
                                   dtype=torch.float32, device=device)
        self.ml = torch.empty(max_batch, num_q_heads, self.chunks, 2,
                              dtype=torch.float32, device=device)

    def view(self, batch: int):
        return self.partial[:batch], self.ml[:batch]


def paged_attention_decode(q, kcache, vcache, page_table, ctx_lens, scale,
                           scratch: "DecodeScratch | None" = None, out=None,
                           v_transposed=False, nt_policy: int = -1):
    """nt_policy: K/V load cache policy of the d-major (VT4) kernel:
    -1 = DYNAMO_DECODE_NT, 0 = default policy, 1 = non-temporal."""
    if q.is_cuda:
        if out is None:
            out = torch.empty_like(q)
        assert scratch is not None, "GPU decode needs a DecodeScratch"
        partial, ml = scratch.view(q.shape[0])
        hip().paged_attention_decode(out, q, kcache, vcache, page_table,
                                     ctx_lens, partial, ml, scale,
                                     scratch.chunk_tokens, v_transposed,
                                     nt_policy)
        return out
    r = torch_ref.paged_attention_decode(q, kcache, vcache, page_table,
                                         ctx_lens, scale,
                                         v_transposed=v_transposed)
    if out is not None:
        out.copy_(r)
        return out
    return r


def prefill_tile_rows(num_q_heads: int, num_kv_heads: int) -> int:
    """Q-tile granularity of the native prefill kernel: the 8-wave 32x32
    kernel handles GQA groups G in {2,4,8} with (8/G)*32-row tiles; the
    4-wave 16x16 kernel takes 64-row tiles. MUST match the dispatch in
    attention_prefill.hip."""
    if num_q_heads % num_kv_heads == 0:
        g = num_q_heads // num_kv_heads
        if g in (2, 4, 8):
            return (8 // g) * 32
    return 64


def build_prefill_tiles(seq_q_lens, device, rows: int = 64):
    """Host-side tile descriptors for the prefill kernel."""
    tile_seq, tile_q0 = [], []
    for s, ql in enumerate(seq_q_lens):
        for q0 in range(0, int(ql), rows):
            tile_seq.append(s)
            tile_q0.append(q0)
    return (torch.tensor(tile_seq, dtype=torch.int32, device=device),
            torch.tensor(tile_q0, dtype=torch.int32, device=device))


def attention_prefill_paged(q, kcache, vcache, page_table, seq_q_start,
                            seq_q_len, seq_ctx_len, scale, tiles=None,
                            v_transposed=False):
    if q.is_cuda:
        out = torch.empty_like(q)
        if tiles is None:
            rows = prefill_tile_rows(q.shape[1], kcache.shape[1])
            tiles = build_prefill_tiles(seq_q_len.tolist(), q.device, rows)
        tile_seq, tile_q0 = tiles
        hip().attention_prefill_paged(out, q, kcache, vcache, page_table,
                                      tile_seq, tile_q0, seq_q_start,
                                      seq_q_len, seq_ctx_len, scale,
                                      v_transposed)
        return out
    return torch_ref.attention_prefill_paged(q, kcache, vcache, page_table,
                                             seq_q_start, seq_q_len,
                                             seq_ctx_len, scale,
                                             v_transposed=v_transposed)


def greedy_sample(logits: torch.Tensor, allow_fast: bool = True) -> torch.Tensor:
    if logits.is_cuda:
        out = torch.empty(logits.shape[0], dtype=torch.int32,
                          device=logits.device)
        hip().greedy_sample(out, logits.float().contiguous(), allow_fast)
        return out
    return torch_ref.greedy_sample(logits)


def _splitmix64(x: torch.Tensor) -> torch.Tensor:
    """splitmix64 finalizer on int64 tensors (wrapping arithmetic; torch
    >> is arithmetic, so logical shifts are emulated with masks). Bit-for-
    bit the same hash as the HIP sampling kernel's hash_u64."""
    def lsr(v, k):
        return (v >> k) & ((1 << (64 - k)) - 1)
    x = x + 0x9e3779b97f4a7c15
    x = (x ^ lsr(x, 30)) * -0x40a7b892e31b1a47   # 0xbf58476d1ce4e5b9
    x = (x ^ lsr(x, 27)) * -0x6b2fb644ecceee15   # 0x94d049bb133111eb
    return x ^ lsr(x, 31)


def gumbel_sample(logits: torch.Tensor, inv_temp: torch.Tensor,
                  seed: int, row_seeds: torch.Tensor = None,
                  allow_fast: bool = True) -> torch.Tensor:
    if logits.is_cuda:
        out = torch.empty(logits.shape[0], dtype=torch.int32,
                          device=logits.device)
        hip().gumbel_sample(out, logits.float().contiguous(), inv_temp, seed,
                            row_seeds, allow_fast)
        return out
    # CPU: DETERMINISTIC counter-based Gumbel noise — the same
    # splitmix64(row_seed ^ v) stream as the HIP kernel (row_seed defaults
    # to seed ^ b<<32), so sampling is reproducible across
    # engines/processes (TP lockstep needs this)
    B, V = logits.shape
    if row_seeds is None:
        rs = (torch.tensor(seed, dtype=torch.int64)
              ^ (torch.arange(B, dtype=torch.int64) << 32))
    else:
        rs = row_seeds.to(torch.int64).cpu()
    v = torch.arange(V, dtype=torch.int64).unsqueeze(0)
    h = _splitmix64(rs.unsqueeze(1) ^ v)
    u = (((h >> 11) & ((1 << 53) - 1)) + 1).double() * (2.0 ** -53)
    g = -torch.log(-torch.log(u.float()))
    return (logits.float() * inv_temp.unsqueeze(-1) + g).argmax(-1).to(torch.int32)


def topkp_sample(logits: torch.Tensor, inv_temp: torch.Tensor,
                 top_k: torch.Tensor, top_p: torch.Tensor,
                 seed: int, row_seeds: torch.Tensor = None) -> torch.Tensor:
    """Fused top-k/top-p Gumbel sampling (GPU only; per-row params)."""
    out = torch.empty(logits.shape[0], dtype=torch.int32,
                      device=logits.device)
    hip().topkp_sample(out, logits.float().contiguous(), inv_temp,
                       top_k, top_p, seed, row_seeds)
    return out


def topk_gating(logits: torch.Tensor, k: int):
    """softmax + renormalized top-k over experts. logits [T, E] fp32."""
    if logits.is_cuda:
        T = logits.shape[0]
        topw = torch.empty(T, k, dtype=torch.float32, device=logits.device)
        topi = torch.empty(T, k, dtype=torch.int32, device=logits.device)
        hip().topk_gating(topw, topi, logits.float().contiguous())
        return topw, topi
    p = torch.softmax(logits.float(), dim=-1)
    # stable descending sort: among equal probabilities the lowest index
    # wins, as in the kernel (torch.topk leaves tie order unspecified)
    topw, topi = torch.sort(p, dim=-1, descending=True, stable=True)
    topw, topi = topw[..., :k], topi[..., :k]
    return topw / topw.sum(-1, keepdim=True), topi.to(torch.int32)


def build_moe_tiles(counts, max_m: int = 16):
    """Host-side tile list [(expert, row0, m)] for the grouped GEMM;
    segments larger than max_m split into multiple tiles."""
    tiles = []
    r0 = 0
    for e, n in enumerate(counts):
        off = 0
        while off < n:
            m = min(max_m, n - off)
            tiles.append((e, r0 + off, m))
            off += m
        r0 += n
    return tiles


def moe_grouped_gemm(x: torch.Tensor, w: torch.Tensor, tiles_t: torch.Tensor):
    """x [T, D] gathered by expert; w [E, N, D]; -> y [T, N]."""
    y = torch.empty(x.shape[0], w.shape[1], dtype=x.dtype, device=x.device)
    hip().moe_grouped_gemm(y, x.contiguous(), w, tiles_t)
    return y


def moe_grouped_gemm_seg(x, w, seg_start, max_tokens):
    """Sync-free grouped GEMM: seg_start [E+1] int32 on DEVICE."""
    y = torch.empty(x.shape[0], w.shape[1], dtype=x.dtype, device=x.device)
    hip().moe_grouped_gemm_seg(y, x.contiguous(), w, seg_start, max_tokens)
    return y


def gather_pages(staging, cache, page_ids):
    if cache.is_cuda:
        hip().gather_pages(staging, cache, page_ids)
    else:
        n = page_ids.shape[0]
        pe = cache[0].numel()
        staging.view(-1)[: n * pe] = cache[page_ids.long()].reshape(-1)


def scatter_pages(staging, cache, page_ids):
    if cache.is_cuda:
        hip().scatter_pages(staging, cache, page_ids)
    else:
        n = page_ids.shape[0]
        pe = cache[0].numel()
        cache[page_ids.long()] = staging.view(-1)[: n * pe].view(n, *cache.shape[1:])


def copy_pages(dst_cache, src_cache, pairs):
    if src_cache.is_cuda:
        hip().copy_pages(dst_cache, src_cache, pairs)
    else:
        src = pairs[:, 0].long()
        dst = pairs[:, 1].long()
        dst_cache[dst] = src_cache[src]


# --------------------------------------------------------------------------
# Batched LoRA (csrc/lora.hip): row i of the batch takes the adapter in bank
# slot slots[i] (device int32, -1 = none). A bank is the tuple
# (A_bank [S, R, K], B_bank [S, N, R], ranks [S] int32, scales [S] fp32) of
# one (layer, target); dynamo_amd.lora.LoRABank owns them.
def lora_shrink(t, x, A_bank, slots, ranks):
    """t[i, r] = x[i] . A_bank[slots[i], r] for r < ranks[slots[i]], fp32."""
    if x.is_cuda:
        hip().lora_shrink(t, x, A_bank, slots, ranks)
        return t
    return torch_ref.lora_shrink(t, x, A_bank, slots, ranks)


def lora_expand_add(y, t, B_bank, slots, ranks, scales):
    """In place: y[i] += scales[s] * B_bank[s, :, :rank] @ t[i, :rank], one
    rounding; rows with slots[i] < 0 stay bit-untouched."""
    if y.is_cuda:
        hip().lora_expand_add(y, t, B_bank, slots, ranks, scales)
        return y
    return torch_ref.lora_expand_add(y, t, B_bank, slots, ranks, scales)


def lora_delta_(y, x, bank, slots):
    """y += the per-row LoRA delta of x under `bank` (see above), in place."""
    A_bank, B_bank, ranks, scales = bank
    # rows and columns the kernels skip are neither written nor read
    t = torch.empty(x.shape[0], A_bank.shape[1], dtype=torch.float32,
                    device=x.device)
    lora_shrink(t, x, A_bank, slots, ranks)
    lora_expand_add(y, t, B_bank, slots, ranks, scales)
    return y


# --------------------------------------------------------------------------
# Per-request logit processors (csrc/logits_process.hip; the semantics are
# written out at torch_ref.apply_logit_processors). engine/penalties.py owns
# the bank and builds the per-step tensors.
def penalty_fold(counts, slots, tokens, is_prompt):
    """Add entries (slots[i], tokens[i], is_prompt[i]), int32 each, to the
    [slots, V] int32 bank `counts` (word = prompt bit | output count << 1)."""
    if counts.is_cuda:
        hip().penalty_fold(counts, slots, tokens, is_prompt)
        return counts
    return torch_ref.penalty_fold(counts, slots, tokens, is_prompt)


def apply_logit_processors(logits, counts, slots, params, bias=None,
                           allow_fast: bool = True):
    """Penalties, logit_bias and min_p in place on contiguous fp32 logits
    [B, V]: bank `counts` (or None if no row has a slot), slots [B] int32
    (-1 = none), params [B, 5] fp32 = (repetition, presence, frequency, min_p,
    temperature), bias = (offsets [B + 1] int32, ids int32, vals fp32) or
    None. Rows with neutral parameters stay bit-untouched."""
    if logits.is_cuda:
        hip().logits_process(logits, counts, slots, params,
                             *(bias or (None, None, None)), allow_fast)
        return logits
    return torch_ref.apply_logit_processors(logits, counts, slots, params,
                                            bias)
