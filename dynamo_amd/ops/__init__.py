"""Op dispatch: native HIP kernels on GPU, torch reference on CPU.

On a GPU box the HIP extension is REQUIRED — a missing/failed extension
raises instead of silently falling back to eager PyTorch, so GPU tests can
never pass on a non-native path.
"""
from __future__ import annotations

import torch

from . import fp8_weights, mxfp4_weights, mxfp8, torch_ref
from .fp8_weights import (Fp8ExpertWeight, Fp8Weight,  # re-export
                          quantize_fp8_rowwise, quantize_model_fp8)
from .mxfp4_weights import (Mxfp4ExpertWeight, Mxfp4Weight,  # re-export
                            quantize_mxfp4, quantize_model_mxfp4)
from .mxfp8 import (dequantize_mxfp8_rows,  # re-export
                    quantize_mxfp8_rows)
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


def _quant_linear_path(x, w, dequant_k, gemm_config, fmt=None):
    """("kernel", cfg) | ("tile", point) | ("mx", point) | ("dequant", None) |
    ("torch", None) for linear(x, w) with a quantised weight holder w whose
    dequantise kernel needs K % dequant_k == 0. fmt names the format's mx and
    tiled kernels, asked first (mx, then tiled) where they are switched on
    (the tiled kernel's MIN_M may lie below the skinny kernel's largest M);
    None: the weight can take none of the kernels."""
    N, K = w.shape
    if not x.is_cuda:
        return "torch", None
    if x.dtype != torch.bfloat16 or K % dequant_k or x.shape[-1] != K:
        return "torch", None
    if x.dim() == 2 and x.is_contiguous() and x.data_ptr() % 16 == 0:
        if (fmt is not None and mx_gemm_enabled()
                and w.q.data_ptr() % 16 == 0 and w.scale.data_ptr() % 4 == 0):
            point = mx_gemm_config(fmt, x.shape[0], N, K)
            if point is not None:
                return "mx", point
        if fmt is not None and tile_gemm_enabled():
            point = tile_gemm_config(fmt, x.shape[0], N, K)
            if point is not None:
                return "tile", point
        cfg = gemm_config(x.shape[0], N, K)
        if cfg is not None:
            return "kernel", cfg
    return "dequant", None


def _linear_quant(x, w, path, cfg, gemm: str, dequant: str, glu=False):
    """linear(x, w) on `path`; gemm and dequant name the format's bindings
    (the tiled and mx kernels' are the skinny one's with "tile" / "mx" for
    "skinny"). glu (kernel, tile and mx paths only): the fused SwiGLU form,
    y = [M, N / 2]."""
    if path in ("kernel", "tile", "mx"):
        y = torch.empty(x.shape[0], w.shape[0] // 2 if glu else w.shape[0],
                        dtype=x.dtype, device=x.device)
        if path == "mx":
            # x to MXFP8 rows in the device's scratch pair, then the GEMM
            xq, xs = mxfp8.scratch_views(x.device, *x.shape)
            hip().mxfp8_quantize_rows(xq, xs, x)
            getattr(hip(), gemm.replace("_skinny_", "_mx_"))(
                y, xq, xs, w.q, w.scale, *cfg, glu)
        elif path == "tile":
            getattr(hip(), gemm.replace("_skinny_", "_tile_"))(
                y, x, w.q, w.scale, *cfg, glu)
        else:
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
    serve). With the tiled kernel switched on (set_tile_gemm) also
    ("tile", (BM, WN, WK, NT, U)) for fp8_tile_gemm, with the mx kernel
    switched on (set_mx_gemm) ("mx", (BM, BN, WM, WN)) for x quantised to
    MXFP8 rows + fp8_mx_gemm."""
    return _quant_linear_path(x, w, 16, fp8_gemm_config, "fp8")


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
    F.linear(x, W_eff) with W_eff formed by torch (CPU, or x not bf16). With
    the tiled kernel switched on (set_tile_gemm) also
    ("tile", (BM, WN, WK, NT, U)) for mxfp4_tile_gemm, with the mx kernel
    switched on (set_mx_gemm) ("mx", (BM, BN, WM, WN)) for x quantised to
    MXFP8 rows + mxfp4_mx_gemm."""
    if w.q.data_ptr() % 16 or w.scale.data_ptr() % 8:
        return _quant_linear_path(x, w, 32, lambda M, N, K: None)
    return _quant_linear_path(x, w, 32, mxfp4_gemm_config, "mxfp4")


def _linear_mxfp4(x: torch.Tensor, w: Mxfp4Weight) -> torch.Tensor:
    return _linear_quant(x, w, *mxfp4_linear_path(x, w), "mxfp4_skinny_gemm",
                         "mxfp4_dequant")


# --------------------------------------------------------------------------
# Tiled W8A16 / W4A16 GEMM (csrc/quant_tile_gemm.hip): the same formats above
# the skinny kernel's M, with x staged once per block in LDS. Opt-in
# (DYNAMO_QUANT_TILE_GEMM=1 / set_tile_gemm): off, every call runs where it
# ran before. (BM, WN, WK, NT, U) points the bindings can launch; they need
# K % (WK * KSTEP * U) == 0. Copies of the kernel file's tables that tests can
# read without the extension; they check them against
# hip().tile_gemm_configs(). The first point of a format accepts every
# K % KSTEP == 0. Every point has a GLU form (even NT).
FP8_TILE_GEMM_CONFIGS: tuple = (
    (64, 4, 1, 2, 1), (128, 4, 1, 2, 2), (64, 4, 2, 2, 2),
    (128, 4, 2, 2, 1), (128, 8, 1, 2, 2), (64, 2, 2, 2, 2), (64, 2, 4, 2, 1),
)
MXFP4_TILE_GEMM_CONFIGS: tuple = (
    (64, 4, 1, 2, 1), (128, 4, 1, 2, 1), (64, 4, 2, 2, 1),
    (128, 8, 1, 2, 1), (64, 8, 1, 2, 2), (64, 2, 2, 2, 1), (64, 1, 2, 2, 1),
)
TILE_GEMM_CONFIGS: dict = {"fp8": FP8_TILE_GEMM_CONFIGS,
                           "mxfp4": MXFP4_TILE_GEMM_CONFIGS}
TILE_GEMM_KSTEP: dict = {"fp8": 128, "mxfp4": 256}
# (N, K) -> ((largest M, point), ...) with M ascending, for the llama-3-70b
# layer shapes: the cold-sweep winners (kernel_bench.py --which tile_sweep;
# profiles/README.md, "Tiled quantised GEMM"). A shape outside the table, or a
# K its point does not divide, takes the format's first point.
FP8_TILE_GEMM_SHAPES: dict = {
    (10240, 8192): ((128, (64, 4, 2, 2, 2)), (256, (128, 4, 2, 2, 1))),  # qkv
    (8192, 8192): ((128, (64, 2, 4, 2, 1)), (256, (64, 4, 2, 2, 2))),    # o
    (57344, 8192): ((256, (128, 8, 1, 2, 2)),),                     # gate/up
    (8192, 28672): ((128, (64, 2, 4, 2, 1)), (256, (64, 4, 2, 2, 2))),   # down
}
MXFP4_TILE_GEMM_SHAPES: dict = {
    (10240, 8192): ((64, (64, 2, 2, 2, 1)), (128, (64, 4, 2, 2, 1)),
                    (256, (64, 8, 1, 2, 2))),                            # qkv
    (8192, 8192): ((128, (64, 2, 2, 2, 1)), (256, (64, 4, 2, 2, 1))),    # o
    (57344, 8192): ((64, (64, 8, 1, 2, 2)), (256, (128, 8, 1, 2, 1))),
    (8192, 28672): ((128, (64, 2, 2, 2, 1)), (256, (64, 4, 2, 2, 1))),   # down
}
TILE_GEMM_SHAPES: dict = {"fp8": FP8_TILE_GEMM_SHAPES,
                          "mxfp4": MXFP4_TILE_GEMM_SHAPES}
# The M the tiled kernel takes. MIN_M: the skinny kernel's largest M + 1, so
# that no M from 1 to MAX_M dequantises; not lower, because at the skinny
# kernel's own M the tiled one was ahead on some shapes only (fp8 qkv and
# gate/up at M = 48 and 64) and behind on the others. MAX_M: at M = 256 it was
# ahead of dequantise + library on all four shapes in both sweeps (1.16-2.0x
# fp8, 1.4-2.5x mxfp4); at M = 512, the next M measured, it was behind on qkv
# (0.82x fp8, 1.00x mxfp4).
TILE_GEMM_MIN_M: dict = {"fp8": FP8_GEMM_MAX_M + 1,
                         "mxfp4": MXFP4_GEMM_MAX_M + 1}
TILE_GEMM_MAX_M: dict = {"fp8": 256, "mxfp4": 256}

_tile_gemm_override: "bool | None" = None


def set_tile_gemm(on: "bool | None") -> None:
    """In-process override of DYNAMO_QUANT_TILE_GEMM (None = follow the
    env)."""
    global _tile_gemm_override
    _tile_gemm_override = on


def tile_gemm_enabled() -> bool:
    if _tile_gemm_override is not None:
        return _tile_gemm_override
    from dynamo_amd import envs
    return envs.get("DYNAMO_QUANT_TILE_GEMM", False, bool)


def tile_gemm_config(fmt: str, M: int, N: int, K: int):
    """The (BM, WN, WK, NT, U) the tiled kernel of fmt ("fp8" | "mxfp4") runs
    an [M, K] x [N, K]^T call at, or None if it does not take the call: M
    outside [TILE_GEMM_MIN_M, TILE_GEMM_MAX_M] or a shape the kernel cannot
    do. The switch is the caller's business."""
    kstep = TILE_GEMM_KSTEP[fmt]
    if not (TILE_GEMM_MIN_M[fmt] <= M <= TILE_GEMM_MAX_M[fmt]
            and K >= kstep and K % kstep == 0 and N >= 16 and N % 16 == 0):
        return None
    point = TILE_GEMM_CONFIGS[fmt][0]
    for max_m, p in TILE_GEMM_SHAPES[fmt].get((N, K), ()):
        if M <= max_m and K % (p[2] * kstep * p[4]) == 0:
            point = p
            break
    return point


# --------------------------------------------------------------------------
# W8A8 / W4A8 prefill GEMM (csrc/mx_gemm.hip): above the tiled kernel's M the
# activations are quantised to MXFP8 rows (ops/mxfp8.py) and the product runs
# on the block-scaled fp8 x fp8 / fp8 x fp4 MFMA instead of dequantising the
# weight for the bf16 library GEMM. A numerical change (x loses precision),
# so opt-in (DYNAMO_MX_GEMM=1 / set_mx_gemm): off, every call runs where it
# ran before. (BM, BN, WM, WN) points the bindings can launch, a copy of the
# kernel file's table that tests can read without the extension; they check
# it against hip().mx_gemm_configs(). Every point accepts every K % 128 == 0
# and has a GLU form.
MX_GEMM_POINTS: tuple = (
    (128, 128, 2, 2), (256, 128, 2, 2), (256, 128, 4, 2), (128, 256, 2, 2),
)
MX_GEMM_CONFIGS: dict = {"fp8": MX_GEMM_POINTS, "mxfp4": MX_GEMM_POINTS}
MX_GEMM_KSTEP = 128
# (N, K) -> ((largest M, point), ...) with M ascending, for the llama-3-70b
# layer shapes (kernel_bench.py --which mx_gemm_sweep; profiles/README.md,
# "MX GEMM"): an M range is listed only where quantise + mx GEMM beat
# dequantise + library GEMM in both of two sweeps by more than the runs
# differ, and a listed shape above its last M stays on the dequantise path.
# qkv and o won at no measured M above 256 and are listed empty.
FP8_MX_GEMM_SHAPES: dict = {
    (10240, 8192): (),                                              # qkv
    (8192, 8192): (),                                               # o
    (57344, 8192): ((512, (256, 128, 4, 2)), (1024, (128, 128, 2, 2))),
    (8192, 28672): ((512, (128, 128, 2, 2)), (1024, (128, 256, 2, 2))),
}
MXFP4_MX_GEMM_SHAPES: dict = {
    (10240, 8192): (),                                              # qkv
    (8192, 8192): (),                                               # o
    (57344, 8192): ((512, (128, 128, 2, 2)),),                      # gate/up
    (8192, 28672): ((512, (128, 128, 2, 2)),),                      # down
}
MX_GEMM_SHAPES: dict = {"fp8": FP8_MX_GEMM_SHAPES,
                        "mxfp4": MXFP4_MX_GEMM_SHAPES}
# The M a shape outside the table takes the mx path at, on the first point.
# MIN_M: the tiled kernel's largest M + 1. MAX_M: the largest measured M at
# which the mx path was ahead on gate/up and down; above it the kernel (0.9 -
# 1.15 PFLOP/s) is behind the library GEMM on every measured shape.
MX_GEMM_MIN_M: dict = {"fp8": 257, "mxfp4": 257}
MX_GEMM_MAX_M: dict = {"fp8": 1024, "mxfp4": 512}

_mx_gemm_override: "bool | None" = None


def set_mx_gemm(on: "bool | None") -> None:
    """In-process override of DYNAMO_MX_GEMM (None = follow the env)."""
    global _mx_gemm_override
    _mx_gemm_override = on


def mx_gemm_enabled() -> bool:
    if _mx_gemm_override is not None:
        return _mx_gemm_override
    from dynamo_amd import envs
    return envs.get("DYNAMO_MX_GEMM", False, bool)


def mx_gemm_config(fmt: str, M: int, N: int, K: int):
    """The (BM, BN, WM, WN) the mx kernel of fmt ("fp8" | "mxfp4") runs an
    [M, K] x [N, K]^T call at, or None if it does not take the call: M below
    MX_GEMM_MIN_M, above the shape's last table entry (MX_GEMM_MAX_M for a
    shape outside the table) or a shape the kernel cannot do. The switch is
    the caller's business."""
    if not (M >= MX_GEMM_MIN_M[fmt] and K >= MX_GEMM_KSTEP
            and K % MX_GEMM_KSTEP == 0 and N >= 16 and N % 16 == 0):
        return None
    entries = MX_GEMM_SHAPES[fmt].get((N, K))
    if entries is None:
        return (MX_GEMM_CONFIGS[fmt][0] if M <= MX_GEMM_MAX_M[fmt] else None)
    for max_m, p in entries:
        if M <= max_m:
            return p
    return None


def reserve_mx_scratch(model, tokens: int) -> None:
    """Size the MXFP8 scratch pair of the model's device for a step of
    `tokens` tokens: tokens x the largest K of its quantised dense
    projections. The model runner calls this before any graph capture when
    the mx path is switched on."""
    for layer in model.layers:
        for sub, name in fp8_weights.PROJECTIONS:
            w = getattr(getattr(layer, sub, None), name, None)
            if isinstance(w, (Fp8Weight, Mxfp4Weight)):
                mxfp8.reserve_scratch(w.device, tokens * w.shape[1])


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
    if isinstance(w, (Fp8Weight, Mxfp4Weight)):
        fmt = "fp8" if isinstance(w, Fp8Weight) else "mxfp4"
        path, cfg = (fp8_linear_path if fmt == "fp8"
                     else mxfp4_linear_path)(x, w)
        if path == "tile":   # every point of the tiled kernel has a GLU form
            return ((f"{fmt}_tile_gemm", cfg) if fmt in FUSED_GLU_FORMATS
                    and cfg[3] % 2 == 0 else None)
        if path == "mx":     # every point of the mx kernel has one too
            return ((f"{fmt}_mx_gemm", cfg) if fmt in FUSED_GLU_FORMATS
                    else None)
        hit = (f"{fmt}_skinny_gemm", fmt, cfg) if path == "kernel" else None
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
        path = ("tile" if gemm.endswith("_tile_gemm") else
                "mx" if gemm.endswith("_mx_gemm") else "kernel")
        return _linear_quant(x, w_gate_up, path, cfg,
                             gemm.replace("_mx_", "_skinny_"), None, True)
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


# --------------------------------------------------------------------------
# Rope + KV append inside decode attention (paged_decode_mfma_swapped_dmajor_
# rope, csrc/attention_decode_impl.h): a decode step's rope_append_qkv launch
# folded into phase 1 of the d-major decode kernel, equal bits in the output
# and in both caches. DYNAMO_FUSED_ROPE_ATTN / set_fused_rope_attn switch it;
# off, and wherever fused_rope_attn_ready says no, the two kernels run.
FUSED_ROPE_ATTN_DEFAULT = True

_fused_rope_attn_override: "bool | None" = None


def set_fused_rope_attn(on: "bool | None") -> None:
    """In-process override of DYNAMO_FUSED_ROPE_ATTN (None = follow the
    env). A captured decode graph keeps the route it was captured with."""
    global _fused_rope_attn_override
    _fused_rope_attn_override = on


def fused_rope_attn_enabled() -> bool:
    if _fused_rope_attn_override is not None:
        return _fused_rope_attn_override
    from dynamo_amd import envs
    return envs.get("DYNAMO_FUSED_ROPE_ATTN", FUSED_ROPE_ATTN_DEFAULT, bool)


def fused_rope_attn_ready(Hq: int, Hkv: int, head_dim: int, page_size: int,
                          v_transposed: bool, kv_dtype, *, decode_step: bool,
                          num_tokens: int, num_decode: int,
                          shared_prefix: bool = False,
                          on_gpu: bool = True) -> bool:
    """Does this attention call take the fused kernel? Only a pure decode
    step of the engine's persistent-buffer path (decode_step: one row per
    sequence, slot_mapping[b] the slot of token ctx_lens[b] - 1, padded rows
    at slot -1) over bf16 d-major V pages with a GQA group the d-major kernel
    serves. fp8 KV, token-major V, prefill and mixed steps, multi-query,
    shared-prefix and the CPU path keep rope_append_qkv + the attention
    kernels."""
    if not (on_gpu and decode_step and fused_rope_attn_enabled()):
        return False
    if shared_prefix or num_decode <= 0 or num_tokens != num_decode:
        return False
    if Hkv <= 0 or Hq % Hkv:
        return False
    return (v_transposed and kv_dtype == torch.bfloat16
            and 2 <= Hq // Hkv <= 16 and head_dim == 128
            and page_size % 32 == 0 and page_size & (page_size - 1) == 0)


def paged_attention_decode_rope(qkv, bias, positions, slot_mapping, cos_sin,
                                kcache, vcache, page_table, ctx_lens, scale,
                                scratch: "DecodeScratch | None",
                                num_q_heads: int, num_kv_heads: int,
                                head_dim: int, out=None, nt_policy: int = -1):
    """rope_append_qkv(v_transposed=True) followed by
    paged_attention_decode(v_transposed=True) for one decode step, qkv
    [B, (Hq + 2 Hkv) * hd] -> [B, Hq, hd]; the new token's k and v land in
    the caches. On the GPU one phase-1 kernel does both (bf16 d-major V
    pages); slot_mapping[b] must be the slot of token ctx_lens[b] - 1 under
    page_table[b], or negative for a row that appends nothing."""
    B = qkv.shape[0]
    if qkv.is_cuda:
        if out is None:
            out = torch.empty(B, num_q_heads, head_dim, dtype=qkv.dtype,
                              device=qkv.device)
        assert scratch is not None, "GPU decode needs a DecodeScratch"
        partial, ml = scratch.view(B)
        hip().paged_attention_decode_rope(
            out, qkv, bias, positions, slot_mapping, cos_sin, kcache, vcache,
            page_table, ctx_lens, partial, ml, scale, scratch.chunk_tokens,
            nt_policy)
        return out
    q = rope_append_qkv(qkv, bias, positions, slot_mapping, cos_sin, kcache,
                        vcache, num_q_heads, num_kv_heads, head_dim,
                        v_transposed=True)
    return paged_attention_decode(q.view(B, num_q_heads, head_dim), kcache,
                                  vcache, page_table, ctx_lens, scale,
                                  scratch, out=out, v_transposed=True)


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


# --------------------------------------------------------------------------
# Split-KV multi-query attention (csrc/attention_multiquery.hip): short query
# runs (a prefix-cache hit's remainder, a chunked prefill's tail, a
# speculative verification step) on long contexts, streamed like decode with
# the run folded onto the MFMA columns beside the GQA group. Opt-in
# (DYNAMO_MQ_ATTN=1 / set_multiquery_attn): off, such steps take the prefill
# kernel as before.
MQ_MAX_Q = 8        # query tokens per sequence
MQ_MAX_COLS = 64    # q_len * G: four 16-column MFMA tiles

_multiquery_override: "bool | None" = None


def set_multiquery_attn(on: "bool | None") -> None:
    """In-process override of DYNAMO_MQ_ATTN (None = follow the env)."""
    global _multiquery_override
    _multiquery_override = on


def multiquery_attn_enabled() -> bool:
    if _multiquery_override is not None:
        return _multiquery_override
    from dynamo_amd import envs
    return envs.get("DYNAMO_MQ_ATTN", False, bool)


def multiquery_ready(q_lens, Hq: int, Hkv: int, head_dim: int, page_size: int,
                     v_transposed: bool, kv_dtype) -> bool:
    """Can the multi-query kernel take a step whose sequences bring q_lens
    (host ints) new tokens? Host values only: no device sync."""
    if not q_lens or Hkv <= 0 or Hq % Hkv:
        return False
    G = Hq // Hkv
    longest = max(q_lens)
    return (v_transposed and 2 <= G <= 16 and head_dim == 128
            and page_size % 32 == 0 and page_size & (page_size - 1) == 0
            and kv_dtype in (torch.bfloat16, torch.float8_e4m3fn)
            and min(q_lens) >= 0 and 1 <= longest <= MQ_MAX_Q
            and longest * G <= MQ_MAX_COLS)


class MultiQueryScratch:
    """Chunk partials of the multi-query kernel, one row per query token
    (DecodeScratch's chunk rule)."""

    def __init__(self, max_rows: int, num_q_heads: int, head_dim: int,
                 max_ctx: int, device):
        self.chunks = int(hip().paged_decode_num_chunks(max_ctx))
        self.chunk_tokens = int(hip().decode_chunk_tokens(max_ctx))
        self.max_rows = max_rows
        self.partial = torch.empty(max_rows, num_q_heads, self.chunks,
                                   head_dim, dtype=torch.float32,
                                   device=device)
        self.ml = torch.empty(max_rows, num_q_heads, self.chunks, 2,
                              dtype=torch.float32, device=device)


def multiquery_row_ctx(seq_q_start, seq_q_len, seq_ctx_len, Tq: int):
    """[Tq] int32: the tokens each flattened q row sees, ctx - q_len + j + 1
    for row j of its run. Stays on the tensors' device, no host sync."""
    base = (seq_ctx_len - seq_q_len - seq_q_start).to(torch.int32)
    rows = torch.arange(1, Tq + 1, dtype=torch.int32, device=base.device)
    return torch.repeat_interleave(base, seq_q_len.long(),
                                   output_size=Tq) + rows


def paged_attention_multiquery(q, kcache, vcache, page_table, seq_q_start,
                               seq_q_len, seq_ctx_len, scale,
                               scratch: "MultiQueryScratch | None" = None,
                               max_q_len: int = MQ_MAX_Q, v_transposed=True):
    """Causal paged attention of short query runs, q [Tq, Hq, hd] ->
    [Tq, Hq, hd], with attention_prefill_paged's semantics: row j of a run
    sits at position ctx - q_len + j. max_q_len is the host's bound on
    seq_q_len (it picks the kernel's column tiles)."""
    if q.is_cuda:
        assert v_transposed, "the multi-query kernel reads d-major V pages"
        assert scratch is not None, "GPU multi-query needs a MultiQueryScratch"
        Tq = q.shape[0]
        assert Tq <= scratch.max_rows, (Tq, scratch.max_rows)
        out = torch.empty_like(q)
        row_ctx = multiquery_row_ctx(seq_q_start, seq_q_len, seq_ctx_len, Tq)
        hip().paged_attention_multiquery(
            out, q, kcache, vcache, page_table, seq_q_start, seq_q_len,
            seq_ctx_len, row_ctx, scratch.partial, scratch.ml, scale,
            scratch.chunk_tokens, max_q_len)
        return out
    return torch_ref.attention_prefill_paged(q, kcache, vcache, page_table,
                                             seq_q_start, seq_q_len,
                                             seq_ctx_len, scale,
                                             v_transposed=v_transposed)


# --------------------------------------------------------------------------
# Shared-prefix decode attention (csrc/attention_shared_prefix.hip): decode
# rows whose page tables begin with the same physical pages (the prefix cache
# hands a common prompt's pages to every request that hits it) stream those
# pages once, the rows folded onto the MFMA columns beside the GQA group.
# Opt-in (DYNAMO_SHARED_PREFIX_ATTN=1 / set_shared_prefix_attn): off, and in
# any step without such a group, decode runs the per-row kernel as before.
SP_MAX_COLS = 64    # members * G: four 16-column MFMA tiles

_shared_prefix_override: "bool | None" = None


def set_shared_prefix_attn(on: "bool | None") -> None:
    """In-process override of DYNAMO_SHARED_PREFIX_ATTN (None = follow the
    env)."""
    global _shared_prefix_override
    _shared_prefix_override = on


def shared_prefix_attn_enabled() -> bool:
    if _shared_prefix_override is not None:
        return _shared_prefix_override
    from dynamo_amd import envs
    return envs.get("DYNAMO_SHARED_PREFIX_ATTN", False, bool)


def shared_prefix_ready(Hq: int, Hkv: int, head_dim: int, page_size: int,
                        v_transposed: bool, kv_dtype) -> bool:
    """Can the shared-prefix kernel serve this engine's decode steps?"""
    if Hkv <= 0 or Hq % Hkv:
        return False
    return (v_transposed and 2 <= Hq // Hkv <= 16 and head_dim == 128
            and page_size % 32 == 0 and page_size & (page_size - 1) == 0
            and kv_dtype in (torch.bfloat16, torch.float8_e4m3fn))


def shared_prefix_plan(page_lists, ctx_lens, chunk_tokens: int,
                       page_size: int, G: int, capacity: int):
    """Work items of the shared-prefix kernel for one decode batch, from host
    values only (page id lists and context lengths per row): (item_rows
    [capacity, R] int32, item_range [capacity, 2] int32, max_members) as host
    tensors, R = SP_MAX_COLS // G, or None when no two rows share a chunk.

    Rows are bucketed by their first chunk's page ids. A bucket's prefix_len
    is the common leading page run of all its rows in tokens, capped at
    min(ctx) - 1 (the token being decoded stays in every row's own tail) and
    rounded down to a multiple of chunk_tokens; sharing below the first level
    (a tree of prefixes) is not looked for. A group is one prefix item per R
    members over [0, prefix_len) plus one item per member over
    [prefix_len, ctx); every other row is one item over [0, ctx). So every
    (row, chunk) below ctx is written by exactly one item, and the plan stays
    valid while contexts only grow and new pages only join the tails."""
    R = SP_MAX_COLS // G
    ppc = chunk_tokens // page_size if chunk_tokens % page_size == 0 else 0
    buckets = {}
    for b, (pages, ctx) in enumerate(zip(page_lists, ctx_lens)):
        if ppc and ctx > chunk_tokens and len(pages) >= ppc:
            buckets.setdefault(tuple(pages[:ppc]), []).append(b)
    items = []                              # (rows, t_begin, t_end)
    grouped = set()
    for rows in buckets.values():
        if len(rows) < 2:
            continue
        run = 0
        for col in zip(*(page_lists[b] for b in rows)):
            if any(p != col[0] for p in col):
                break
            run += 1
        prefix = min(run * page_size, min(ctx_lens[b] for b in rows) - 1)
        prefix -= prefix % chunk_tokens
        if prefix <= 0:
            continue
        grouped.update(rows)
        for i in range(0, len(rows), R):
            items.append((rows[i:i + R], 0, prefix))
        items.extend(([b], prefix, -1) for b in rows)
    if not grouped:
        return None
    items.extend(([b], 0, -1) for b in range(len(page_lists))
                 if b not in grouped)
    if len(items) > capacity:
        raise ValueError(f"{len(items)} shared-prefix work items exceed the "
                         f"capacity {capacity}")
    item_rows = torch.full((capacity, R), -1, dtype=torch.int32)
    item_range = torch.zeros(capacity, 2, dtype=torch.int32)
    for w, (rows, t0, t1) in enumerate(items):
        item_rows[w, :len(rows)] = torch.tensor(rows, dtype=torch.int32)
        item_range[w, 0], item_range[w, 1] = t0, t1
    return item_rows, item_range, max(len(it[0]) for it in items)


def paged_attention_decode_shared(q, kcache, vcache, page_table, ctx_lens,
                                  plan, scale,
                                  scratch: "DecodeScratch | None" = None,
                                  out=None):
    """paged_attention_decode over d-major V pages with the work split of
    `plan` = (item_rows, item_range, max_members) from shared_prefix_plan,
    built with the scratch's chunk_tokens, on q's device. The plan changes
    which block reads what, not the result."""
    if q.is_cuda:
        if out is None:
            out = torch.empty_like(q)
        assert scratch is not None, "GPU decode needs a DecodeScratch"
        partial, ml = scratch.view(q.shape[0])
        item_rows, item_range, max_members = plan
        hip().paged_attention_decode_shared(
            out, q, kcache, vcache, page_table, ctx_lens, item_rows,
            item_range, partial, ml, scale, scratch.chunk_tokens, max_members)
        return out
    r = torch_ref.paged_attention_decode(q, kcache, vcache, page_table,
                                         ctx_lens, scale, v_transposed=True)
    if out is not None:
        out.copy_(r)
        return out
    return r


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


# --------------------------------------------------------------------------
# Fused top-N logprobs (csrc/logprobs.hip; the semantics are written out at
# torch_ref.top_logprobs). Opt-in: values differ from torch.log_softmax by
# fp32 rounding and ties are ordered (lowest id first) where torch.topk
# leaves them unspecified.
LOGPROBS_MAX_N = 20           # the OpenAI top_logprobs ceiling
_LOGPROBS_MAX_SLICES = 64     # kMaxSlices of the kernel

_logprobs_kernel_override: "bool | None" = None


def set_logprobs_kernel(on: "bool | None") -> None:
    """In-process override of DYNAMO_LOGPROBS_KERNEL (None = follow the
    env)."""
    global _logprobs_kernel_override
    _logprobs_kernel_override = on


def logprobs_kernel_enabled() -> bool:
    if _logprobs_kernel_override is not None:
        return _logprobs_kernel_override
    from dynamo_amd import envs
    return envs.get("DYNAMO_LOGPROBS_KERNEL", False, bool)


def _logprobs_slices(B: int, V: int) -> int:
    """Slices per row of the kernel's first phase: two blocks per CU over the
    batch, no slice under 2048 tokens (one block-wide step of 16-byte loads).
    profiles/README.md, "Fused logprobs"."""
    return max(1, min(_LOGPROBS_MAX_SLICES, -(-512 // max(B, 1)), V // 2048))


def top_logprobs(logits: torch.Tensor, sampled: torch.Tensor,
                 want: torch.Tensor, nmax: int, out=None, slices=None):
    """(token_lp [B] fp32, top_lp [B, nmax] fp32, top_ids [B, nmax] int32) of
    contiguous fp32 logits [B, V]: the logprob of sampled[b] and the top
    min(want[b], V) entries of row b, larger logit first and lower id first
    among equal logits. want[b] == 0 skips the row; slots past want[b] keep
    what `out` (the three tensors, else fresh uninitialised ones) held.
    sampled and want are int32 [B]; 1 <= nmax <= LOGPROBS_MAX_N. `slices`
    overrides the kernel's slices per row (benchmarks)."""
    if not 1 <= nmax <= LOGPROBS_MAX_N:
        raise ValueError(f"nmax {nmax} outside [1, {LOGPROBS_MAX_N}]")
    if not logits.is_cuda:
        return torch_ref.top_logprobs(logits, sampled, want, nmax, out)
    B, V = logits.shape
    if out is None:
        out = (torch.empty(B, dtype=torch.float32, device=logits.device),
               torch.empty(B, nmax, dtype=torch.float32, device=logits.device),
               torch.empty(B, nmax, dtype=torch.int32, device=logits.device))
    S = slices or _logprobs_slices(B, V)
    stats = torch.empty(B, S, 2, dtype=torch.float32, device=logits.device)
    cand = torch.empty(B, S, nmax, dtype=torch.int64, device=logits.device)
    hip().top_logprobs(*out, logits, sampled, want, stats, cand, nmax, S)
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


# --------------------------------------------------------------------------
# Routed MoE decode (csrc/moe_decode.hip): T <= 64 tokens, top-k <= 8 of
# E <= 64 experts, bf16, fp8 or mxfp4 expert weights. Route, expert-grouped
# gate/up GEMM with SwiGLU in its epilogue, expert-grouped down GEMM weighted
# by the gate weights, per-token combine: four launches, and only live
# experts' weights are read. For bf16 experts opt-in through
# DYNAMO_MOE_FUSED=1 (models/mixtral.py); quantised experts always take it.
MOE_DECODE_MAX_T, MOE_DECODE_MAX_TOPK, MOE_DECODE_MAX_E = 64, 8, 64
# (WPB, U, NT) points of moe_routed_gemm; it needs K % (WPB * 64 * U) == 0.
# A copy of the kernel file's MOE_DECODE_CONFIGS that tests can read without
# the extension; they check it against hip().moe_decode_configs().
MOE_DECODE_CONFIGS: tuple = (
    (1, 1, 2), (1, 2, 2), (1, 2, 4), (2, 2, 2), (4, 1, 2), (4, 2, 2),
    (4, 1, 4), (8, 1, 2),
)
# (N, K) of an expert's weight -> ((WPB, U, NT) for T <= 16, for T > 16):
# Mixtral-8x7B's gate/up (2I, D) and down (D, I) and their TP-2/4/8 shards of
# I; the winners of `kernel_bench.py --which moe_decode_sweep`
# (profiles/README.md, "Routed MoE decode").
MOE_DECODE_SHAPES: dict = {
    (28672, 4096): ((8, 1, 2), (4, 1, 4)),    # gate/up
    (14336, 4096): ((4, 2, 2), (4, 1, 4)),    # gate/up, TP 2
    (7168, 4096): ((8, 1, 2), (4, 1, 4)),     # gate/up, TP 4
    (3584, 4096): ((4, 2, 2), (4, 1, 4)),     # gate/up, TP 8
    (4096, 14336): ((4, 2, 2), (4, 1, 4)),    # down
    (4096, 7168): ((8, 1, 2), (4, 1, 4)),     # down, TP 2
    (4096, 3584): ((4, 1, 2), (4, 1, 4)),     # down, TP 4
    (4096, 1792): ((4, 1, 2), (4, 1, 4)),     # down, TP 8
}


# Quantised experts (Fp8ExpertWeight, Mxfp4ExpertWeight): the points of
# moe_routed_gemm_fp8 / moe_routed_gemm_mxfp4, whose steps are 128 / 256 k;
# copies of MOE_DECODE_FP8_CONFIGS / MOE_DECODE_MXFP4_CONFIGS of the kernel
# file, checked against hip().moe_decode_quant_configs(). The routed kernels
# are these holders' only decode route, so DYNAMO_MOE_FUSED does not apply.
MOE_DECODE_FP8_CONFIGS: tuple = (
    (1, 1, 2), (1, 2, 2), (2, 1, 4), (2, 2, 2), (4, 1, 2), (4, 2, 2),
    (4, 1, 4), (8, 1, 2),
)
MOE_DECODE_MXFP4_CONFIGS: tuple = (
    (1, 1, 2), (1, 2, 2), (2, 1, 2), (2, 1, 4), (4, 1, 2), (4, 1, 4),
    (8, 1, 2),
)
# As MOE_DECODE_SHAPES, per format (`kernel_bench.py --which
# moe_decode_sweep`; profiles/README.md, "Routed MoE decode"); a shape not
# listed takes the fallback rule of moe_decode_config.
MOE_DECODE_FP8_SHAPES: dict = {
    (28672, 4096): ((4, 2, 2), (2, 1, 4)),    # gate/up
    (14336, 4096): ((4, 2, 2), (2, 1, 4)),    # gate/up, TP 2
    (7168, 4096): ((8, 1, 2), (2, 1, 4)),     # gate/up, TP 4
    (3584, 4096): ((2, 2, 2), (4, 1, 4)),     # gate/up, TP 8
    (4096, 14336): ((4, 2, 2), (4, 1, 4)),    # down
    (4096, 7168): ((8, 1, 2), (4, 1, 4)),     # down, TP 2
    (4096, 3584): ((4, 1, 2), (4, 1, 4)),     # down, TP 4
    (4096, 1792): ((1, 2, 2), (1, 2, 2)),     # down, TP 8
}
MOE_DECODE_MXFP4_SHAPES: dict = {
    (28672, 4096): ((1, 2, 2), (1, 1, 2)),    # gate/up
    (14336, 4096): ((4, 1, 4), (2, 1, 4)),    # gate/up, TP 2
    (7168, 4096): ((4, 1, 4), (1, 1, 2)),     # gate/up, TP 4
    (3584, 4096): ((1, 2, 2), (2, 1, 4)),     # gate/up, TP 8
    (4096, 14336): ((8, 1, 2), (4, 1, 4)),    # down
    (4096, 7168): ((4, 1, 4), (2, 1, 4)),     # down, TP 2
    (4096, 3584): ((1, 2, 2), (2, 1, 4)),     # down, TP 4
    (4096, 1792): ((1, 1, 2), (1, 1, 2)),     # down, TP 8
}
# format -> (k per step, points, shape table)
MOE_DECODE_FORMATS: dict = {
    "bf16": (64, MOE_DECODE_CONFIGS, MOE_DECODE_SHAPES),
    "fp8": (128, MOE_DECODE_FP8_CONFIGS, MOE_DECODE_FP8_SHAPES),
    "mxfp4": (256, MOE_DECODE_MXFP4_CONFIGS, MOE_DECODE_MXFP4_SHAPES),
}


def moe_format(w) -> str:
    """"bf16" | "fp8" | "mxfp4": the routed-GEMM format of expert weights w,
    a tensor [E, N, K] or an expert holder."""
    if isinstance(w, Fp8ExpertWeight):
        return "fp8"
    return "mxfp4" if isinstance(w, Mxfp4ExpertWeight) else "bf16"


def moe_decode_config(N: int, K: int, T: int, fmt: str = "bf16"):
    """The (WPB, U, NT) the routed GEMM of format `fmt` runs an expert weight
    [N, K] at for T tokens: the shape's entry in the format's table, else the
    deepest point of the format's points (largest K step WPB * kstep * U, the
    earlier one among equals) that divides K. None if the kernel does not
    take the shape."""
    kstep, configs, shapes = MOE_DECODE_FORMATS[fmt]
    if not (1 <= T <= MOE_DECODE_MAX_T and N >= 16 and N % 16 == 0
            and K >= kstep and K % kstep == 0):
        return None
    entry = shapes.get((N, K))
    if entry is not None:
        return entry[0 if T <= 16 else 1]
    fits = [c for c in configs if K % (c[0] * kstep * c[1]) == 0]
    return max(fits, key=lambda c: c[0] * c[1])


def moe_route(topi: torch.Tensor, E: int):
    """topi [T, K] int32 -> (seg_start [E + 1], pair_of [T K]), int32: the
    pairs p = t K + j grouped by expert, ascending within an expert (equal to
    argsort(topi.flatten(), stable=True)), and each expert's first sorted
    position."""
    if not topi.is_cuda:
        return torch_ref.moe_route(topi, E)
    seg_start = torch.empty(E + 1, dtype=torch.int32, device=topi.device)
    pair_of = torch.empty(topi.numel(), dtype=torch.int32, device=topi.device)
    hip().moe_route(topi.contiguous(), seg_start, pair_of)
    return seg_start, pair_of


def _moe_cfg(w, T, cfg):
    cfg = cfg or moe_decode_config(w.shape[1], w.shape[2], T, moe_format(w))
    if cfg is None:
        raise ValueError(f"no routed MoE GEMM for {moe_format(w)} expert "
                         f"weights {tuple(w.shape)} at T = {T}")
    return cfg


def _moe_launch(out, a, w, seg_start, pair_of, topw, topk, gather, epilogue,
                cfg):
    """The routed GEMM binding of w's format."""
    fmt = moe_format(w)
    if fmt == "bf16":
        return hip().moe_routed_gemm(out, a, w, seg_start, pair_of, topw,
                                     topk, gather, epilogue, *cfg)
    getattr(hip(), "moe_routed_gemm_" + fmt)(
        out, a, w.q, w.scale, seg_start, pair_of, topw, topk, gather,
        epilogue, *cfg)


def _moe_effective(w, dtype):
    """Expert weights as a tensor: W_eff of a holder (the CPU path)."""
    return w if isinstance(w, torch.Tensor) else w.effective(dtype)


def moe_routed_gemm(a, w, seg_start, pair_of, topk: int, *, gather: bool,
                    glu: bool, cfg=None):
    """Sorted row i of expert e times w[e]^T, w [E, N, K] -> bf16 [T topk, N]
    in sorted order. gather: a is x [T, K] and row i is x[pair_of[i] // topk];
    else a is [T topk, K], already sorted. glu: w[e] is a gate/up weight and
    the result is [T topk, N / 2] = silu_mul of the plain one, equal bits.
    w is a bf16 tensor or an Fp8ExpertWeight / Mxfp4ExpertWeight."""
    if not a.is_cuda:
        return torch_ref.moe_routed_gemm(a, _moe_effective(w, a.dtype),
                                         seg_start, pair_of, topk, gather,
                                         glu)
    P = pair_of.numel()
    cfg = _moe_cfg(w, P // topk, cfg)
    y = torch.empty(P, w.shape[1] // 2 if glu else w.shape[1], dtype=a.dtype,
                    device=a.device)
    _moe_launch(y, a, w, seg_start, pair_of, None, topk, gather,
                1 if glu else 0, cfg)
    return y


def moe_down_combine(act, w_down, seg_start, pair_of, topw, cfg=None):
    """out[t] = bf16(sum_j topw[t, j] * act[row of pair (t, j)] @ w_down[e]^T)
    -> [T, D]: act [T topk, I] in sorted order, topw [T, topk] fp32. The GEMM
    writes fp32 rows already multiplied by the gate weight, the combine sums
    them in ascending j and rounds once."""
    if not act.is_cuda:
        return torch_ref.moe_down_combine(
            act, _moe_effective(w_down, act.dtype), seg_start, pair_of, topw)
    T, topk = topw.shape
    cfg = _moe_cfg(w_down, T, cfg)
    part = torch.empty(T * topk, w_down.shape[1], dtype=torch.float32,
                       device=act.device)
    _moe_launch(part, act, w_down, seg_start, pair_of, topw.contiguous(),
                topk, False, 2, cfg)
    out = torch.empty(T, w_down.shape[1], dtype=act.dtype, device=act.device)
    hip().moe_combine(out, part, topk)
    return out


def _moe_weight_ready(w, fmt: str) -> bool:
    """What the format's routed GEMM asks of the expert weights' storage."""
    if fmt == "bf16":
        return w.dtype == torch.bfloat16 and w.is_contiguous()
    return (w.q.is_contiguous() and w.scale.is_contiguous()
            and w.q.data_ptr() % 16 == 0 and w.scale.data_ptr() % 8 == 0)


def moe_decode_ready(x, topk: int, w_gate_up, w_down) -> bool:
    """Whether moe_decode_mlp takes the call on the GPU: the kernels' limits
    on T, top-k and E, bf16 activations, both weights of one format, and a
    configuration of that format for both GEMMs."""
    T = x.shape[0]
    E, N, K = w_gate_up.shape
    fmt = moe_format(w_gate_up)
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16
            and moe_format(w_down) == fmt
            and _moe_weight_ready(w_gate_up, fmt)
            and _moe_weight_ready(w_down, fmt)
            and 1 <= T <= MOE_DECODE_MAX_T
            and 1 <= topk <= MOE_DECODE_MAX_TOPK and E <= MOE_DECODE_MAX_E
            and N % 32 == 0 and x.is_contiguous()
            and moe_decode_config(N, K, T, fmt) is not None
            and moe_decode_config(w_down.shape[1], w_down.shape[2], T, fmt)
            is not None)


def moe_decode_mlp(x, topw, topi, w_gate_up, w_down):
    """The routed expert MLP of a decode step: x [T, D] bf16, topw / topi
    [T, topk] fp32 / int32 of topk_gating, w_gate_up [E, 2I, D] (gate rows
    first), w_down [E, D, I] -> [T, D] bf16. The weights are bf16 tensors or
    expert holders of one format; on the CPU holders compute through
    torch_ref with effective()."""
    topk = topi.shape[1]
    seg_start, pair_of = moe_route(topi, w_gate_up.shape[0])
    act = moe_routed_gemm(x, w_gate_up, seg_start, pair_of, topk,
                          gather=True, glu=True)
    return moe_down_combine(act, w_down, seg_start, pair_of, topw.float())


# --------------------------------------------------------------------------
# Routed MoE, tiled (csrc/moe_tile_gemm.hip): quantised experts above the
# decode route's 64 tokens. A route for up to MOE_TILE_KERNEL_MAX_T * 8 pairs
# that also writes the map of BM-row tiles, the expert-grouped tiled GEMM
# (the dense tiled kernel's main loop over expert segments) for gate/up +
# SwiGLU and for the gate-weighted down projection, and moe_combine: five
# launches, no host read, hipGraph-safe. Opt-in (DYNAMO_MOE_TILED=1 /
# set_moe_tiled): off, such calls take MoEMLP._expert_loop as before.
MOE_TILE_KERNEL_MAX_T = 4096
# The dispatch limit: the largest swept T (128 .. 2048) at which the route was
# ahead of the host loop on the full and the TP-2 shapes in both runs of
# `kernel_bench.py --which moe_tiled_sweep` (profiles/README.md, "Routed MoE,
# tiled"): all of them, 1.2-4.7x; nothing above 2048 was measured.
MOE_TILE_MAX_T = 2048
MOE_TILE_BMS: tuple = (32, 64, 128)
# pairs per block of the route kernels (ROUTE_THREADS of the kernel file): the
# histogram scratch holds one row of E counts per block
MOE_TILE_ROUTE_BLOCK = 512
# (BM, WN, WK, NT, U) points of moe_tiled_gemm_fp8 / _mxfp4; they need
# K % (WK * kstep * U) == 0. Copies of the kernel file's tables, checked
# against hip().moe_tile_configs(). The first point of every BM accepts every
# K % kstep == 0.
MOE_TILE_CONFIGS: dict = {
    "fp8": ((32, 4, 1, 2, 1), (64, 4, 1, 2, 1), (128, 4, 1, 2, 1),
            (32, 4, 2, 2, 2), (64, 4, 2, 2, 2), (128, 4, 2, 2, 2),
            (32, 8, 1, 2, 2), (64, 8, 1, 2, 2), (128, 8, 1, 2, 2)),
    "mxfp4": ((32, 4, 1, 2, 1), (64, 4, 1, 2, 1), (128, 4, 1, 2, 1),
              (32, 4, 2, 2, 1), (64, 4, 2, 2, 1),
              (32, 8, 1, 2, 1), (64, 8, 1, 2, 1), (128, 8, 1, 2, 1)),
}
# format -> (N, K) of an expert's weight -> the (WN, WK, NT, U) at BM = 32,
# 64, 128, for the Mixtral-8x7B expert shapes of MOE_DECODE_SHAPES that
# `kernel_bench.py --which moe_tiled_sweep` covers (profiles/README.md,
# "Routed MoE, tiled"); a shape not listed takes moe_tile_config's fallback.
MOE_TILE_SHAPES: dict = {
    "fp8": {
        (28672, 4096): ((8, 1, 2, 2), (8, 1, 2, 2), (8, 1, 2, 2)),  # gate/up
        (14336, 4096): ((4, 1, 2, 1), (4, 1, 2, 1), (8, 1, 2, 2)),  # ..., TP 2
        (4096, 14336): ((4, 2, 2, 2), (4, 1, 2, 1), (8, 1, 2, 2)),  # down
        (4096, 7168): ((4, 2, 2, 2), (4, 1, 2, 1), (8, 1, 2, 2)),   # ..., TP 2
    },
    "mxfp4": {
        (28672, 4096): ((8, 1, 2, 1), (8, 1, 2, 1), (8, 1, 2, 1)),
        (14336, 4096): ((4, 1, 2, 1), (8, 1, 2, 1), (8, 1, 2, 1)),
        (4096, 14336): ((4, 1, 2, 1), (8, 1, 2, 1), (8, 1, 2, 1)),
        (4096, 7168): ((4, 1, 2, 1), (8, 1, 2, 1), (8, 1, 2, 1)),
    },
}

_moe_tiled_override: "bool | None" = None


def set_moe_tiled(on: "bool | None") -> None:
    """In-process override of DYNAMO_MOE_TILED (None = follow the env)."""
    global _moe_tiled_override
    _moe_tiled_override = on


def moe_tiled_enabled() -> bool:
    if _moe_tiled_override is not None:
        return _moe_tiled_override
    from dynamo_amd import envs
    return envs.get("DYNAMO_MOE_TILED", False, bool)


def moe_tile_bm(T: int, topk: int, E: int) -> int:
    """The tile height for T tokens: the smallest BM that holds the mean
    segment T topk / E in one tile, 128 above that."""
    mean = T * topk / E
    return next((bm for bm in MOE_TILE_BMS if mean <= bm), MOE_TILE_BMS[-1])


def moe_tile_config(N: int, K: int, T: int, topk: int, E: int, fmt: str):
    """The (BM, WN, WK, NT, U) the tiled routed GEMM of `fmt` runs an expert
    weight [N, K] at: BM from the mean segment size, the rest from the
    shape's entry in MOE_TILE_SHAPES, else (or where K does not allow the
    entry) the deepest point of that BM (largest K step WK * kstep * U, the
    earlier one among equals) that divides K. None if the kernel does not
    take the call."""
    if fmt not in MOE_TILE_CONFIGS:
        return None
    kstep = MOE_DECODE_FORMATS[fmt][0]
    if not (MOE_DECODE_MAX_T < T <= MOE_TILE_KERNEL_MAX_T
            and 1 <= topk <= MOE_DECODE_MAX_TOPK and 1 <= E <= MOE_DECODE_MAX_E
            and N >= 16 and N % 16 == 0 and K >= kstep and K % kstep == 0):
        return None
    bm = moe_tile_bm(T, topk, E)
    fits = [c for c in MOE_TILE_CONFIGS[fmt]
            if c[0] == bm and K % (c[2] * kstep * c[4]) == 0]
    entry = MOE_TILE_SHAPES[fmt].get((N, K))
    if entry is not None:
        point = (bm, *entry[MOE_TILE_BMS.index(bm)])
        if point in fits:
            return point
    return max(fits, key=lambda c: c[2] * c[4])


def moe_route_tiled(topi: torch.Tensor, E: int, BM: int):
    """moe_route for up to MOE_TILE_KERNEL_MAX_T tokens, with the map of
    BM-row tiles: -> (seg_start [E + 1], pair_of [T K], tile_expert,
    tile_row0, ntiles), int32. On the GPU the tile arrays hold
    T K // BM + min(E, T K) entries of which the first ntiles [1] (a device
    tensor) are written; on the CPU they hold exactly ntiles (an int)."""
    if not topi.is_cuda:
        seg_start, pair_of = torch_ref.moe_route(topi, E)
        return (seg_start, pair_of, *torch_ref.moe_tile_map(seg_start, BM))
    P = topi.numel()

    def i32(n):
        return torch.empty(n, dtype=torch.int32, device=topi.device)
    max_tiles = P // BM + min(E, P)
    route = (i32(E + 1), i32(P), i32(max_tiles), i32(max_tiles), i32(1))
    hist = i32(-(-P // MOE_TILE_ROUTE_BLOCK) * E)
    hip().moe_route_tiled(topi.contiguous(), *route, hist, BM)
    return route


def _moe_tiled_cfg(w, T, topk, cfg):
    fmt = moe_format(w)
    cfg = cfg or moe_tile_config(w.shape[1], w.shape[2], T, topk, w.shape[0],
                                 fmt)
    if cfg is None:
        raise ValueError(f"no tiled routed MoE GEMM for {fmt} expert weights "
                         f"{tuple(w.shape)} at T = {T}")
    return cfg


def moe_tiled_gemm(a, w, route, topk: int, *, gather: bool, glu: bool,
                   cfg=None):
    """moe_routed_gemm on the tiled kernel: `route` is moe_route_tiled's
    result at cfg's BM, w an Fp8ExpertWeight / Mxfp4ExpertWeight."""
    seg_start, pair_of = route[:2]
    if not a.is_cuda:
        return torch_ref.moe_routed_gemm(a, _moe_effective(w, a.dtype),
                                         seg_start, pair_of, topk, gather,
                                         glu)
    P = pair_of.numel()
    cfg = _moe_tiled_cfg(w, P // topk, topk, cfg)
    y = torch.empty(P, w.shape[1] // 2 if glu else w.shape[1], dtype=a.dtype,
                    device=a.device)
    getattr(hip(), "moe_tiled_gemm_" + moe_format(w))(
        y, a, w.q, w.scale, *route, None, topk, gather, 1 if glu else 0, *cfg)
    return y


def moe_tiled_down_combine(act, w_down, route, topw, cfg=None):
    """moe_down_combine on the tiled kernel: fp32 rows times the gate weight,
    summed per token in ascending j and rounded once."""
    seg_start, pair_of = route[:2]
    if not act.is_cuda:
        return torch_ref.moe_down_combine(
            act, _moe_effective(w_down, act.dtype), seg_start, pair_of, topw)
    T, topk = topw.shape
    cfg = _moe_tiled_cfg(w_down, T, topk, cfg)
    part = torch.empty(T * topk, w_down.shape[1], dtype=torch.float32,
                       device=act.device)
    getattr(hip(), "moe_tiled_gemm_" + moe_format(w_down))(
        part, act, w_down.q, w_down.scale, *route, topw.contiguous(), topk,
        False, 2, *cfg)
    out = torch.empty(T, w_down.shape[1], dtype=act.dtype, device=act.device)
    hip().moe_combine(out, part, topk)
    return out


def moe_tiled_ready(x, topk: int, w_gate_up, w_down) -> bool:
    """Whether moe_tiled_mlp takes the call on the GPU: 64 < T <=
    MOE_TILE_MAX_T, quantised weights of one format stored as the kernels
    ask, bf16 contiguous x, and a configuration for both GEMMs."""
    T = x.shape[0]
    E, N, K = w_gate_up.shape
    fmt = moe_format(w_gate_up)
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16
            and fmt != "bf16" and moe_format(w_down) == fmt
            and _moe_weight_ready(w_gate_up, fmt)
            and _moe_weight_ready(w_down, fmt)
            and MOE_DECODE_MAX_T < T <= MOE_TILE_MAX_T
            and N % 32 == 0 and x.is_contiguous()
            and x.data_ptr() % 16 == 0
            and moe_tile_config(N, K, T, topk, E, fmt) is not None
            and moe_tile_config(w_down.shape[1], w_down.shape[2], T, topk, E,
                                fmt) is not None)


def moe_tiled_mlp(x, topw, topi, w_gate_up, w_down):
    """moe_decode_mlp for 64 < T <= MOE_TILE_MAX_T and quantised experts, on
    the tiled kernels; the CPU computes through torch_ref with effective()."""
    T, topk = topi.shape
    E = w_gate_up.shape[0]
    route = moe_route_tiled(topi, E, moe_tile_bm(T, topk, E))
    act = moe_tiled_gemm(x, w_gate_up, route, topk, gather=True, glu=True)
    return moe_tiled_down_combine(act, w_down, route, topw.float())


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
