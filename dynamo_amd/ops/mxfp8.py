"""MXFP8 activation rows: the A operand of the W8A8 / W4A8 prefill GEMM
(csrc/mx_gemm.hip).

A row of x is stored in the OCP microscaling FP8 format: e4m3 elements with
one e8m0 power-of-two scale byte per block of 32 consecutive k,

    x_eff[m, k] = xq[m, k] * 2^(xs[m, k/32] - 127)

The quantiser: per block, e = floor(log2(amax)) - 7, so amax / 2^e lies in
[128, 256) and nothing saturates (e4m3 reaches 448); elements are x / 2^e
rounded to nearest even into e4m3, subnormals (spacing 2^-9) included. Hence
|x - x_eff| <= max(2^-4 |x|, 2^(e - 10)) per element. e is clamped to
[-126, 127] (an all-zero block gets 0), so 2^e and 2^-e are normal fp32
numbers and e + 127 is a valid e8m0 byte.

quantize_mxfp8_rows is the specification; the kernel mxfp8_quantize_rows
reproduces its bytes. The kernel converts with v_cvt_pk_fp8_f32 after an exact
power-of-two scaling in fp32 rather than with the v_cvt_scalef32 family: the
plain conversion is the one whose rounding (nearest even, e4m3 subnormals
kept) is torch's.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .mxfp4_weights import _pow2

BLOCK = 32
E_MIN, E_MAX = -126, 127


def quantize_mxfp8_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [M, K] -> (xq float8_e4m3fn [M, K], xs uint8 [M, K/32]);
    K % 32 == 0."""
    if x.dim() != 2 or x.shape[1] % BLOCK:
        raise ValueError(
            f"quantize_mxfp8_rows: x must be [M, K] with K % {BLOCK} == 0, "
            f"got {tuple(x.shape)}")
    M, K = x.shape
    xf = x.float().view(M, K // BLOCK, BLOCK)
    amax = xf.abs().amax(dim=2)
    # amax = m * 2^ex with m in [0.5, 1): floor(log2(amax)) = ex - 1, exactly
    _, ex = torch.frexp(amax)
    e = torch.where(amax > 0, (ex - 8).clamp(E_MIN, E_MAX),
                    torch.zeros_like(ex)).to(torch.int32)
    v = xf * _pow2(-e)[:, :, None]              # a power-of-two scaling: exact
    xq = v.view(M, K).to(torch.float8_e4m3fn)
    return xq.contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_mxfp8_rows(xq: torch.Tensor, xs: torch.Tensor,
                          dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """x_eff [M, K] of (xq [M, K], xs [M, K/32])."""
    M, K = xq.shape
    s = _pow2(xs.to(torch.int32) - 127)
    return (xq.float().view(M, K // BLOCK, BLOCK)
            * s[:, :, None]).view(M, K).to(dtype)


# One (xq, xs) scratch pair per device for the quantise-then-GEMM path. Stream
# order makes one pair enough: the GEMM that reads it is queued before the
# next quantisation that overwrites it.
_scratch: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor]] = {}


def reserve_scratch(device, numel: int) -> None:
    """Make the device's scratch pair hold at least `numel` elements of x
    (numel bytes of codes, numel / 32 scale bytes). The model runner calls
    this before any graph capture."""
    device = torch.device(device)
    pair = _scratch.get(device)
    if pair is None or pair[0].numel() < numel:
        _scratch[device] = (
            torch.empty(numel, dtype=torch.float8_e4m3fn, device=device),
            torch.empty(-(-numel // BLOCK), dtype=torch.uint8, device=device))


def scratch_views(device, M: int, K: int):
    """(xq [M, K], xs [M, K/32]) views of the device's scratch pair."""
    reserve_scratch(device, M * K)
    xq, xs = _scratch[torch.device(device)]
    return xq[:M * K].view(M, K), xs[:M * K // BLOCK].view(M, K // BLOCK)
