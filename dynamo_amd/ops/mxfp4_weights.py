"""Opt-in MXFP4 weights: W4A16 weight-only quantisation in the OCP
microscaling FP4 format.

The dense projections are stored as e2m1 codes, two per byte (even k in the
low nibble, odd k in the high one: the OCP and hardware packing order), with
one e8m0 power-of-two scale byte per block of 32 consecutive k of a row: 4.25
bits per weight. Activations, accumulation and outputs stay as they are (bf16
in, fp32 accumulate, bf16 out). The effective weight is defined once,

    W_eff[n, k] = grid[code & 7] * (-1 if code & 8) * 2^(scale[n, k/32] - 127)

with grid = {0, 0.5, 1, 1.5, 2, 3, 4, 6}; it is exact in bf16 (at most two
significant bits times a power of two). Every path computes x @ W_eff^T: the
in-tree W4A16 kernel (the Mxfp4Coal format of csrc/skinny_gemm_impl.h) for
decode-regime calls on the GPU, mxfp4_dequant into the per-device scratch
buffer (shared with ops/fp8_weights.py) followed by the library GEMM for every
other GPU call, and F.linear(x, W_eff) on the CPU. Dispatch lives in
ops.linear.

The quantiser: per block, e = floor(log2(amax)) - 2, so amax / 2^e lies in
[4, 8) and the largest element lands on code 6 or 7; elements in (6, 8)
saturate at 6. The grid's spacing is at most 2 and saturation loses less than
2, hence |w - W_eff| < 2 * 2^e per element. e is clamped to [-100, 100] (an
all-zero block gets 0), which keeps every code * 2^e a normal bf16 and fp32
number: no path depends on a denormal mode.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import fp8_weights
from .fp8_weights import PROJECTIONS

BLOCK = 32
E_MIN, E_MAX = -100, 100
E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# value of each of the 16 codes; code 8 is -0
_CODE_VALUES = E2M1_GRID + tuple(-v for v in E2M1_GRID)


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for an integer tensor e in [-126, 127], built from the
    exponent bits: exact."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def quantize_mxfp4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] -> (q uint8 [N, K/2], scale uint8 [N, K/32]); K % 32 == 0.

    Rounds to the nearest grid point, ties to the even code, saturating at 6;
    bit 3 of a code is the sign of w."""
    if w.dim() != 2 or w.shape[1] % BLOCK:
        raise ValueError(
            f"quantize_mxfp4: w must be [N, K] with K % {BLOCK} == 0, got "
            f"{tuple(w.shape)}")
    N, K = w.shape
    wf = w.float().view(N, K // BLOCK, BLOCK)
    amax = wf.abs().amax(dim=2)
    # amax = m * 2^ex with m in [0.5, 1): floor(log2(amax)) = ex - 1, exactly
    _, ex = torch.frexp(amax)
    e = torch.where(amax > 0, (ex - 3).clamp(E_MIN, E_MAX),
                    torch.zeros_like(ex)).to(torch.int32)
    v = wf.abs() * _pow2(-e)[:, :, None]        # a power-of-two scaling: exact
    # midpoints of the grid; >= where the upper neighbour is the even code
    code = ((v > 0.25).to(torch.uint8) + (v >= 0.75) + (v > 1.25)
            + (v >= 1.75) + (v > 2.5) + (v >= 3.5) + (v > 5.0))
    code = (code | (torch.signbit(wf).to(torch.uint8) << 3)).view(N, K)
    q = code[:, 0::2] | (code[:, 1::2] << 4)
    return q.contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4(q: torch.Tensor, scale: torch.Tensor,
                     dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """W_eff [N, K] of (q [N, K/2], scale [N, K/32])."""
    N, K = q.shape[0], q.shape[1] * 2
    codes = torch.stack((q & 15, q >> 4), dim=2).view(N, K).long()
    values = torch.tensor(_CODE_VALUES, dtype=torch.float32, device=q.device)
    s = _pow2(scale.to(torch.int32) - 127)
    return (values[codes].view(N, K // BLOCK, BLOCK)
            * s[:, :, None]).view(N, K).to(dtype)


class Mxfp4Weight:
    """A quantised [N, K] weight: `q` uint8 [N, K/2], `scale` uint8
    [N, K/32]. Deliberately not a torch.Tensor: code that expects a plain
    weight tensor fails loudly instead of computing on the raw codes."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        assert q.dtype == torch.uint8 and q.dim() == 2
        assert q.shape[1] % (BLOCK // 2) == 0
        assert scale.dtype == torch.uint8
        assert scale.shape == (q.shape[0], q.shape[1] * 2 // BLOCK)
        self.q = q
        self.scale = scale

    @staticmethod
    def from_tensor(w: torch.Tensor) -> "Mxfp4Weight":
        return Mxfp4Weight(*quantize_mxfp4(w))

    @property
    def shape(self):
        """The logical (N, K)."""
        return torch.Size((self.q.shape[0], self.q.shape[1] * 2))

    @property
    def device(self):
        return self.q.device

    def dim(self) -> int:
        return 2

    def effective(self, dtype: torch.dtype) -> torch.Tensor:
        """W_eff in the compute dtype."""
        return dequantize_mxfp4(self.q, self.scale, dtype)


def is_mxfp4_model(model) -> bool:
    return getattr(model, "weight_dtype", None) == "mxfp4"


def quantize_model_mxfp4(model) -> int:
    """Replace Attention.wqkv / wo and SwiGLUMLP.w_gate_up / w_down of every
    layer by Mxfp4Weight holders, layer by layer, freeing each bf16 tensor as
    it goes. Rank-local: a TP shard quantises its own rows or columns, so
    blocks never span ranks. Embedding, lm_head, norms and biases keep the
    compute dtype. Raises ValueError if a projection's K is no multiple of
    32. Returns the number of quantised matrices."""
    # refuse before the first matrix is replaced
    for layer in model.layers:
        for sub, name in PROJECTIONS:
            w = getattr(getattr(layer, sub, None), name, None)
            if not isinstance(w, torch.Tensor):
                raise ValueError(
                    f"mxfp4 weights: layer has no dense {sub}.{name}")
            if w.shape[1] % BLOCK:
                raise ValueError(
                    f"mxfp4 weights: {sub}.{name} has K = {w.shape[1]}, "
                    f"not a multiple of the {BLOCK}-element MX block")
    count, largest, device = 0, 0, None
    with torch.no_grad():
        for layer in model.layers:
            for sub, name in PROJECTIONS:
                mod = getattr(layer, sub)
                w = getattr(mod, name)
                holder = Mxfp4Weight.from_tensor(w)
                setattr(mod, name, holder)
                largest = max(largest, w.numel())
                device = w.device
                del w
                count += 1
    model.weight_dtype = "mxfp4"
    if device is not None and device.type == "cuda":
        fp8_weights.reserve_scratch(device, largest)
        # hand the freed bf16 blocks back so the KV pool sizing sees them
        torch.cuda.empty_cache()
    return count
