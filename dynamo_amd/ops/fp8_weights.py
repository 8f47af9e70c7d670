"""Opt-in FP8 (OCP e4m3) weights: W8A16 weight-only quantisation.

The dense projections are stored as float8_e4m3fn with one fp32 scale per
output row; activations, accumulation and outputs stay as they are (bf16 in,
fp32 accumulate, bf16 out). The effective weight is defined once,

    W_eff = (q.float() * scale[:, None]).to(compute dtype)

and every path computes x @ W_eff^T: the in-tree W8A16 kernel (the Fp8Coal
format of csrc/skinny_gemm_impl.h) for decode-regime calls on the GPU,
fp8_dequant into a per-device scratch buffer followed by the library GEMM for
every other GPU call, and F.linear(x, W_eff) on the CPU. Dispatch lives in
ops.linear.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

E4M3_MAX = 448.0


def quantize_fp8_rowwise(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] -> (q float8_e4m3fn [N, K], scale fp32 [N]).

    scale = absmax(row) / 448, or 1 for an all-zero row. The clamp matters:
    torch's e4m3fn cast does not saturate, so a quotient that the fp32 divide
    rounds past 448 would otherwise become a NaN code."""
    assert w.dim() == 2, "quantize_fp8_rowwise: w [N, K]"
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    q = (wf / scale[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(
        torch.float8_e4m3fn)
    return q.contiguous(), scale.contiguous()


class Fp8Weight:
    """A quantised [N, K] weight: `q` float8_e4m3fn [N, K], `scale` fp32 [N].
    Deliberately not a torch.Tensor: code that expects a plain weight tensor
    fails loudly instead of computing on the raw codes."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        assert q.dtype == torch.float8_e4m3fn and q.dim() == 2
        assert scale.dtype == torch.float32 and scale.shape == (q.shape[0],)
        self.q = q
        self.scale = scale

    @staticmethod
    def from_tensor(w: torch.Tensor) -> "Fp8Weight":
        return Fp8Weight(*quantize_fp8_rowwise(w))

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    def dim(self) -> int:
        return 2

    def effective(self, dtype: torch.dtype) -> torch.Tensor:
        """W_eff in the compute dtype."""
        return (self.q.float() * self.scale[:, None]).to(dtype)


# One bf16 scratch buffer per device for the dequantise-then-library path.
# Stream order makes one buffer enough: the GEMM that reads it is queued
# before the next dequantisation that overwrites it.
_scratch: Dict[torch.device, torch.Tensor] = {}


def reserve_scratch(device, numel: int) -> None:
    """Make the device's scratch buffer hold at least `numel` bf16 elements.
    quantize_model_fp8 calls this before any graph capture."""
    device = torch.device(device)
    buf = _scratch.get(device)
    if buf is None or buf.numel() < numel:
        _scratch[device] = torch.empty(numel, dtype=torch.bfloat16,
                                       device=device)


def scratch_view(w) -> torch.Tensor:
    """A bf16 [N, K] view of the device's scratch buffer for the quantised
    weight holder w (an Fp8Weight or an Mxfp4Weight) to be dequantised
    into."""
    N, K = w.shape
    reserve_scratch(w.q.device, N * K)
    return _scratch[w.q.device][:N * K].view(N, K)


PROJECTIONS = (("attn", "wqkv"), ("attn", "wo"),
               ("mlp", "w_gate_up"), ("mlp", "w_down"))


def is_fp8_model(model) -> bool:
    return getattr(model, "weight_dtype", None) == "fp8"


def quantize_model_fp8(model) -> int:
    """Replace Attention.wqkv / wo and SwiGLUMLP.w_gate_up / w_down of every
    layer by Fp8Weight holders, layer by layer, freeing each bf16 tensor as it
    goes. Rank-local: a TP shard quantises its own rows or columns.
    Embedding, lm_head, norms and biases keep the compute dtype. Returns the
    number of quantised matrices."""
    count, largest, device = 0, 0, None
    with torch.no_grad():
        for layer in model.layers:
            for sub, name in PROJECTIONS:
                mod = getattr(layer, sub, None)
                w = getattr(mod, name, None) if mod is not None else None
                if not isinstance(w, torch.Tensor):
                    raise ValueError(
                        f"fp8 weights: layer has no dense {sub}.{name}")
                holder = Fp8Weight.from_tensor(w)
                setattr(mod, name, holder)
                largest = max(largest, w.numel())
                device = w.device
                del w
                count += 1
    model.weight_dtype = "fp8"
    if device is not None and device.type == "cuda":
        reserve_scratch(device, largest)
        # hand the freed bf16 blocks back so the KV pool sizing sees them
        torch.cuda.empty_cache()
    return count
