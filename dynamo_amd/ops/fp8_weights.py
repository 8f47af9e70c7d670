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


class Fp8ExpertWeight:
    """Quantised expert weights [E, N, K]: `q` float8_e4m3fn [E, N, K],
    `scale` fp32 [E, N], the row-wise quantiser applied to every expert's
    rows. holder[e] is expert e's Fp8Weight over views of both, so ops.linear
    and fp8_dequant serve a single expert. Not a tensor, as Fp8Weight."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        assert q.dtype == torch.float8_e4m3fn and q.dim() == 3
        assert scale.dtype == torch.float32 and scale.shape == q.shape[:2]
        self.q = q
        self.scale = scale

    @staticmethod
    def from_tensor(w: torch.Tensor) -> "Fp8ExpertWeight":
        """Quantises one expert at a time: the fp32 temporaries are one
        expert's, not the tensor's."""
        assert w.dim() == 3, "Fp8ExpertWeight: w [E, N, K]"
        q = torch.empty(w.shape, dtype=torch.float8_e4m3fn, device=w.device)
        scale = torch.empty(w.shape[:2], dtype=torch.float32, device=w.device)
        for e in range(w.shape[0]):
            q[e], scale[e] = quantize_fp8_rowwise(w[e])
        return Fp8ExpertWeight(q, scale)

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    def dim(self) -> int:
        return 3

    def __len__(self) -> int:
        return self.q.shape[0]

    def __getitem__(self, e: int) -> Fp8Weight:
        return Fp8Weight(self.q[e], self.scale[e])

    def effective(self, dtype: torch.dtype) -> torch.Tensor:
        """W_eff [E, N, K] in the compute dtype."""
        return (self.q.float() * self.scale[:, :, None]).to(dtype)


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


def layer_projections(layer, what: str):
    """[(module, attribute, dim)] of the weights a quantiser replaces in one
    layer: the four dense projections (dim 2), or for a MoE layer attn.wqkv /
    wo and the expert tensors moe.w_gate_up / w_down (dim 3, [E, N, K]); the
    router stays in the compute dtype. ValueError (`what` names the format)
    if a weight is missing or is no tensor of that rank."""
    moe = getattr(layer, "moe", None)
    if moe is not None and getattr(moe, "ep", False):
        raise ValueError(f"{what} weights: expert-parallel MoE layers slice "
                         "bf16 expert tensors on the host")
    names = (PROJECTIONS[:2] + (("moe", "w_gate_up", 3), ("moe", "w_down", 3))
             if moe is not None else PROJECTIONS)
    out = []
    for sub, name, *rank in names:
        mod = getattr(layer, sub, None)
        w = getattr(mod, name, None) if mod is not None else None
        dim = rank[0] if rank else 2
        if not isinstance(w, torch.Tensor) or w.dim() != dim:
            raise ValueError(f"{what} weights: layer has no dense {sub}.{name}"
                             f" of rank {dim}")
        out.append((mod, name, dim))
    return out


def quantize_model_fp8(model) -> int:
    """Replace Attention.wqkv / wo and SwiGLUMLP.w_gate_up / w_down of every
    layer by Fp8Weight holders, and a MoE layer's expert tensors by
    Fp8ExpertWeight holders (one expert at a time), layer by layer, freeing
    each bf16 tensor as it goes. Rank-local: a TP shard quantises its own rows
    or columns. Embedding, lm_head, the router, norms and biases keep the
    compute dtype. Returns the number of quantised tensors."""
    count, largest, device = 0, 0, None
    with torch.no_grad():
        for layer in model.layers:
            for mod, name, dim in layer_projections(layer, "fp8"):
                w = getattr(mod, name)
                holder = (Fp8Weight if dim == 2
                          else Fp8ExpertWeight).from_tensor(w)
                setattr(mod, name, holder)
                # the scratch buffer holds one matrix: a single expert's
                largest = max(largest, w[0].numel() if dim == 3 else w.numel())
                device = w.device
                del w
                count += 1
    model.weight_dtype = "fp8"
    if device is not None and device.type == "cuda":
        reserve_scratch(device, largest)
        # hand the freed bf16 blocks back so the KV pool sizing sees them
        torch.cuda.empty_cache()
    return count
