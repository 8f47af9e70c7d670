"""LoRA adapters for the native engine.

Capability parity with the reference's LoRA stack (ai-dynamo/dynamo
lib/llm/src/lora: downloader/cache/lora-aware routing, and the worker
endpoints load_lora/unload_lora/list_loras,
components/src/dynamo/vllm/worker_factory.py:1378-1413).

Design: low-rank deltas on the attention qkv/o and MLP gate_up/down
projections (y += (x A^T) B^T * alpha/r). Two modes:

* Adapter bank (EngineConfig.max_loras > 0): per-request adapter selection.
  LoRABank holds up to max_loras adapters in device-resident slots; every
  request names its adapter (or none) and the rows of one batch take their
  own adapter through the gathered kernels of csrc/lora.hip (decode rows) or
  two library GEMMs per prefill chunk. Loading or unloading an adapter
  touches only its slot: captured decode graphs stay valid, since the kernels
  read the row -> slot map from a device buffer.
* Engine-level activation (max_loras == 0, the default): one adapter is
  ACTIVE per engine at a time, for every request; activating/deactivating
  invalidates captured decode graphs. Multi-adapter serving then happens
  across workers - the router filters workers by the adapters they list.

Adapters load from a torch state-dict file, an HF PEFT directory, or are
random-initialized (seeded) for synthetic serving.
"""
from __future__ import annotations

import logging
from typing import Dict, List, Optional

import torch

log = logging.getLogger("dynamo_amd.lora")

TARGETS = ("qkv", "o", "gate_up", "down")


class LoRAAdapter:
    def __init__(self, name: str, rank: int, alpha: float,
                 weights: Dict[str, tuple]):
        """weights: {f"{layer}.{target}": (A [r, in], B [out, r])}"""
        self.name = name
        self.rank = rank
        self.alpha = alpha
        self.scale = alpha / rank
        self.weights = weights

    @staticmethod
    def random(name: str, model, rank: int = 8, alpha: float = 16.0,
               seed: int = 0, std: float = 0.1) -> "LoRAAdapter":
        g = torch.Generator(device="cpu").manual_seed(seed)
        weights = {}
        for li, layer in enumerate(model.layers):
            mods = _layer_targets(layer)
            for tgt, (w,) in mods.items():
                out_f, in_f = w.shape[-2], w.shape[-1]
                A = torch.empty(rank, in_f).normal_(0, std, generator=g)
                B = torch.empty(out_f, rank).normal_(0, std, generator=g)
                weights[f"{li}.{tgt}"] = (
                    A.to(w.device, w.dtype), B.to(w.device, w.dtype))
        return LoRAAdapter(name, rank, alpha, weights)

    @staticmethod
    def load(name: str, path: str, model, rank: int, alpha: float
             ) -> "LoRAAdapter":
        sd = torch.load(path, map_location="cpu")
        weights = {}
        for li, layer in enumerate(model.layers):
            for tgt, (w,) in _layer_targets(layer).items():
                key = f"{li}.{tgt}"
                A = sd[f"{key}.A"].to(w.device, w.dtype)
                B = sd[f"{key}.B"].to(w.device, w.dtype)
                weights[key] = (A, B)
        return LoRAAdapter(name, rank, alpha, weights)


def _layer_targets(layer) -> Dict[str, tuple]:
    out = {}
    if hasattr(layer, "attn"):
        out["qkv"] = (layer.attn.wqkv,)
        out["o"] = (layer.attn.wo,)
    if hasattr(layer, "mlp"):
        out["gate_up"] = (layer.mlp.w_gate_up,)
        out["down"] = (layer.mlp.w_down,)
    return out


class LoRAManager:
    """Holds loaded adapters and applies/clears the active one."""

    def __init__(self, model):
        self.model = model
        self.adapters: Dict[str, LoRAAdapter] = {}
        self.active: Optional[str] = None

    def load(self, name: str, path: Optional[str] = None, rank: int = 8,
             alpha: float = 16.0, seed: int = 0):
        import os
        if path and os.path.isdir(path) and os.path.exists(
                os.path.join(path, "adapter_config.json")):
            ad = load_peft_adapter(name, path, self.model)
        elif path:
            ad = LoRAAdapter.load(name, path, self.model, rank, alpha)
        else:
            ad = LoRAAdapter.random(name, self.model, rank, alpha, seed)
        self.adapters[name] = ad
        log.info("loaded LoRA %s (rank %d)", name, rank)

    def unload(self, name: str):
        if self.active == name:
            self.deactivate()
        self.adapters.pop(name, None)

    def list(self) -> List[str]:
        return sorted(self.adapters)

    def activate(self, name: str):
        ad = self.adapters[name]

        def pick(li, keys):
            # PEFT adapters may target a subset of projections
            return {k: ad.weights[f"{li}.{k}"] + (ad.scale,)
                    for k in keys if f"{li}.{k}" in ad.weights} or None

        for li, layer in enumerate(self.model.layers):
            if hasattr(layer, "attn"):
                layer.attn.lora = pick(li, ("qkv", "o"))
            if hasattr(layer, "mlp"):
                layer.mlp.lora = pick(li, ("gate_up", "down"))
        self.active = name

    def deactivate(self):
        for layer in self.model.layers:
            if hasattr(layer, "attn"):
                layer.attn.lora = None
            if hasattr(layer, "mlp"):
                layer.mlp.lora = None
        self.active = None


class LoRATargetBank:
    """The adapter slots of one (layer, target) projection [N, K]:
    A [S, R, K] and B [S, N, R] in the model dtype, ranks [S] int32 (the
    true rank of the adapter in each slot, 0 = none) and scales [S] fp32 on
    the device, plus host copies of ranks/scales for the prefill path."""

    def __init__(self, A, B, ranks, scales, host_ranks, host_scales):
        self.A, self.B, self.ranks, self.scales = A, B, ranks, scales
        self.host_ranks, self.host_scales = host_ranks, host_scales
        # what ops.lora_delta_ takes
        self.dev = (A, B, ranks, scales)


class LoRABank:
    """max_loras adapter slots of rank <= max_rank for every layer's four
    projections, allocated once; maps adapter name -> slot."""

    def __init__(self, model, max_loras: int, max_rank: int):
        if max_loras < 1:
            raise ValueError("LoRABank needs max_loras >= 1")
        if max_rank < 8 or max_rank % 8:
            raise ValueError(
                f"max_lora_rank must be a positive multiple of 8, got "
                f"{max_rank}")
        self.model = model
        self.S, self.R = max_loras, max_rank
        self.slot_of: Dict[str, int] = {}
        layers = list(model.layers)
        dev = dtype = None
        for layer in layers:
            for tgt, (w,) in _layer_targets(layer).items():
                if not isinstance(w, torch.Tensor) or w.dim() != 2:
                    raise ValueError(
                        "the LoRA adapter bank needs plain 2-D projection "
                        f"weights; {tgt} is {type(w).__name__}")
                dev, dtype = w.device, w.dtype
        S, R = self.S, self.R
        self.scales = torch.zeros(S, dtype=torch.float32, device=dev)
        self.host_scales = [0.0] * S
        self.ranks = torch.zeros(len(layers), len(TARGETS), S,
                                 dtype=torch.int32, device=dev)
        self.targets: Dict[str, LoRATargetBank] = {}
        for li, layer in enumerate(layers):
            for tgt, (w,) in _layer_targets(layer).items():
                N, K = w.shape
                if N % 8 or K % 8:
                    raise ValueError(
                        f"layer {li} {tgt} is [{N}, {K}]: the adapter bank "
                        "needs both to be multiples of 8")
                tb = LoRATargetBank(
                    torch.zeros(S, R, K, dtype=dtype, device=dev),
                    torch.zeros(S, N, R, dtype=dtype, device=dev),
                    self.ranks[li, TARGETS.index(tgt)], self.scales,
                    [0] * S, self.host_scales)
                self.targets[f"{li}.{tgt}"] = tb
            if hasattr(layer, "attn"):
                layer.attn.lora_bank = {
                    t: self.targets[f"{li}.{t}"] for t in ("qkv", "o")}
            if hasattr(layer, "mlp"):
                layer.mlp.lora_bank = {
                    t: self.targets[f"{li}.{t}"] for t in ("gate_up", "down")}

    def list(self) -> List[str]:
        return sorted(self.slot_of)

    def slot(self, name: str) -> int:
        return self.slot_of[name]

    def load(self, name: str, path: Optional[str] = None, rank: int = 8,
             alpha: float = 16.0, seed: int = 0) -> int:
        """Read the adapter and copy its block-form (A, B) of every target
        into a free slot (the slot it already has, when reloading a name)."""
        import os
        slot = self.slot_of.get(name)
        if slot is None:
            used = set(self.slot_of.values())
            free = [s for s in range(self.S) if s not in used]
            if not free:
                raise ValueError(
                    f"cannot load LoRA {name!r}: all {self.S} adapter slots "
                    f"(max_loras) are in use by {self.list()}")
            slot = free[0]
        if path and os.path.isdir(path) and os.path.exists(
                os.path.join(path, "adapter_config.json")):
            ad = load_peft_adapter(name, path, self.model)
        elif path:
            ad = LoRAAdapter.load(name, path, self.model, rank, alpha)
        else:
            ad = LoRAAdapter.random(name, self.model, rank, alpha, seed)
        # PEFT block forms (3r for qkv, 2r for gate/up) count against R
        for key, (A, _B) in ad.weights.items():
            if A.shape[0] > self.R:
                raise ValueError(
                    f"cannot load LoRA {name!r}: target {key} has rank "
                    f"{A.shape[0]} (fused block form), above max_lora_rank "
                    f"{self.R}")
        with torch.no_grad():
            # rank 0 first: a slot is never seen half-written with a rank
            self.ranks[:, :, slot] = 0
            host = torch.zeros(self.ranks.shape[:2], dtype=torch.int32)
            for key, tb in self.targets.items():
                # a target the adapter leaves out keeps rank 0
                w = ad.weights.get(key)
                r = 0 if w is None else int(w[0].shape[0])
                if r:
                    tb.A[slot, :r].copy_(w[0])
                    tb.B[slot, :, :r].copy_(w[1])
                tb.host_ranks[slot] = r
                li, tgt = key.split(".")
                host[int(li), TARGETS.index(tgt)] = r
            self.ranks[:, :, slot] = host.to(self.ranks.device)
            self.scales[slot] = ad.scale
        self.host_scales[slot] = float(ad.scale)
        self.slot_of[name] = slot
        log.info("loaded LoRA %s into bank slot %d (rank %d)", name, slot,
                 ad.rank)
        return slot

    def unload(self, name: str):
        slot = self.slot_of.pop(name, None)
        if slot is None:
            return
        with torch.no_grad():
            self.ranks[:, :, slot] = 0
        for tb in self.targets.values():
            tb.host_ranks[slot] = 0


def lora_block_salt(block_salt: int, lora: Optional[str]) -> int:
    """The prefix-cache block salt of a request: KV computed under an adapter
    is not the base model's, so the adapter's name is hashed in. Stable
    across processes (TP ranks must agree); base requests keep block_salt."""
    if not lora:
        return block_salt
    import hashlib
    h = int.from_bytes(
        hashlib.blake2b(lora.encode("utf-8"), digest_size=8).digest(),
        "little")
    return (block_salt ^ (h | 1)) & 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------
def load_peft_adapter(name: str, path: str, model) -> LoRAAdapter:
    """Load an HF PEFT-format adapter dir (adapter_config.json +
    adapter_model.safetensors) onto this build's FUSED projections.

    PEFT targets q/k/v (and gate/up) separately; the fused qkv/gate_up
    modules take a block form: A = stacked per-target A rows, B =
    block-diagonal per-target B columns — an exact rank-(sum r) adapter
    with y += scale * B(Ax) unchanged. TP: B rows follow each target's
    row shard (q by rank, k/v by the rank's kv-head window, gate/up by
    the I shard); input-side As of o_proj/down_proj are column-sliced to
    this rank's input shard (the row-parallel all-reduce sums the
    partial LoRA terms exactly like the base GEMM).
    """
    import json
    import os

    from safetensors import safe_open

    with open(os.path.join(path, "adapter_config.json")) as f:
        acfg = json.load(f)
    r = int(acfg.get("r", 8))
    alpha = float(acfg.get("lora_alpha", 16.0))
    sd = {}
    with safe_open(os.path.join(path, "adapter_model.safetensors"),
                   framework="pt") as f:
        for k in f.keys():
            sd[k.replace("base_model.model.", "")] = f.get_tensor(k)

    tp = model.tp
    cfg = model.cfg
    hd = cfg.head_dim
    kv_idx = (tp.rank if tp.size <= cfg.num_kv_heads
              else (tp.rank * cfg.num_kv_heads) // tp.size)

    def get(li: int, proj: str, mat: str):
        for stem in (f"model.layers.{li}.self_attn.{proj}",
                     f"model.layers.{li}.mlp.{proj}"):
            t = sd.get(f"{stem}.lora_{mat}.weight")
            if t is not None:
                return t.float()
        return None

    def fused(li: int, parts, row_slices, dev_w):
        """Block-form (A, B) over the present `parts`; row_slices gives
        each part's (row0, nrows) in the fused LOCAL weight."""
        present = [(p, sl) for p, sl in zip(parts, row_slices)
                   if get(li, p, "A") is not None]
        if not present:
            return None
        rt = r * len(present)
        in_f = dev_w.shape[-1]
        A = torch.zeros(rt, in_f)
        B = torch.zeros(dev_w.shape[0], rt)
        for j, (p, (row0, nrows, src0)) in enumerate(present):
            A[j * r:(j + 1) * r] = get(li, p, "A")
            Bp = get(li, p, "B")               # [full_out, r]
            B[row0:row0 + nrows, j * r:(j + 1) * r] = \
                Bp[src0:src0 + nrows]
        return (A.to(dev_w.device, dev_w.dtype),
                B.to(dev_w.device, dev_w.dtype))

    weights = {}
    for li, layer in enumerate(model.layers):
        if hasattr(layer, "attn"):
            at = layer.attn
            qr, kr = at.hq * hd, at.hkv * hd
            qkv = fused(li, ("q_proj", "k_proj", "v_proj"),
                        ((0, qr, tp.rank * qr),
                         (qr, kr, kv_idx * kr),
                         (qr + kr, kr, kv_idx * kr)), at.wqkv)
            if qkv is not None:
                weights[f"{li}.qkv"] = qkv
            Ao = get(li, "o_proj", "A")
            Bo = get(li, "o_proj", "B")
            if Ao is not None and Bo is not None:
                if tp.size > 1:
                    n = Ao.shape[1] // tp.size
                    Ao = Ao[:, tp.rank * n:(tp.rank + 1) * n]
                weights[f"{li}.o"] = (Ao.to(at.wo.device, at.wo.dtype),
                                      Bo.to(at.wo.device, at.wo.dtype))
        if hasattr(layer, "mlp"):
            mlp = layer.mlp
            gu = fused(li, ("gate_proj", "up_proj"),
                       ((0, mlp.I, tp.rank * mlp.I),
                        (mlp.I, mlp.I, tp.rank * mlp.I)), mlp.w_gate_up)
            if gu is not None:
                weights[f"{li}.gate_up"] = gu
            Ad = get(li, "down_proj", "A")
            Bd = get(li, "down_proj", "B")
            if Ad is not None and Bd is not None:
                if tp.size > 1:
                    n = Ad.shape[1] // tp.size
                    Ad = Ad[:, tp.rank * n:(tp.rank + 1) * n]
                weights[f"{li}.down"] = (
                    Ad.to(mlp.w_down.device, mlp.w_down.dtype),
                    Bd.to(mlp.w_down.device, mlp.w_down.dtype))
    # rank in the block form varies per module; scale uses the PEFT r
    ad = LoRAAdapter(name, r, alpha, weights)
    return ad
