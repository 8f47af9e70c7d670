"""Centralized environment-variable configuration.

Parity with the reference's centrally-named env config
(ai-dynamo/dynamo runtime/src/config/environment_names.rs, ~180 DYN_* vars;
we implement the subset that is meaningful in this build). Every CLI reads
its defaults from here.
"""
from __future__ import annotations

import os

ENV_VARS = {
    "DYN_DISCOVERY_BACKEND": "discovery backend spec: memory | file:/path",
    "DYN_NAMESPACE": "default namespace for components",
    "DYN_LOG": "log level (INFO, DEBUG, ...)",
    "DYN_LOGGING_JSONL": "1 = structured JSONL logs",
    "DYN_REQUEST_TRACE_FILE": "JSONL request-trace sink path",
    "DYN_HTTP_PORT": "frontend HTTP port",
    "DYN_ROUTER_MODE": "kv | round_robin | random | least_loaded | p2c",
    "DYN_ROUTER_TEMPERATURE": "softmax temperature for kv routing",
    "DYN_KV_BLOCK_SIZE": "KV page size in tokens",
    "DYN_KV_GPU_MEM_FRACTION": "fraction of free HBM for the KV pool",
    "DYN_HOST_CACHE_PAGES": "KVBM G2 pinned-host tier size (pages)",
    "DYN_TUNABLEOP": "0 disables the pre-tuned hipBLASLt table",
    "DYN_WORKER_TYPE": "aggregated | prefill | decode",
    "DYN_BYPASS_TOKEN_THRESHOLD":
        "conditional disagg: net-new prefill tokens below this bypass the "
        "prefill pool (reference conditional_disagg.rs:15; default 2048)",
    # kernel bring-up / A-B toggles (read by the HIP dispatch layer)
    "DYNAMO_DECODE_CHUNK": "decode attention context-chunk tokens override",
    "DYNAMO_DECODE_MFMA": "0 = force the VALU decode path (token-major only)",
    "DYNAMO_DECODE_SWAPPED": "0 = A-operand MFMA decode (token-major only)",
    "DYNAMO_DECODE_NT":
        "1 = non-temporal K/V loads in the d-major (VT4) decode attention "
        "kernel (bit-identical outputs; recorded-negative, slower)",
    "DYNAMO_FUSED_ROPE_ATTN":
        "0 = a decode step runs rope_append_qkv and decode attention as two "
        "kernels (default: on bf16 d-major V pages the d-major decode kernel "
        "ropes q and appends the new token's k / v itself where "
        "ops.fused_rope_attn_ready allows; equal bits either way)",
    "DYNAMO_SKINNY_GEMM":
        "0 = every decode weight GEMM on hipBLASLt (default: the in-tree "
        "skinny-M kernel on the shapes in ops.SKINNY_GEMM_SHAPES)",
    "DYNAMO_FUSED_GLU":
        "0 = gate/up GEMM and silu_mul as two kernels (default: the in-tree "
        "GEMM applies SwiGLU in its epilogue where ops.fused_glu_config "
        "allows; equal bits either way)",
    "DYNAMO_QUANT_TILE_GEMM":
        "1 = fp8 / mxfp4 projection GEMMs above the skinny-M kernel's M run "
        "on the tiled W8A16 / W4A16 kernel (csrc/quant_tile_gemm.hip, x "
        "staged in LDS) up to ops.TILE_GEMM_MAX_M instead of dequantising "
        "the weight for the library GEMM. Default: off",
    "DYNAMO_MX_GEMM":
        "1 = fp8 / mxfp4 projection GEMMs at M >= ops.MX_GEMM_MIN_M (prefill "
        "steps) quantise the activations to MXFP8 rows (e4m3, one e8m0 scale "
        "per 32 k) and run on the block-scaled fp8/fp4 MFMA kernel "
        "(csrc/mx_gemm.hip) instead of dequantising the weight for the bf16 "
        "library GEMM. Changes the numbers: W8A8 / W4A8 above that M. "
        "Default: off",
    "DYNAMO_MQ_ATTN":
        "1 = a step whose prefill part is runs of at most ops.MQ_MAX_Q query "
        "tokens per sequence (q_len * G <= ops.MQ_MAX_COLS, d-major V pages, "
        "head_dim 128) attends through the split-KV multi-query kernel "
        "(csrc/attention_multiquery.hip) instead of the prefill kernel. "
        "Default: off",
    "DYNAMO_SHARED_PREFIX_ATTN":
        "1 = decode rows whose page tables begin with the same pages (a "
        "prefix-cache hit on a common prompt, at least one decode chunk "
        "long) attend through the shared-prefix kernel "
        "(csrc/attention_shared_prefix.hip), which streams the common pages "
        "once per group of up to 64 / G rows; a step without such a group "
        "runs the decode kernel as before (d-major V pages, head_dim 128). "
        "Default: off",
    "DYNAMO_LOGPROBS_KERNEL":
        "1 = requests with logprobs (at most ops.LOGPROBS_MAX_N per token) "
        "get them from the fused kernel (csrc/logprobs.hip: one pass over "
        "the fp32 logits row, no [B, V] temporary, lowest id first among "
        "equal logits) instead of torch log_softmax + topk + gather. Values "
        "differ from the torch path by fp32 rounding. Default: off",
    "DYNAMO_MAX_LORAS":
        "default of the worker's --max-loras: adapter-bank slots for "
        "per-request LoRA (default 0 = engine-level activation only)",
    "DYNAMO_MAX_LORA_RANK":
        "default of the worker's --max-lora-rank: the largest (fused block "
        "form) adapter rank a bank slot holds, a multiple of 8 (default 64)",
    "DYNAMO_WEIGHT_DTYPE":
        "what EngineConfig.weight_dtype=\"auto\" resolves to: bf16 (default; "
        "the compute dtype, unquantised) | fp8 (e4m3 projection weights, "
        "W8A16) | mxfp4 (OCP microscaling FP4 projection weights: e2m1 codes "
        "with one e8m0 scale per 32 k, W4A16)",
    "DYNAMO_MOE_BMM": "0 = grouped-kernel MoE decode instead of padded bmm",
    "DYNAMO_MOE_FUSED":
        "1 = routed MoE decode for T <= 64 (csrc/moe_decode.hip: route, "
        "expert-grouped gate/up GEMM with SwiGLU, weighted down GEMM, "
        "combine; idle experts' weights are not read). Default: the padded "
        "bmm route",
    "DYNAMO_MOE_TILED":
        "1 = fp8 / mxfp4 Mixtral experts above the routed decode kernels' 64 "
        "tokens, up to ops.MOE_TILE_MAX_T, run the routed tiled kernels "
        "(csrc/moe_tile_gemm.hip: device-side route with a tile map, "
        "expert-grouped tiled gate/up GEMM with SwiGLU, weighted down GEMM, "
        "combine; no host read, hipGraph-safe) instead of the host-side "
        "expert loop. Default: off",
    "DYNAMO_MOE_MFMA": "0 = VALU grouped MoE GEMM",
    "DYNAMO_MOE_GRAPHS": "0 = exclude MoE layers from hipGraph capture",
    "DYNAMO_ROCTX": "1 = roctx range annotations for rocprofv3 traces",
}


def get(name: str, default=None, cast=str):
    v = os.environ.get(name)
    if v is None:
        return default
    try:
        if cast is bool:
            return v not in ("0", "false", "False", "")
        return cast(v)
    except (TypeError, ValueError):
        return default


def discovery(default="memory"):
    return get("DYN_DISCOVERY_BACKEND", default)


def namespace(default="dynamo"):
    return get("DYN_NAMESPACE", default)
