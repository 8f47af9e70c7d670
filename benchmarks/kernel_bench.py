"""Microbenchmarks for the native kernels (run on an MI355X box).

Prints per-kernel achieved bandwidth / TFLOPs vs the hardware ceilings
(HBM ~6.3 TB/s achievable, bf16 MFMA 2.5 PF dense)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dynamo_amd import ops  # noqa: E402


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.monotonic()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.monotonic() - t0) / iters


def bench_rmsnorm(rows=8192, D=8192):
    x = torch.randn(rows, D, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(D, dtype=torch.bfloat16, device="cuda")
    t = timeit(lambda: ops.rmsnorm(x, w, 1e-5))
    gb = 2 * rows * D * 2 / 1e9
    print(f"rmsnorm      [{rows}x{D}]: {t*1e6:8.1f} us  {gb/t:7.2f} GB/s")


def bench_silu_mul(rows=8192, I=14336):
    x = torch.randn(rows, 2 * I, dtype=torch.bfloat16, device="cuda")
    t = timeit(lambda: ops.silu_mul(x))
    gb = 3 * rows * I * 2 / 1e9
    print(f"silu_mul     [{rows}x{I}]: {t*1e6:8.1f} us  {gb/t:7.2f} GB/s")


def bench_decode_attn(B=16, ctx=8192, Hq=64, Hkv=8, ps=64):
    hd = 128
    npages = B * ((ctx + ps - 1) // ps)
    kc = torch.randn(npages, Hkv, ps, hd, dtype=torch.bfloat16, device="cuda")
    vc = torch.randn_like(kc)
    pt = torch.arange(npages, dtype=torch.int32, device="cuda").view(B, -1)
    q = torch.randn(B, Hq, hd, dtype=torch.bfloat16, device="cuda")
    ctxl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    scratch = ops.DecodeScratch(B, Hq, hd, ctx, "cuda")
    t = timeit(lambda: ops.paged_attention_decode(
        q, kc, vc, pt, ctxl, hd ** -0.5, scratch))
    vct = vc.permute(0, 1, 3, 2).contiguous()
    tv = timeit(lambda: ops.paged_attention_decode(
        q, kc, vct, pt, ctxl, hd ** -0.5, scratch, v_transposed=True))
    gb = 2 * B * ctx * Hkv * hd * 2 / 1e9  # K+V bytes
    print(f"decode_attn  [B{B} ctx{ctx} Hq{Hq}/{Hkv}]: {t*1e6:8.1f} us  "
          f"{gb/t:7.2f} GB/s | vt {tv*1e6:8.1f} us {gb/tv:7.2f} GB/s")
    # K/V cache policy of the d-major kernel (DYNAMO_DECODE_NT), alternated.
    # K + V of one layer (537 MB at the flagship shape) exceed the Infinity
    # Cache, so this replay loop is already cache-cold for them.
    ts = {0: [], 1: []}
    for _ in range(3):
        for nt in (0, 1):
            ts[nt].append(timeit(lambda: ops.paged_attention_decode(
                q, kc, vct, pt, ctxl, hd ** -0.5, scratch, v_transposed=True,
                nt_policy=nt)))
    d, n = min(ts[0]), min(ts[1])
    print(f"  vt K/V policy: default {d*1e6:8.1f} us {gb/d:7.2f} GB/s | "
          f"nt {n*1e6:8.1f} us {gb/n:7.2f} GB/s")


def bench_prefill_attn(S=8192, Hq=32, Hkv=8, ps=64, v_transposed=False):
    hd = 128
    npages = (S + ps - 1) // ps
    kc = torch.randn(npages, Hkv, ps, hd, dtype=torch.bfloat16, device="cuda")
    vc = torch.randn_like(kc)
    pt = torch.arange(npages, dtype=torch.int32, device="cuda").view(1, -1)
    q = torch.randn(S, Hq, hd, dtype=torch.bfloat16, device="cuda")
    starts = torch.tensor([0], dtype=torch.int32, device="cuda")
    qlen = torch.tensor([S], dtype=torch.int32, device="cuda")
    ctxl = torch.tensor([S], dtype=torch.int32, device="cuda")
    tiles = ops.build_prefill_tiles([S], "cuda",
                                    ops.prefill_tile_rows(Hq, Hkv))
    if v_transposed:
        vc = vc.permute(0, 1, 3, 2).contiguous()
    t = timeit(lambda: ops.attention_prefill_paged(
        q, kc, vc, pt, starts, qlen, ctxl, hd ** -0.5, tiles,
        v_transposed=v_transposed), iters=5)
    # causal flops: 2 gemms * 2*S*S/2*hd per head
    fl = 2 * 2 * Hq * (S * S / 2) * hd
    print(f"prefill_attn [S{S} Hq{Hq}/{Hkv} vt{int(v_transposed)}]: "
          f"{t*1e3:8.2f} ms  {fl/t/1e12:7.1f} TFLOP/s (causal)")


def bench_kv_append(T=8192, Hkv=8, ps=64):
    hd = 128
    npages = (T + ps - 1) // ps
    kc = torch.zeros(npages, Hkv, ps, hd, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    k = torch.randn(T, Hkv, hd, dtype=torch.bfloat16, device="cuda")
    v = torch.randn_like(k)
    slots = torch.arange(T, dtype=torch.int64, device="cuda")
    t = timeit(lambda: ops.kv_cache_append(kc, vc, k, v, slots))
    gb = 4 * T * Hkv * hd * 2 / 1e9
    print(f"kv_append    [T{T}]: {t*1e6:8.1f} us  {gb/t:7.2f} GB/s")


def bench_sampling(B=16, V=128256):
    logits = torch.randn(B, V, device="cuda")
    t = timeit(lambda: ops.greedy_sample(logits))
    print(f"greedy       [B{B} V{V}]: {t*1e6:8.1f} us")
    # the filtered sampler with every row on the same filter, on N(0, 1)
    # logits and on the nearly flat rows of the benchmark model (sigma 0.01);
    # min of three, alternated, like every comparison in this file
    inv_t = torch.ones(B, device="cuda")
    modes = (("k only", 50, 1.0), ("p only", 0, 0.9), ("k and p", 50, 0.9))
    for name, rows in (("randn", logits), ("flat", logits * 0.01)):
        ts = {m[0]: [] for m in modes}
        for _ in range(3):
            for mode, k, p in modes:
                tk = torch.full((B,), k, dtype=torch.int32, device="cuda")
                tp = torch.full((B,), p, dtype=torch.float32, device="cuda")
                ts[mode].append(timeit(
                    lambda: ops.topkp_sample(rows, inv_t, tk, tp, 1234)))
        row = " | ".join(f"{m} {min(v)*1e6:7.1f} us" for m, v in ts.items())
        print(f"topkp_sample [B{B} V{V}] {name:5s}: {row}")


def timeit_graph(fn, n=100, reps=20):
    """Per-call time of a latency-bound kernel as the decode graph runs it:
    n dependent calls captured into one hipGraph, so the figure is kernel +
    dependent-kernel boundary without the eager host launch cost."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    t0 = time.monotonic()
    for _ in range(reps):
        g.replay()
    torch.cuda.synchronize()
    return (time.monotonic() - t0) / (reps * n)


def _fast_vs_general(name, fn):
    """fn(allow_fast) -> one call; prints general | fast, alternated."""
    ts = {False: [], True: []}
    for _ in range(3):
        for fast in (False, True):
            ts[fast].append(timeit_graph(lambda: fn(fast)))
    g, f = min(ts[False]), min(ts[True])
    print(f"{name}: general {g*1e6:7.2f} us | fast {f*1e6:7.2f} us "
          f"({g/f:4.2f}x)")


def bench_rmsnorm_decode(rows=16, D=8192):
    x = torch.randn(rows, D, dtype=torch.bfloat16, device="cuda")
    res = torch.zeros(rows, D, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(D, dtype=torch.bfloat16, device="cuda")
    _fast_vs_general(f"fused_add_rmsnorm [{rows}x{D}]",
                     lambda fast: ops.fused_add_rmsnorm(x, res, w, 1e-5, fast))
    _fast_vs_general(f"rmsnorm           [{rows}x{D}]",
                     lambda fast: ops.rmsnorm(x, w, 1e-5, fast))


def bench_rope_append(T=16, Hq=64, Hkv=8, ps=64):
    hd = 128
    npages = (T + ps - 1) // ps
    qkv = torch.randn(T, (Hq + 2 * Hkv) * hd, dtype=torch.bfloat16,
                      device="cuda")
    kc = torch.zeros(npages, Hkv, ps, hd, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros(npages, Hkv, hd, ps, dtype=torch.bfloat16, device="cuda")
    pos = torch.arange(T, dtype=torch.int32, device="cuda")
    slots = torch.arange(T, dtype=torch.int64, device="cuda")
    cs = ops.make_cos_sin_cache(max(T, 64), hd, 10000.0, device="cuda")
    q_out = torch.empty(T, Hq * hd, dtype=torch.bfloat16, device="cuda")
    _fast_vs_general(
        f"rope_append  [T{T} Hq{Hq}/{Hkv} vt1]",
        lambda fast: ops.hip().rope_append_qkv(q_out, kc, vc, qkv, None, pos,
                                               slots, cs, True, fast))


def bench_sampling_decode(B=16, V=128256):
    logits = torch.randn(B, V, device="cuda")
    out = torch.empty(B, dtype=torch.int32, device="cuda")
    _fast_vs_general(f"greedy       [B{B} V{V}]",
                     lambda fast: ops.hip().greedy_sample(out, logits, fast))


def bench_logit_processors(B=16, V=128256):
    """logits_process with every row penalised, as the decode graph's
    neighbour runs it (timeit_graph), against the 12 B per vocabulary entry
    of its contract (logits read + write, counts read), and the greedy
    kernel (4 B per entry) at the same shape as the yardstick. `sparse`: each
    row has seen 2048 prompt and 512 output tokens, so most 16-byte logits
    vectors are not written back; `dense`: every token seen, every vector
    written; `+min_p` adds the max and mask passes over the row."""
    logits = torch.randn(B, V, device="cuda")
    slots = torch.arange(B, dtype=torch.int32, device="cuda")
    sparse = torch.zeros(B, V, dtype=torch.int32, device="cuda")
    for b in range(B):
        sparse[b, torch.randint(0, V, (2048,), device="cuda")] = 1
        sparse[b, torch.randint(0, V, (512,), device="cuda")] += 2
    dense = torch.full((B, V), 3, dtype=torch.int32, device="cuda")
    gb = B * V * 12 / 1e9
    for name, bank, p in (("sparse", sparse, (1.1, 0.1, 0.1, 0.0, 1.0)),
                          ("dense", dense, (1.1, 0.1, 0.1, 0.0, 1.0)),
                          ("dense+min_p", dense, (1.1, 0.1, 0.1, 0.05, 1.0))):
        params = torch.tensor([p] * B, dtype=torch.float32, device="cuda")
        ts = {False: [], True: []}
        for _ in range(3):
            for fast in (False, True):
                work = logits.clone()
                ts[fast].append(timeit_graph(
                    lambda: ops.hip().logits_process(
                        work, bank, slots, params, None, None, None, fast)))
        g, f = min(ts[False]), min(ts[True])
        print(f"logits_process [B{B} V{V}] {name:12s}: scalar {g*1e6:7.2f} us "
              f"| vector {f*1e6:7.2f} us  {gb/f:7.1f} GB/s of 12 B/entry")
    out = torch.empty(B, dtype=torch.int32, device="cuda")
    t = min(timeit_graph(lambda: ops.hip().greedy_sample(out, logits, True))
            for _ in range(3))
    print(f"greedy         [B{B} V{V}]             : vector {t*1e6:7.2f} us  "
          f"{B * V * 4 / 1e9 / t:7.1f} GB/s of 4 B/entry")


def bench_gemm(M=16, K=8192, N=8192):
    a = torch.randn(M, K, dtype=torch.bfloat16, device="cuda")
    w = torch.randn(N, K, dtype=torch.bfloat16, device="cuda")
    t = timeit(lambda: torch.nn.functional.linear(a, w))
    fl = 2 * M * N * K
    gb = (M * K + N * K + M * N) * 2 / 1e9
    print(f"gemm(blaslt) [{M}x{K}x{N}]: {t*1e6:8.1f} us  {fl/t/1e12:7.1f} TF  "
          f"{gb/t:7.2f} GB/s")


def bench_skinny_gemm(M=16, sweep=False, mxfp4_sweep=False):
    """Decode weight GEMMs at the flagship shapes, cache-cold: launch i reads
    copy i % R of W, R * bytes(W) >= 1 GiB (the step never re-reads a matrix
    before 137 GB of other weights have passed). hipBLASLt under the
    project's TunableOp table vs the in-tree kernel at the shape's shipped
    configuration (row-coalesced WPB8/U1/NT2 where the shape is not shipped),
    with non-temporal and with default-policy W loads; then the W8A16 kernel
    on e4m3 copies of the same matrices (`sweep`: at every configuration) and
    the W4A16 kernel on MXFP4 copies (`mxfp4_sweep`: at every
    configuration)."""
    from dynamo_amd.utils import enable_tunableop
    enable_tunableop(tuning=False)
    x_by_k = {}
    for name, N, K in (("qkv", 10240, 8192), ("o", 8192, 8192),
                       ("gateup", 57344, 8192), ("down", 8192, 28672),
                       ("lm_head", 128256, 8192)):
        x = x_by_k.setdefault(K, torch.randn(M, K, dtype=torch.bfloat16,
                                             device="cuda"))
        wbytes = N * K * 2
        R = max(2, -(-(1 << 30) // wbytes))
        ws = [torch.randn(N, K, dtype=torch.bfloat16, device="cuda") * 0.02
              for _ in range(R)]
        y = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        cfg = ops.SKINNY_GEMM_SHAPES.get((N, K), (8, 1, 2, True, True))
        i = [0]

        def lib():
            i[0] += 1
            return torch.nn.functional.linear(x, ws[i[0] % R])

        def ours(nontemporal=True):
            i[0] += 1
            ops.hip().skinny_gemm(y, x, ws[i[0] % R], *cfg[:3], nontemporal,
                                  cfg[4])

        # the in-tree bf16 kernel stops at M = 16
        ts = {"lib": [], "nt": [], "dflt": []} if M <= 16 else {"lib": []}
        for _ in range(3):
            ts["lib"].append(timeit(lib, iters=24))
            if M <= 16:
                ts["nt"].append(timeit(ours, iters=24))
                ts["dflt"].append(timeit(lambda: ours(False), iters=24))
        gb = wbytes / 1e9
        row = " | ".join(f"{k} {min(v)*1e6:7.1f} us {gb/min(v)/1e3:5.2f} TB/s"
                         for k, v in ts.items())
        shipped = "shipped" if (N, K) in ops.SKINNY_GEMM_SHAPES else "library"
        print(f"gemm cold {name:8s}[{M}x{K}x{N}] R={R} w{cfg[0]}u{cfg[1]}"
              f"n{cfg[2]} ({shipped}): {row}")
        t_bf16 = min(ts["lib"] if shipped == "library" or M > 16
                     else ts["nt"])
        if name == "gateup" and M <= 16 and cfg[4]:
            _bench_fused_glu(
                f"{name:8s}[{M}x{K}x{N}] R={R} w{cfg[0]}u{cfg[1]}n{cfg[2]}",
                "bf16_coalesced", cfg, y, lambda out, r, glu:
                ops.hip().skinny_gemm(out, x, ws[r % R], *cfg, glu))
        _bench_fp8_gemm(name, x, ws, y, t_bf16, sweep)
        if name != "lm_head":       # not quantised by weight_dtype="mxfp4"
            _bench_mxfp4_gemm(name, x, ws, y, t_bf16, mxfp4_sweep)
        del ws


def _bench_fp8_gemm(name, x, ws, y, t_bf16, sweep):
    """The W8A16 kernel on the same shape, cache-cold the same way (R8
    copies of the e4m3 matrix, R8 * bytes >= 1 GiB); bytes/s are of W.
    `t_bf16` is the time of the current bf16 dispatch for the shape. With
    `sweep`, every launchable configuration instead of the dispatch's."""
    M, K = x.shape
    N = ws[0].shape[0]
    wbytes = N * K
    R8 = max(2, -(-(1 << 30) // wbytes))
    qs, scale = [], None
    for r in range(R8):
        q, scale = ops.quantize_fp8_rowwise(ws[r % len(ws)])
        qs.append(q)
    i = [0]
    cfgs = (ops.FP8_GEMM_CONFIGS if sweep
            else (ops.fp8_gemm_config(M, N, K),))
    for cfg in cfgs:
        if K % (cfg[0] * 128 * cfg[1]):
            continue

        def fp8():
            i[0] += 1
            ops.hip().fp8_skinny_gemm(y, x, qs[i[0] % R8], scale, *cfg)

        t = min(timeit(fp8, iters=24) for _ in range(3))
        print(f"gemm cold {name:8s}[{M}x{K}x{N}] R={R8} fp8 w{cfg[0]}u{cfg[1]}"
              f"n{cfg[2]}: {t*1e6:7.1f} us {wbytes/1e9/t/1e3:5.2f} TB/s "
              f"({t_bf16/t:4.2f}x the bf16 dispatch)")
        if name == "gateup" and not sweep:
            _bench_fused_glu(
                f"{name:8s}[{M}x{K}x{N}] R={R8} fp8 w{cfg[0]}u{cfg[1]}"
                f"n{cfg[2]}", "fp8", cfg, y, lambda out, r, glu, cfg=cfg:
                ops.hip().fp8_skinny_gemm(out, x, qs[r % R8], scale, *cfg,
                                          True, glu))


def _bench_mxfp4_gemm(name, x, ws, y, t_bf16, sweep):
    """The W4A16 kernel on the same shape, cache-cold the same way (R4
    copies of the packed matrix and its scales, R4 * bytes >= 1 GiB);
    bytes/s are of W, scales included. M above the kernel's limit prints
    nothing."""
    M, K = x.shape
    N = ws[0].shape[0]
    if M > ops.MXFP4_GEMM_MAX_M:
        return
    wbytes = N * K // 2 + N * K // 32
    R4 = max(2, -(-(1 << 30) // wbytes))
    first = [ops.quantize_mxfp4(w) for w in ws[:R4]]
    qs = [first[r] if r < len(first) else
          tuple(t.clone() for t in first[r % len(first)]) for r in range(R4)]
    i = [0]
    cfgs = (ops.MXFP4_GEMM_CONFIGS if sweep
            else (ops.mxfp4_gemm_config(M, N, K),))
    for cfg in cfgs:
        if K % (cfg[0] * 256 * cfg[1]):
            continue

        def mxfp4():
            i[0] += 1
            ops.hip().mxfp4_skinny_gemm(y, x, *qs[i[0] % R4], *cfg)

        t = min(timeit(mxfp4, iters=24) for _ in range(3))
        print(f"gemm cold {name:8s}[{M}x{K}x{N}] R={R4} mxfp4 w{cfg[0]}"
              f"u{cfg[1]}n{cfg[2]}: {t*1e6:7.1f} us "
              f"{wbytes/1e9/t/1e3:5.2f} TB/s "
              f"({t_bf16/t:4.2f}x the bf16 dispatch)")
        if name == "gateup" and not sweep:
            _bench_fused_glu(
                f"{name:8s}[{M}x{K}x{N}] R={R4} mxfp4 w{cfg[0]}u{cfg[1]}"
                f"n{cfg[2]}", "mxfp4", cfg, y, lambda out, r, glu, cfg=cfg:
                ops.hip().mxfp4_skinny_gemm(out, x, *qs[r % R4], *cfg, True,
                                            glu))


def _bench_fused_glu(label, fmt, cfg, y, gemm):
    """The gate/up GEMM with the SwiGLU epilogue against the unfused GEMM
    followed by silu_mul, both cache-cold the same way: gemm(out, r, glu)
    launches the format's kernel on weight copy r into out."""
    if not ops.glu_capable(fmt, cfg):
        print(f"gemm cold {label}: no fused SwiGLU form")
        return
    M, N = y.shape
    act = torch.empty(M, N // 2, dtype=y.dtype, device=y.device)
    i = [0]

    def fused():
        i[0] += 1
        gemm(act, i[0], True)

    def two():
        i[0] += 1
        gemm(y, i[0], False)
        ops.hip().silu_mul(act, y)

    def plain():
        i[0] += 1
        gemm(y, i[0], False)

    tf, t2, tp = ([], [], [])
    for _ in range(3):
        tf.append(timeit(fused, iters=24))
        t2.append(timeit(two, iters=24))
        tp.append(timeit(plain, iters=24))
    ts = min(timeit(lambda: ops.hip().silu_mul(act, y), iters=24)
             for _ in range(3))
    print(f"gemm cold {label} +silu_mul: fused {min(tf)*1e6:7.1f} us | "
          f"gemm, then silu_mul {min(t2)*1e6:7.1f} us (gemm {min(tp)*1e6:7.1f}"
          f" + silu_mul alone, hot {ts*1e6:5.1f})")


def bench_lora(T=16, R=64):
    """The gathered LoRA kernel pair (csrc/lora.hip) at the four llama-3-70b
    projection shapes, cache-cold: launch i reads copy i % C of a 16-slot
    bank, C * bytes(bank) >= 1 GiB. Rank 16 and rank 64 in R = 64 slots, with
    1, 4 and 16 distinct adapters among the T rows. GB/s are of the bytes
    that must move: distinct adapters * rank * (K + N) * 2 B."""
    S = 16
    for name, N, K in (("qkv", 10240, 8192), ("o", 8192, 8192),
                       ("gateup", 57344, 8192), ("down", 8192, 28672)):
        bank_bytes = S * R * (K + N) * 2
        C = max(2, -(-(1 << 30) // bank_bytes))
        As = [torch.randn(S, R, K, dtype=torch.bfloat16, device="cuda") * 0.02
              for _ in range(C)]
        Bs = [torch.randn(S, N, R, dtype=torch.bfloat16, device="cuda") * 0.02
              for _ in range(C)]
        x = torch.randn(T, K, dtype=torch.bfloat16, device="cuda")
        y = torch.randn(T, N, dtype=torch.bfloat16, device="cuda")
        t = torch.empty(T, R, dtype=torch.float32, device="cuda")
        scales = torch.ones(S, device="cuda")
        for rank in (16, 64):
            ranks = torch.full((S,), rank, dtype=torch.int32, device="cuda")
            for distinct in (1, 4, 16):
                slots = (torch.arange(T, device="cuda") % distinct).to(
                    torch.int32)
                i = [0]

                def shrink():
                    i[0] += 1
                    ops.lora_shrink(t, x, As[i[0] % C], slots, ranks)

                def expand():
                    i[0] += 1
                    ops.lora_expand_add(y, t, Bs[i[0] % C], slots, ranks,
                                        scales)

                def both():
                    shrink()
                    expand()

                ts = [min(timeit(f, iters=24) for _ in range(3))
                      for f in (shrink, expand, both)]
                gbs = [distinct * rank * n * 2 / 1e9 for n in (K, N, K + N)]
                row = " | ".join(
                    f"{k} {tt*1e6:6.1f} us {gb/tt:6.0f} GB/s"
                    for k, tt, gb in zip(("shrink", "expand", "pair"), ts,
                                         gbs))
                print(f"lora cold {name:7s}[{T}x{K}x{N}] C={C} rank {rank:2d} "
                      f"adapters {distinct:2d}: {row}")
        del As, Bs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="all")
    a = ap.parse_args()
    torch.manual_seed(0)
    w = a.which
    if w in ("all", "rmsnorm"):
        bench_rmsnorm()
    if w in ("all", "silu"):
        bench_silu_mul()
    if w in ("all", "decode"):
        bench_decode_attn()
        bench_decode_attn(B=16, ctx=8192, Hq=32, Hkv=8)
    if w in ("all", "prefill"):
        bench_prefill_attn()
        bench_prefill_attn(v_transposed=True)
        bench_prefill_attn(S=8192, Hq=64)
        bench_prefill_attn(S=8192, Hq=64, v_transposed=True)
        bench_prefill_attn(S=2048)
        bench_prefill_attn(Hq=64)          # GQA 8 (llama-70b TP1)
        bench_prefill_attn(S=2048, Hq=64)
    if w in ("all", "append"):
        bench_kv_append()
    if w in ("all", "sample"):
        bench_sampling()
    if w in ("all", "tail"):
        # the decode step's latency-bound kernels at the flagship shapes,
        # plus rope-append at the prefill shape
        bench_rmsnorm_decode()
        bench_rope_append()
        bench_rope_append(T=8192)
        bench_sampling_decode()
    if w in ("all", "logits"):
        bench_logit_processors(B=16)
        bench_logit_processors(B=64)
    if w in ("all", "gemm"):
        bench_gemm()
        bench_gemm(M=8192)
        bench_skinny_gemm()
        bench_skinny_gemm(M=64)
    if w in ("all", "lora"):
        bench_lora()
    if w == "fp8sweep":
        # every launchable W8A16 configuration per shape: picks
        # ops.FP8_GEMM_SHAPES
        bench_skinny_gemm(sweep=True)
        bench_skinny_gemm(M=64, sweep=True)
    if w == "mxfp4sweep":
        # every launchable W4A16 configuration per shape, next to the bf16
        # and fp8 dispatches: picks ops.MXFP4_GEMM_SHAPES
        bench_skinny_gemm(mxfp4_sweep=True)
        bench_skinny_gemm(M=ops.MXFP4_GEMM_MAX_M, mxfp4_sweep=True)
