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


def bench_mq_attn(S=16, Hkv=8, G=8, ps=64, ctxs=(8192, 2048),
                  q_lens=(2, 4, 8), rounds=3, window=0.2):
    """Short query runs on long contexts: ops.paged_attention_multiquery
    against ops.attention_prefill_paged on the same inputs, and the
    single-token decode kernel at the same context as the bandwidth
    yardstick. Cache-cold: call i reads copy i % R of the K/V caches, R
    copies together past 640 MB (the Infinity Cache holds 256 MB). Device
    events around >= `window` s of back-to-back eager calls, the three
    alternated `rounds` times, best of the rounds. The multi-query figure is
    the whole op: row_ctx construction, phase 1 and the chunk merge."""
    hd, Hq, dev = 128, Hkv * G, "cuda"
    scale = hd ** -0.5

    def event_time(fn, n):
        start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        start.record()
        for i in range(n):
            fn(i)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e-3 / n

    for fp8 in (False, True):
        for ctx in ctxs:
            ppseq = (ctx + ps - 1) // ps
            kv_bytes = 2 * S * ctx * Hkv * hd * (1 if fp8 else 2)
            R = max(1, -(-640_000_000 // kv_bytes))
            store = torch.float8_e4m3fn if fp8 else torch.bfloat16
            caches = []
            for _ in range(R):
                k = torch.randn(S * ppseq, Hkv, ps, hd, dtype=torch.bfloat16,
                                device=dev)
                v = torch.randn(S * ppseq, Hkv, hd, ps, dtype=torch.bfloat16,
                                device=dev)
                caches.append((k.to(store), v.to(store)))
            pt = torch.arange(S * ppseq, dtype=torch.int32,
                              device=dev).view(S, -1)
            ctxl = torch.full((S,), ctx, dtype=torch.int32, device=dev)
            dscratch = ops.DecodeScratch(S, Hq, hd, ctx, dev)
            q1 = torch.randn(S, Hq, hd, dtype=torch.bfloat16, device=dev)

            def decode(i):
                kc, vc = caches[i % R]
                ops.paged_attention_decode(q1, kc, vc, pt, ctxl, scale,
                                           dscratch, v_transposed=True)

            for ql in q_lens:
                q = torch.randn(S * ql, Hq, hd, dtype=torch.bfloat16,
                                device=dev)
                starts = torch.arange(0, S * ql, ql, dtype=torch.int32,
                                      device=dev)
                qlen = torch.full((S,), ql, dtype=torch.int32, device=dev)
                tiles = ops.build_prefill_tiles(
                    [ql] * S, dev, ops.prefill_tile_rows(Hq, Hkv))
                scratch = ops.MultiQueryScratch(S * ql, Hq, hd, ctx, dev)

                def mq(i):
                    kc, vc = caches[i % R]
                    return ops.paged_attention_multiquery(
                        q, kc, vc, pt, starts, qlen, ctxl, scale, scratch, ql)

                def prefill(i):
                    kc, vc = caches[i % R]
                    return ops.attention_prefill_paged(
                        q, kc, vc, pt, starts, qlen, ctxl, scale, tiles,
                        v_transposed=True)

                diff = float((mq(0).float() - prefill(0).float()).abs().max())
                fns = {"mq": mq, "prefill": prefill, "decode": decode}
                n = {}
                for name, fn in fns.items():
                    event_time(fn, 2 * R)                       # warm-up
                    n[name] = max(2 * R, int(window / event_time(fn, 2 * R)))
                ts = {name: [] for name in fns}
                for _ in range(rounds):
                    for name, fn in fns.items():
                        ts[name].append(event_time(fn, n[name]))
                t = {name: min(v) for name, v in ts.items()}
                gb = kv_bytes / 1e9
                print(f"mq_attn {'fp8 ' if fp8 else 'bf16'} S{S} Hq{Hq}/{Hkv} "
                      f"ctx{ctx} q{ql} R={R}: mq {t['mq']*1e6:7.1f} us "
                      f"{gb/t['mq']:5.0f} GB/s | prefill "
                      f"{t['prefill']*1e6:7.1f} us | decode(q1) "
                      f"{t['decode']*1e6:7.1f} us {gb/t['decode']:5.0f} GB/s | "
                      f"prefill/mq {t['prefill']/t['mq']:5.2f}x | mq/decode "
                      f"{t['mq']/t['decode']:4.2f}x | max |mq - prefill| "
                      f"{diff:.1e}", flush=True)
            del caches


def bench_shared_prefix(Hkv=8, G=8, ps=64, ctx=8192,
                        shapes=((16, 1), (64, 4)),
                        shared_lens=(2048, 4096, 6144), rounds=3, window=0.2):
    """Decode rows that share leading pages: ops.paged_attention_decode_shared
    (plan built once on the host, as the graph runner does; phase 1 and the
    chunk merge timed) against ops.paged_attention_decode on the same
    tensors, i.e. the same page table with the groups' common page ids.
    `shapes` is (batch, groups): each group's rows share `shared` tokens and
    own the rest of their ctx. Cache-cold: call i reads copy i % R of the K/V
    caches, R copies together past 640 MB of distinct pages (the Infinity
    Cache holds 256 MB). Device events around >= `window` s of back-to-back
    eager calls, the two alternated `rounds` times, best of the rounds.
    `streamed` is what each kernel's blocks load of K and V: batch * ctx
    tokens for the decode kernel, the plan's item ranges for the shared one."""
    hd, Hq, dev = 128, Hkv * G, "cuda"
    scale = hd ** -0.5

    def event_time(fn, n):
        start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        start.record()
        for i in range(n):
            fn(i)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e-3 / n

    for fp8 in (False, True):
        store = torch.float8_e4m3fn if fp8 else torch.bfloat16
        tok_bytes = 2 * Hkv * hd * (1 if fp8 else 2)        # K + V
        for B, groups in shapes:
            scratch = ops.DecodeScratch(B, Hq, hd, ctx, dev)
            chunk = scratch.chunk_tokens
            q = torch.randn(B, Hq, hd, dtype=torch.bfloat16, device=dev)
            ctxl = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            for shared in shared_lens:
                per, sp, tp = B // groups, shared // ps, (ctx - shared) // ps
                pages, nxt = [], 0
                for g in range(groups):
                    common = list(range(nxt, nxt + sp))
                    nxt += sp
                    for _ in range(per):
                        pages.append(common + list(range(nxt, nxt + tp)))
                        nxt += tp
                plan = ops.shared_prefix_plan(pages, [ctx] * B, chunk, ps, G,
                                              B + B // 2)
                item_tokens = sum(
                    (ctx if t1 < 0 else t1) - t0
                    for (t0, t1), r0 in zip(plan[1].tolist(),
                                            plan[0][:, 0].tolist()) if r0 >= 0)
                plan = (plan[0].to(dev), plan[1].to(dev), plan[2])
                pt = torch.tensor(pages, dtype=torch.int32, device=dev)
                R = max(1, -(-640_000_000 // (nxt * ps * tok_bytes)))
                caches = []
                for _ in range(R):
                    k = torch.randn(nxt, Hkv, ps, hd, dtype=torch.bfloat16,
                                    device=dev)
                    v = torch.randn(nxt, Hkv, hd, ps, dtype=torch.bfloat16,
                                    device=dev)
                    caches.append((k.to(store), v.to(store)))

                def decode(i):
                    kc, vc = caches[i % R]
                    return ops.paged_attention_decode(
                        q, kc, vc, pt, ctxl, scale, scratch,
                        v_transposed=True)

                def shared_fn(i):
                    kc, vc = caches[i % R]
                    return ops.paged_attention_decode_shared(
                        q, kc, vc, pt, ctxl, plan, scale, scratch)

                diff = float((shared_fn(0).float()
                              - decode(0).float()).abs().max())
                fns = {"decode": decode, "shared": shared_fn}
                n = {}
                for name, fn in fns.items():
                    event_time(fn, 2 * R)                       # warm-up
                    n[name] = max(2 * R, int(window / event_time(fn, 2 * R)))
                ts = {name: [] for name in fns}
                for _ in range(rounds):
                    for name, fn in fns.items():
                        ts[name].append(event_time(fn, n[name]))
                t = {name: min(v) for name, v in ts.items()}
                gb_d = B * ctx * tok_bytes / 1e9
                gb_s = item_tokens * tok_bytes / 1e9
                print(f"shared_prefix {'fp8 ' if fp8 else 'bf16'} B{B} "
                      f"groups {groups} Hq{Hq}/{Hkv} ctx{ctx} shared {shared} "
                      f"R={R} members {plan[2]}: decode "
                      f"{t['decode']*1e6:7.1f}-{max(ts['decode'])*1e6:7.1f} us"
                      f" streamed {gb_d*1e3:5.0f} MB {gb_d/t['decode']:5.0f} "
                      f"GB/s | shared {t['shared']*1e6:7.1f}-"
                      f"{max(ts['shared'])*1e6:7.1f} us streamed "
                      f"{gb_s*1e3:5.0f} MB {gb_s/t['shared']:5.0f} GB/s | "
                      f"decode/shared {t['decode']/t['shared']:5.2f}x | "
                      f"max |shared - decode| {diff:.1e}", flush=True)
                del caches


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


def bench_logprobs(V=128256, Bs=(1, 16, 64), Ns=(1, 5, 20), rounds=3,
                   calls=200):
    """ops.top_logprobs (csrc/logprobs.hip) against the torch sequence of
    compute_logprobs (log_softmax, topk, gather) on the same fp32 logits.
    cold: call i reads copy i % R of the rows, R copies together past 640 MB
    (the Infinity Cache holds 256 MB); warm: the same rows every call, as
    right after the sampler has read them. Device events around `calls`
    back-to-back eager calls, the two alternated `rounds` times, best of the
    rounds. Then the kernel at every power-of-two slices per row next to the
    dispatch's own choice (ops._logprobs_slices), cold, N = 20."""
    def event_time(fn):
        start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        for i in range(5):
            fn(i)
        start.record()
        for i in range(calls):
            fn(i)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e-3 / calls

    for B in Bs:
        R = -(-640_000_000 // (B * V * 4))
        pool = torch.randn(R * B, V, device="cuda")
        sampled = torch.randint(0, V, (B,), dtype=torch.int32, device="cuda")
        idx = sampled.long().unsqueeze(-1)

        def rows(i, cold):
            r = i % R if cold else 0
            return pool[r * B:(r + 1) * B]

        for N in Ns:
            want = torch.full((B,), N, dtype=torch.int32, device="cuda")
            out = ops.top_logprobs(rows(0, False), sampled, want, N)

            def old(i, cold):
                lp = torch.log_softmax(rows(i, cold), dim=-1)
                torch.topk(lp, N, dim=-1)
                lp.gather(-1, idx)

            def new(i, cold, S=None):
                ops.top_logprobs(rows(i, cold), sampled, want, N, out, S)

            for cold in (True, False):
                ts = {"torch": [], "kernel": []}
                for _ in range(rounds):
                    ts["torch"].append(event_time(lambda i: old(i, cold)))
                    ts["kernel"].append(event_time(lambda i: new(i, cold)))
                t, k = min(ts["torch"]), min(ts["kernel"])
                print(f"logprobs [B{B} V{V} N{N}] {'cold' if cold else 'warm'}"
                      f": torch {t*1e6:7.1f} us | kernel {k*1e6:7.1f} us "
                      f"{B*V*4/k/1e9:7.1f} GB/s | {t/k:5.2f}x")
        pick = ops._logprobs_slices(B, V)
        sweep = sorted({1, 2, 4, 8, 16, 32, 64, pick})
        ts = {S: [] for S in sweep}
        for _ in range(rounds):
            for S in sweep:
                ts[S].append(event_time(lambda i: new(i, True, S)))
        print(f"logprobs [B{B} V{V} N{Ns[-1]}] cold, slices (dispatch {pick}): "
              + " | ".join(f"{S} {min(v)*1e6:6.1f} us" for S, v in ts.items()))
        del pool


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


def bench_tile_sweep(Ms=(32, 48, 64, 96, 128, 256, 512), reps=3):
    """The tiled W8A16 / W4A16 GEMM (csrc/quant_tile_gemm.hip) at every
    launchable point and both W cache policies on the four llama-3-70b layer
    shapes, cache-cold as bench_skinny_gemm is (launch i reads copy i % R of
    W, R * bytes(W) >= 1 GiB), against (1) what the dispatch runs with the
    tiled kernel switched off - the skinny kernel where it applies, else
    dequantise + the library GEMM, timed as one unit - and (2) the bf16
    dispatch. The candidates alternate inside each of `reps` rounds; the
    figure is the minimum. Bytes/s are of stored W (scales included). Picks
    ops.*_TILE_GEMM_SHAPES and TILE_GEMM_MIN_M / MAX_M."""
    from dynamo_amd.utils import enable_tunableop
    enable_tunableop(tuning=False)
    ops.set_tile_gemm(False)
    for name, N, K in (("qkv", 10240, 8192), ("o", 8192, 8192),
                       ("gateup", 57344, 8192), ("down", 8192, 28672)):
        R = max(2, -(-(1 << 30) // (N * K * 2)))
        ws = [torch.randn(N, K, dtype=torch.bfloat16, device="cuda") * 0.02
              for _ in range(R)]
        for fmt in ("fp8", "mxfp4"):
            wbytes = N * K if fmt == "fp8" else N * K // 2 + N * K // 32
            Rq = max(2, -(-(1 << 30) // wbytes))
            holder = ops.Fp8Weight if fmt == "fp8" else ops.Mxfp4Weight
            first = [holder.from_tensor(w) for w in ws]
            hs = [first[r] if r < R else
                  holder(first[r % R].q.clone(), first[r % R].scale.clone())
                  for r in range(Rq)]
            gemm = getattr(ops.hip(), f"{fmt}_tile_gemm")
            kstep = ops.TILE_GEMM_KSTEP[fmt]
            for M in Ms:
                x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda")
                y = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
                i = [0]

                def parent():
                    i[0] += 1
                    return ops.linear(x, hs[i[0] % Rq])

                def bf16():
                    i[0] += 1
                    return ops.linear(x, ws[i[0] % R])

                def tile(p, nt):
                    i[0] += 1
                    h = hs[i[0] % Rq]
                    gemm(y, x, h.q, h.scale, *p, False, nt)

                path = (ops.fp8_linear_path if fmt == "fp8"
                        else ops.mxfp4_linear_path)(x, hs[0])
                cands = {f"parent:{path[0]}": parent, "bf16": bf16}
                for p in ops.TILE_GEMM_CONFIGS[fmt]:
                    if K % (p[2] * kstep * p[4]) == 0:
                        for nt in (1, 0):
                            cands["tile:" + ",".join(map(str, p)) +
                                  (":nt" if nt else ":dflt")] = (
                                lambda p=p, nt=nt: tile(p, nt))
                ts = {c: [] for c in cands}
                for _ in range(reps):
                    for c, fn in cands.items():
                        ts[c].append(timeit(fn, iters=30, warmup=3))
                for c, v in ts.items():
                    t = min(v)
                    print(f"tile_sweep {fmt} {name} M={M} {c}: {t*1e6:8.1f} us "
                          f"{wbytes/t/1e12:5.2f} TB/s "
                          f"{2*M*N*K/t/1e12:7.1f} TF", flush=True)
            del hs, first
        del ws


# MI355X dense peak of the fp8 MFMA (v_mfma_*_f8f6f4 with fp8 operands),
# 2 x the bf16 MFMA's 2.5 PFLOP/s: the bound of the mx_gemm_sweep rows.
MX_FP8_PEAK_TF = 5000.0


def bench_mx_gemm_sweep(Ms=(256, 512, 1024, 2048, 4096, 8192), reps=3,
                        shapes=None, acc_m=512):
    """The W8A8 / W4A8 prefill GEMM (csrc/mx_gemm.hip) at every launchable
    point on the four llama-3-70b layer shapes, cache-cold as bench_tile_sweep
    is (launch i reads copy i % R of W, R * bytes(W) >= 1 GiB), against (1)
    what the dispatch runs with the mx kernel switched off - dequantise + the
    library GEMM (the tiled kernel at M = 256 if that is switched on), timed
    as one unit - and (2) the bf16 dispatch. The new path's time includes the
    activation quantiser. The candidates alternate inside each of `reps`
    rounds; the figure is the minimum. At M = acc_m it also prints the
    relative Frobenius error of the new path and of the parent path against
    x.double() @ W_exact.T. Picks ops.*_MX_GEMM_SHAPES and MX_GEMM_MIN_M."""
    from dynamo_amd.utils import enable_tunableop
    enable_tunableop(tuning=False)
    ops.set_mx_gemm(False)
    for name, N, K in (("qkv", 10240, 8192), ("o", 8192, 8192),
                       ("gateup", 57344, 8192), ("down", 8192, 28672)):
        if shapes and name not in shapes:
            continue
        R = max(2, -(-(1 << 30) // (N * K * 2)))
        ws = [torch.randn(N, K, dtype=torch.bfloat16, device="cuda") * 0.02
              for _ in range(R)]
        for fmt in ("fp8", "mxfp4"):
            wbytes = N * K if fmt == "fp8" else N * K // 2 + N * K // 32
            Rq = max(2, -(-(1 << 30) // wbytes))
            holder = ops.Fp8Weight if fmt == "fp8" else ops.Mxfp4Weight
            first = [holder.from_tensor(w) for w in ws]
            hs = [first[r] if r < R else
                  holder(first[r % R].q.clone(), first[r % R].scale.clone())
                  for r in range(Rq)]
            gemm = getattr(ops.hip(), f"{fmt}_mx_gemm")
            for M in Ms:
                x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda")
                y = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
                xq = torch.empty(M, K, dtype=torch.float8_e4m3fn,
                                 device="cuda")
                xs = torch.empty(M, K // 32, dtype=torch.uint8, device="cuda")
                i = [0]

                def parent():
                    i[0] += 1
                    return ops.linear(x, hs[i[0] % Rq])

                def bf16():
                    i[0] += 1
                    return ops.linear(x, ws[i[0] % R])

                def mx(p):
                    i[0] += 1
                    h = hs[i[0] % Rq]
                    ops.hip().mxfp8_quantize_rows(xq, xs, x)
                    gemm(y, xq, xs, h.q, h.scale, *p)

                path = (ops.fp8_linear_path if fmt == "fp8"
                        else ops.mxfp4_linear_path)(x, hs[0])
                cands = {f"parent:{path[0]}": parent, "bf16": bf16}
                for p in ops.MX_GEMM_CONFIGS[fmt]:
                    cands["mx:" + ",".join(map(str, p))] = (
                        lambda p=p: mx(p))
                iters = max(4, min(30, (1 << 15) // M))
                ts = {c: [] for c in cands}
                for _ in range(reps):
                    for c, fn in cands.items():
                        ts[c].append(timeit(fn, iters=iters, warmup=2))
                t_parent = min(ts[f"parent:{path[0]}"])
                for c, v in ts.items():
                    t = min(v)
                    tf = 2 * M * N * K / t / 1e12
                    print(f"mx_gemm_sweep {fmt} {name} M={M} {c}: "
                          f"{t*1e6:9.1f} us {tf:7.1f} TF "
                          f"({100 * tf / MX_FP8_PEAK_TF:4.1f} % of the fp8 "
                          f"MFMA peak) parent/this {t_parent/t:5.2f}",
                          flush=True)
                if M == acc_m:
                    h = hs[0]
                    wx = h.effective(torch.float32).double()
                    ref = x.double() @ wx.T
                    ops.hip().mxfp8_quantize_rows(xq, xs, x)
                    gemm(y, xq, xs, h.q, h.scale, *ops.MX_GEMM_CONFIGS[fmt][0])
                    e_new = ((y.double() - ref).norm() / ref.norm()).item()
                    e_par = ((ops.linear(x, h).double() - ref).norm()
                             / ref.norm()).item()
                    print(f"mx_gemm_sweep {fmt} {name} M={M} relative "
                          f"Frobenius error: mx {e_new:.3e} parent "
                          f"{e_par:.3e}", flush=True)
                    del wx, ref
            del hs, first
        del ws


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


# --------------------------------------------------------------------------
# Routed MoE decode (csrc/moe_decode.hip) at Mixtral-8x7B shapes
MIXTRAL = dict(D=4096, I=14336, E=8, topk=2)


def _event_time(g, n):
    """Seconds per replay of graph g over n back-to-back replays, by device
    events."""
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(n):
        g.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3 / n


def _capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def _replays_for(g, window):
    """How many replays fill `window` seconds."""
    return max(5, int(window / _event_time(g, 5)) + 1)


def bench_moe_decode(Ts=(1, 4, 16, 64), rounds=3, window=0.5):
    """One MoEMLP at Mixtral-8x7B shapes: the padded-bmm route (the default),
    the grouped-kernel route (DYNAMO_MOE_BMM=0) and the routed kernels
    (DYNAMO_MOE_FUSED=1), each a captured graph, alternated `rounds` times in
    windows of >= `window` s. us per block (min - max over the rounds) and the
    weight bytes of the experts the routing makes live over the best time."""
    from dynamo_amd.engine.config import ModelConfig
    from dynamo_amd.models.layers import TPContext, linear
    from dynamo_amd.models.mixtral import MoEMLP
    m = MIXTRAL
    cfg = ModelConfig(name="mixtral-8x7b-moe", arch="mixtral",
                      hidden_size=m["D"], intermediate_size=m["I"],
                      num_experts=m["E"], num_experts_per_tok=m["topk"])
    moe = MoEMLP(cfg, TPContext(), "cuda", torch.bfloat16)
    envs_of = {"bmm": {}, "seg": {"DYNAMO_MOE_BMM": "0"},
               "fused": {"DYNAMO_MOE_FUSED": "1"}}
    for T in Ts:
        x = torch.randn(T, m["D"], dtype=torch.bfloat16, device="cuda")
        topi = ops.topk_gating(linear(x, moe.router).float(), m["topk"])[1]
        live = int(topi.unique().numel())
        gb = live * 3 * m["I"] * m["D"] * 2 / 1e9
        graphs, outs = {}, {}
        for route, env in envs_of.items():
            for k in ("DYNAMO_MOE_BMM", "DYNAMO_MOE_FUSED"):
                os.environ.pop(k, None)
            os.environ.update(env)
            with torch.no_grad():
                outs[route] = moe.forward(x).float()
            graphs[route] = _capture(lambda: moe.forward(x))
            os.environ.pop(next(iter(env), ""), None)
        n = {r: _replays_for(g, window) for r, g in graphs.items()}
        ts = {r: [] for r in graphs}
        for _ in range(rounds):
            for r, g in graphs.items():
                ts[r].append(_event_time(g, n[r]))
        diff = float((outs["fused"] - outs["bmm"]).abs().max()
                     / outs["bmm"].abs().max())
        row = " | ".join(
            f"{r} {min(v)*1e6:7.1f}-{max(v)*1e6:7.1f} us "
            f"{gb/min(v):5.0f} GB/s" for r, v in ts.items())
        print(f"moe_decode T={T:2d} live {live} ({gb:.2f} GB): {row} | "
              f"bmm/fused {min(ts['bmm'])/min(ts['fused']):4.2f}x | "
              f"max |fused - bmm| / max |bmm| {diff:.1e}")


def bench_moe_decode_sweep(Ts=(1, 16, 64), tps=(1, 2, 4, 8), window=0.15,
                           fmts=("bf16", "fp8", "mxfp4")):
    """Every point of ops.MOE_DECODE_CONFIGS on Mixtral-8x7B's gate/up
    (SwiGLU epilogue, gathered A) and down (weighted epilogue + combine)
    expert weights and their TP shards of I: picks ops.MOE_DECODE_SHAPES.
    The pick for T <= 16 is the lowest sum of times relative to the best at
    T = 1 and T = 16, the pick for T > 16 the fastest at T = 64.
    With quantised formats in `fmts` the same shapes, T and routings run the
    fp8 / mxfp4 kernels on the quantised weights next to the bf16 column
    (picks ops.MOE_DECODE_FP8_SHAPES / MOE_DECODE_MXFP4_SHAPES); live bytes
    count codes and scales."""
    m = MIXTRAL
    E, K, D = m["E"], m["topk"], m["D"]
    holder = {"bf16": lambda w: w,
              "fp8": ops.Fp8ExpertWeight.from_tensor,
              "mxfp4": ops.Mxfp4ExpertWeight.from_tensor}
    bytes_per_weight = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 0.5 + 1 / 32}
    for tp in tps:
        I = m["I"] // tp
        for name, shape in (("gate_up", (E, 2 * I, D)), ("down", (E, D, I))):
            N, Kd = shape[1:]
            w16 = torch.randn(shape, dtype=torch.bfloat16, device="cuda")
            ws = {f: holder[f](w16) for f in fmts}
            del w16
            fits = {f: [c for c in ops.MOE_DECODE_FORMATS[f][1]
                        if Kd % (c[0] * ops.MOE_DECODE_FORMATS[f][0]
                                 * c[1]) == 0] for f in fmts}
            t = {}
            for T in Ts:
                logits = torch.randn(T, E, device="cuda")
                topw, topi = ops.topk_gating(logits, K)
                seg, pair = ops.moe_route(topi, E)
                live = int(topi.unique().numel())
                x = torch.randn(T, D, dtype=torch.bfloat16, device="cuda")
                act = torch.randn(T * K, I, dtype=torch.bfloat16,
                                  device="cuda")
                for f in fmts:
                    w = ws[f]
                    for c in fits[f]:
                        if name == "gate_up":
                            fn = lambda: ops.moe_routed_gemm(  # noqa: E731
                                x, w, seg, pair, K, gather=True, glu=True,
                                cfg=c)
                        else:
                            fn = lambda: ops.moe_down_combine(  # noqa: E731
                                act, w, seg, pair, topw, cfg=c)
                        g = _capture(fn)
                        t[f, T, c] = _event_time(g, _replays_for(g, window))
                    best = min(t[f, T, c] for c in fits[f])
                    gb = live * N * Kd * bytes_per_weight[f] / 1e9
                    print(f"moe_decode_sweep {f} {name} ({N}, {Kd}) T={T:2d} "
                          f"live {live}: " + " | ".join(
                              f"{c} {t[f, T, c]*1e6:6.1f}" for c in fits[f])
                          + f" us; best {best*1e6:6.1f} us "
                          f"{gb/best:5.0f} GB/s")
            for f in fmts:
                rel = {c: sum(t[f, T, c] / min(t[f, T, d] for d in fits[f])
                              for T in Ts if T <= 16) for c in fits[f]}
                small = min(fits[f], key=rel.get)
                large = min(fits[f], key=lambda c: t[f, max(Ts), c])
                print(f"moe_decode_sweep PICK {f} ({N}, {Kd}): "
                      f"({small}, {large}),")
            del ws


def _eager_time(fn, n):
    """Seconds per call of fn over n back-to-back eager calls, by device
    events around synchronised work (fn may read back to the host)."""
    torch.cuda.synchronize()
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3 / n


def bench_moe_tiled_sweep(Ts=(128, 256, 512, 1024, 2048), tps=(1, 2),
                          fmts=("fp8", "mxfp4"), rounds=3, window=0.1):
    """The tiled routed MoE (ops.moe_tiled_mlp: route + gate/up GEMM with
    SwiGLU + weighted down GEMM + combine) against the host-side expert loop
    it replaces (MoEMLP._expert_loop), on Mixtral-8x7B's experts and their
    TP-2 shards, E = 8, top-2 with seeded random routing. Both are warmed up
    and then alternated `rounds` times eagerly: picks ops.MOE_TILE_MAX_T.
    Before that, every point of ops.MOE_TILE_CONFIGS at the T's BM on each
    GEMM alone (captured graphs): picks ops.MOE_TILE_SHAPES."""
    from dynamo_amd.engine.config import ModelConfig
    from dynamo_amd.models.layers import TPContext
    from dynamo_amd.models.mixtral import MoEMLP
    m = MIXTRAL
    E, K, D = m["E"], m["topk"], m["D"]
    holder = {"fp8": ops.Fp8ExpertWeight.from_tensor,
              "mxfp4": ops.Mxfp4ExpertWeight.from_tensor}
    for tp in tps:
        I = m["I"] // tp
        cfg = ModelConfig(name="mixtral-8x7b-moe", arch="mixtral",
                          hidden_size=D, intermediate_size=I, num_experts=E,
                          num_experts_per_tok=K)
        moe = MoEMLP(cfg, TPContext(), "cuda", torch.bfloat16)
        w16 = (moe.w_gate_up, moe.w_down)
        for f in fmts:
            wgu, wd = (holder[f](w) for w in w16)
            moe.w_gate_up, moe.w_down = wgu, wd
            kstep = ops.MOE_DECODE_FORMATS[f][0]
            t = {}
            for T in Ts:
                gen = torch.Generator(device="cuda").manual_seed(T)
                topw, topi = ops.topk_gating(
                    torch.randn(T, E, device="cuda", generator=gen), K)
                x = torch.randn(T, D, dtype=torch.bfloat16, device="cuda",
                                generator=gen)
                bm = ops.moe_tile_bm(T, K, E)
                route = ops.moe_route_tiled(topi, E, bm)
                act = ops.moe_tiled_gemm(x, wgu, route, K, gather=True,
                                         glu=True)
                for name, w in (("gate_up", wgu), ("down", wd)):
                    fits = [c for c in ops.MOE_TILE_CONFIGS[f] if c[0] == bm
                            and w.shape[2] % (c[2] * kstep * c[4]) == 0]
                    for c in fits:
                        if name == "gate_up":
                            fn = lambda: ops.moe_tiled_gemm(  # noqa: E731
                                x, w, route, K, gather=True, glu=True, cfg=c)
                        else:
                            fn = lambda: ops.moe_tiled_down_combine(  # noqa: E731
                                act, w, route, topw, cfg=c)
                        g = _capture(fn)
                        t[name, T, c] = _event_time(g, _replays_for(g, window))
                    print(f"moe_tiled_sweep POINTS {f} {name} "
                          f"{tuple(w.shape[1:])} T={T:4d} BM={bm}: "
                          + " | ".join(f"{c[1:]} {t[name, T, c]*1e6:7.1f}"
                                       for c in fits) + " us; best "
                          f"{min(fits, key=lambda c: t[name, T, c])[1:]}")
                tiled = lambda: ops.moe_tiled_mlp(x, topw, topi, wgu, wd)  # noqa: E731
                loop = lambda: moe._expert_loop(  # noqa: E731
                    x, topw.to(x.dtype), topi)
                with torch.no_grad():
                    diff = float((tiled().float() - loop().float()).abs().max()
                                 / loop().float().abs().max())
                    n = {r: max(3, int(window / _eager_time(fn, 3)) + 1)
                         for r, fn in (("tiled", tiled), ("loop", loop))}
                    ts = {"tiled": [], "loop": []}
                    for _ in range(rounds):
                        ts["tiled"].append(_eager_time(tiled, n["tiled"]))
                        ts["loop"].append(_eager_time(loop, n["loop"]))
                print(f"moe_tiled_sweep MLP {f} tp{tp} T={T:4d} BM={bm}: "
                      + " | ".join(f"{r} {min(v)*1e6:8.1f}-{max(v)*1e6:8.1f} us"
                                   for r, v in ts.items())
                      + f" | loop/tiled {min(ts['loop'])/min(ts['tiled']):5.2f}x"
                      f" | max |tiled - loop| / max |loop| {diff:.1e}")
            del wgu, wd
        del moe, w16


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
    if w in ("all", "mq_attn"):
        bench_mq_attn()
    if w in ("all", "shared_prefix"):
        bench_shared_prefix()
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
    if w in ("all", "logprobs"):
        bench_logprobs()
    if w in ("all", "gemm"):
        bench_gemm()
        bench_gemm(M=8192)
        bench_skinny_gemm()
        bench_skinny_gemm(M=64)
    if w in ("all", "lora"):
        bench_lora()
    if w in ("all", "moe_decode"):
        bench_moe_decode()
    if w == "moe_decode_sweep":
        # every launchable routed-GEMM configuration per Mixtral shape:
        # picks ops.MOE_DECODE_SHAPES
        bench_moe_decode_sweep()
    if w == "moe_tiled_sweep":
        # the tiled routed MoE against the host-side expert loop, and every
        # launchable point per Mixtral shape: picks ops.MOE_TILE_MAX_T and
        # ops.MOE_TILE_SHAPES
        bench_moe_tiled_sweep()
    if w == "mx_gemm_sweep":
        # every launchable point of the W8A8 / W4A8 prefill GEMM per shape
        # and M: picks ops.*_MX_GEMM_SHAPES and MX_GEMM_MIN_M
        bench_mx_gemm_sweep()
    if w == "tile_sweep":
        # every launchable point of the tiled quantised GEMM per shape and M:
        # picks ops.*_TILE_GEMM_SHAPES, TILE_GEMM_MIN_M and TILE_GEMM_MAX_M
        bench_tile_sweep()
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
