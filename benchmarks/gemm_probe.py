"""Measure hipBLASLt bandwidth on the decode-regime (skinny-M) GEMMs.

At decode the per-step GEMMs are M=conc (16) by the weight shapes of the
flagship models; they are weight-streaming-bound, so report effective
TB/s of W bytes (the only traffic that matters at M=16). This sizes the
headroom for the in-tree skinny GEMM (dynamo_amd/csrc/skinny_gemm.hip).
"""
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [
    # (name, K, N)  y[M,N] = x[M,K] @ W[N,K]^T   (llama-3-70b per-layer)
    ("qkv   ", 8192, 8192 + 2048),
    ("o     ", 8192, 8192),
    ("gateup", 8192, 57344),
    ("down  ", 28672, 8192),
    ("lmhead", 8192, 128256),
    # mixtral-8x7b dense parts
    ("mx_qkv", 4096, 4096 + 2048),
]


def _rate(x, ws, iters):
    """us per x @ w^T, launch i on ws[i % len(ws)]."""
    R = len(ws)
    for i in range(5):
        y = F.linear(x, ws[i % R])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        y = F.linear(x, ws[(i + 5) % R])
    torch.cuda.synchronize()
    del y
    return (time.perf_counter() - t0) / iters * 1e6


def main(M=16, iters=48):
    """hipBLASLt under the project's TunableOp table (as bench.py runs it),
    in two cache states: "hot" replays one W buffer (what this probe used to
    report; the 134 / 168 MB o / qkv matrices then sit in the 256 MiB
    Infinity Cache), "cold" rotates over R distinct copies of W with
    R * bytes(W) >= 1 GiB so no launch reads the buffer of the one before it.
    The decode step streams 137 GB of weights between two uses of a matrix,
    so cold is the state it runs in; compare benchmarks/skinny_sweep.hip."""
    if M >= 1024:
        return main_big(M)

    torch.cuda.init()
    from dynamo_amd.utils import enable_tunableop
    enable_tunableop(tuning=False)
    dev = "cuda:0"
    print(f"M={M} bf16, {iters} iters, W bytes / time")
    for name, K, N in SHAPES:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        wbytes = N * K * 2
        R = max(2, -(-(1 << 30) // wbytes))
        ws = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02
              for _ in range(R)]
        hot = _rate(x, ws[:1], iters)
        cold = _rate(x, ws, iters)
        gb = wbytes / 1e9
        print(f"{name} K={K:6d} N={N:6d}  hot {hot:8.1f} us {gb/hot*1e3:6.2f} "
              f"TB/s | cold (R={R}) {cold:8.1f} us {gb/cold*1e3:6.2f} TB/s")
        del ws


def main_big(M):
    """Prefill-regime GEMMs: report TFLOP/s vs the 2.5 PF bf16 dense peak."""
    import time
    dev = "cuda:0"
    print(f"M={M} bf16 prefill shapes")
    for name, K, N in SHAPES[:5]:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16)
        for _ in range(3):
            y = x @ w.t()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            y = x @ w.t()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 10
        fl = 2.0 * M * N * K
        print(f"{name} K={K:6d} N={N:6d}  {dt*1e3:8.2f} ms  "
              f"{fl/dt/1e12:7.1f} TF  ({fl/dt/25e12:4.1f}% of 2.5PF)")
    del y  # noqa: F841


if __name__ == "__main__":
    import sys
    main(M=int(sys.argv[1]) if len(sys.argv) > 1 else 16)
