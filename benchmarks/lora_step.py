"""Decode step time with per-request LoRA adapters (run on an MI355X box).

The workload is bench.py's flagship decode state (llama-3-70b, ISL 8192,
16 sequences, put at decode by bench.attach_at_decode); bench.py itself has
no adapter flag. One engine per invocation, then one scenario after another
on it, each with fresh requests:

  base      no request names an adapter
  one       every request on one rank-`--rank` adapter
  spread    the requests spread over all `--max-loras` adapters

With --max-loras 0 only `base` runs, and nothing of the adapter interface is
touched, so `--repo DIR` can point the same script at another checkout (the
parent commit, built in DIR) for a paired comparison on one box. Prints one
JSON line per scenario: ms/step over --steps timed steps after --warmup.
"""
import argparse
import json
import os
import sys
import time
import types


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), help="checkout to import from")
    ap.add_argument("--max-loras", type=int, default=8)
    ap.add_argument("--max-lora-rank", type=int, default=64)
    ap.add_argument("--rank", type=int, default=16, help="adapter rank")
    ap.add_argument("--model", default="llama-3-70b")
    ap.add_argument("--isl", type=int, default=8192)
    ap.add_argument("--osl", type=int, default=1024)
    ap.add_argument("--conc", type=int, default=16)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=1,
                    help="repeat the scenario list, interleaved")
    ap.add_argument("--label", default="")
    ap.add_argument("--device", default="cuda:0",
                    help="cpu (with a tiny --model) only rehearses the script")
    a = ap.parse_args()

    sys.path.insert(0, os.path.abspath(a.repo))
    import torch
    import bench
    from dynamo_amd.engine import LLMEngine
    from dynamo_amd.models.registry import resolve_model_config

    bargs = types.SimpleNamespace(
        page_size=64, conc_per_gpu=a.conc, max_batched_tokens=0, isl=a.isl,
        osl=a.osl, kv_pool_pages=0, kv_cache_dtype="auto", kv_v_layout="auto",
        moe_ep=False)
    mc = resolve_model_config(a.model)
    cfg = bench.make_cfg(bargs, mc, a.device)
    if a.max_loras:
        cfg.max_loras, cfg.max_lora_rank = a.max_loras, a.max_lora_rank

    def sync():
        if a.device.startswith("cuda"):
            torch.cuda.synchronize()

    t0 = time.monotonic()
    eng = LLMEngine(cfg, seed=0)
    sync()
    print(f"# engine init {time.monotonic() - t0:.1f}s "
          f"({eng.runner.num_pages} pages, max_loras={a.max_loras})",
          flush=True)
    names = [f"ad{i}" for i in range(a.max_loras)]
    for i, n in enumerate(names):
        eng.load_lora(n, rank=a.rank, seed=100 + i)

    scenarios = [("base", lambda i: None)]
    if a.max_loras:
        scenarios += [("one", lambda i: names[0]),
                      ("spread", lambda i: names[i % len(names)])]
    prompts = bench.make_prompts(bargs, mc, a.conc, 1234)
    run = 0
    for rnd in range(a.rounds):
        for sname, pick in scenarios:
            run += 1
            ids = [f"s{run}-{i}" for i in range(a.conc)]
            bench.attach_at_decode(eng, bargs, mc, ids, prompts, 4321)
            for i, rid in enumerate(ids):
                lo = pick(i)
                if lo is not None:
                    req = eng.requests[rid]
                    req.lora, req.lora_slot = lo, eng.lora_bank.slot(lo)
            eng.step()              # admission
            for _ in range(a.warmup):
                eng.step()
            sync()
            t0 = time.monotonic()
            for _ in range(a.steps):
                eng.step()
            sync()
            ms = (time.monotonic() - t0) / a.steps * 1000
            gr = eng.graph_runner
            print(json.dumps({
                "label": a.label, "scenario": sname, "round": rnd,
                "max_loras": a.max_loras, "adapter_rank": a.rank,
                "ms_per_step": round(ms, 3),
                "tok_s": round(a.conc / ms * 1000, 1),
                "graph_keys": sorted(map(str, gr.graphs)) if gr else None,
            }), flush=True)
            for rid in ids:
                eng.abort(rid)


if __name__ == "__main__":
    main()
