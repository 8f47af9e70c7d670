"""Per-request LoRA adapters in one batch (CPU, tiny-llama, fp32): the
batched delta op against a dense float64 reference, mixed-adapter batches on
a bank engine (EngineConfig.max_loras > 0) against the same requests alone
and against the engine-activated path, prefix-cache isolation, the error
cases, and the serving surface (worker payload, TP command, frontend)."""
import asyncio

import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS

TOL = dict(rtol=1e-4, atol=1e-4)    # as tests/test_lora.py
PROMPT = list(range(40))


def make_engine(max_loras=2, max_lora_rank=8, model="tiny-llama",
                prefix=False, **kw):
    cfg = EngineConfig(model=PRESETS[model], device="cpu", dtype="float32",
                       max_num_seqs=4, max_batched_tokens=256,
                       max_model_len=256, kv_pool_pages=64, page_size=16,
                       enable_prefix_caching=prefix, max_loras=max_loras,
                       max_lora_rank=max_lora_rank, **kw)
    return LLMEngine(cfg, seed=7)


def load_two(e):
    e.load_lora("ad1", rank=4, seed=11)
    e.load_lora("ad2", rank=8, seed=12)
    return e


def run(e, reqs, n=6):
    """reqs: [(id, prompt, adapter)] added together -> {id: tokens}."""
    for rid, prompt, lora in reqs:
        e.add_request(rid, prompt, SamplingParams(max_tokens=n), lora=lora)
    out = {rid: [] for rid, _, _ in reqs}
    while e.has_work():
        for so in e.step():
            out[so.req_id].append(so.new_token)
    return out


@pytest.fixture(scope="module")
def bank_engine():
    return load_two(make_engine())


# -- the op ---------------------------------------------------------------
def test_lora_delta_matches_dense_reference():
    g = torch.Generator().manual_seed(0)
    T, K, N, S, R = 7, 48, 40, 3, 16
    x = torch.randn(T, K, generator=g)
    y = torch.randn(T, N, generator=g)
    A = torch.randn(S, R, K, generator=g) * 0.1
    B = torch.randn(S, N, R, generator=g) * 0.1
    ranks = torch.tensor([4, 0, 16], dtype=torch.int32)   # slot 1: rank 0
    scales = torch.tensor([4.0, 2.0, 0.5])
    # nothing at r >= rank may be read
    for s, r in enumerate(ranks.tolist()):
        A[s, r:] = float("nan")
        B[s, :, r:] = float("nan")
    slots = torch.tensor([0, -1, 2, 1, 0, -1, 2], dtype=torch.int32)
    y0 = y.clone()
    out = ops.lora_delta_(y, x, (A, B, ranks, scales), slots)
    assert out is y
    ref = y0.double().clone()
    for i, s in enumerate(slots.tolist()):
        if s < 0:
            continue
        r = int(ranks[s])
        ref[i] += float(scales[s]) * (
            (x[i].double() @ A[s, :r].double().t()) @ B[s, :, :r].double().t())
    assert torch.isfinite(y).all()
    assert torch.allclose(y.double(), ref, **TOL)
    for i in (1, 5, 3):                 # slot -1 and the rank-0 slot
        assert torch.equal(y[i], y0[i])
    assert not torch.equal(y[0], y0[0])


# -- engine ---------------------------------------------------------------
def test_mixed_batch_matches_each_request_alone(bank_engine):
    e = bank_engine
    mixed = run(e, [("b", PROMPT, None), ("x", PROMPT, "ad1"),
                    ("y", PROMPT, "ad2")])
    alone = {rid: run(e, [(rid + "-alone", PROMPT, lora)])[rid + "-alone"]
             for rid, lora in (("b", None), ("x", "ad1"), ("y", "ad2"))}
    assert mixed == alone
    base = run(make_engine(max_loras=0), [("b0", PROMPT, None)])["b0"]
    assert mixed["b"] == base
    assert mixed["x"] != base and mixed["y"] != base
    assert mixed["x"] != mixed["y"]
    assert all(len(v) == 6 for v in mixed.values())


def test_bank_load_keeps_engine_inactive(bank_engine):
    # never engine-activated: a request that names no adapter is the base
    # model's, and nothing is set on the layers' engine-level hook
    assert bank_engine.list_loras() == ["ad1", "ad2"]
    for layer in bank_engine.runner.model.layers:
        assert layer.attn.lora is None and layer.mlp.lora is None


def _decode_logits(e, lora):
    """Logits of the first decode step of PROMPT, run through the runner."""
    rid = f"lg-{lora}"
    e.add_request(rid, PROMPT, SamplingParams(max_tokens=4), lora=lora)
    first = e.step()                         # the prefill + first token
    assert [so.req_id for so in first] == [rid]
    sched = e.scheduler.schedule()
    assert len(sched.decodes) == 1 and not sched.prefills
    with torch.inference_mode():
        ids, meta = e.runner.prepare(sched)
        h = e.runner.model.forward(ids, e.runner.kv_pool, meta)
        logits = e.runner.model.compute_logits(h[meta.logits_rows]).clone()
    e.abort(rid)
    return first[0].new_token, meta, logits


def test_decode_logits_match_engine_activated_path(bank_engine):
    tok_b, meta, lg_bank = _decode_logits(bank_engine, "ad1")
    assert meta.lora_slots is not None and meta.lora_decode_rows == 1
    e0 = make_engine(max_loras=0)
    e0.load_lora("ad1", rank=4, seed=11)     # today's path: engine-activated
    tok_0, meta0, lg_act = _decode_logits(e0, None)
    assert meta0.lora_slots is None
    assert tok_b == tok_0
    assert torch.allclose(lg_bank, lg_act, **TOL)
    # and the adapter does move the logits
    _, _, lg_base = _decode_logits(bank_engine, None)
    assert not torch.allclose(lg_bank, lg_base, **TOL)


def test_prefix_cache_is_per_adapter():
    e = load_two(make_engine(prefix=True))
    prompt = list(range(64))                 # 4 full pages

    def first_step_prefill(rid, lora):
        e.add_request(rid, prompt, SamplingParams(max_tokens=4), lora=lora)
        toks = []
        prefilled = None
        while e.has_work():
            for so in e.step():
                toks.append(so.new_token)
            if prefilled is None:
                prefilled = e.last_metrics.prefill_tokens_step
        return toks, prefilled

    _, n1 = first_step_prefill("a1", "ad1")
    assert n1 == len(prompt)
    # the cache is on: the same prompt under the same adapter reuses pages
    _, n2 = first_step_prefill("a2", "ad1")
    assert n2 < len(prompt)
    # ... and the base model must not: KV under ad1 is not the base model's
    base_toks, n3 = first_step_prefill("b", None)
    assert n3 == len(prompt), "base request reused an adapter's KV"
    fresh = make_engine(max_loras=0, prefix=True)
    fresh.add_request("f", prompt, SamplingParams(max_tokens=4))
    want = []
    while fresh.has_work():
        want += [so.new_token for so in fresh.step()]
    assert base_toks == want
    _, n4 = first_step_prefill("c", "ad2")
    assert n4 == len(prompt)


def test_block_salt_is_stable_and_base_unchanged():
    from dynamo_amd.lora import lora_block_salt
    assert lora_block_salt(5, None) == 5
    a = lora_block_salt(5, "ad1")
    assert a == lora_block_salt(5, "ad1") and a != 5
    assert a != lora_block_salt(5, "ad2")
    assert 0 <= a < 2 ** 64
    # not Python's per-process hash(): a fixed function of the name
    import hashlib
    h = int.from_bytes(hashlib.blake2b(b"ad1", digest_size=8).digest(),
                       "little")
    assert lora_block_salt(0, "ad1") == (h | 1)


# -- errors ---------------------------------------------------------------
def test_errors(bank_engine):
    e = bank_engine
    with pytest.raises(ValueError, match="not loaded"):
        e.add_request("u", PROMPT, SamplingParams(max_tokens=2), lora="nope")
    assert "u" not in e.requests
    e0 = make_engine(max_loras=0)
    with pytest.raises(ValueError, match="max_loras"):
        e0.add_request("u", PROMPT, SamplingParams(max_tokens=2), lora="ad1")
    with pytest.raises(ValueError, match="slots"):
        e.load_lora("ad3", rank=4, seed=13)
    assert e.list_loras() == ["ad1", "ad2"]
    e.unload_lora("ad2")
    with pytest.raises(ValueError, match="max_lora_rank"):
        e.load_lora("big", rank=16, seed=14)       # bank holds rank <= 8
    assert e.list_loras() == ["ad1"]
    e.load_lora("ad2", rank=8, seed=12)            # the freed slot is reused
    e.add_request("live", PROMPT, SamplingParams(max_tokens=3), lora="ad1")
    with pytest.raises(ValueError, match="live request"):
        e.unload_lora("ad1")
    while e.has_work():
        e.step()
    e.unload_lora("ad1")                           # finished: allowed now
    assert e.list_loras() == ["ad2"]
    e.load_lora("ad1", rank=4, seed=11)


@pytest.mark.parametrize("kw, match", [
    (dict(model="tiny-opt"), "arch"),
    (dict(model="tiny-mixtral"), "arch"),
    (dict(weight_dtype="fp8"), "fp8"),
    (dict(weight_dtype="mxfp4"), "mxfp4"),
    (dict(max_lora_rank=12), "multiple of 8"),
])
def test_bank_engine_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        make_engine(**kw)


def test_bank_engine_refuses_a_weight_pool():
    from dynamo_amd.engine.model_runner import ModelRunner
    cfg = EngineConfig(model=PRESETS["tiny-llama"], device="cpu",
                       dtype="float32", kv_pool_pages=16, max_loras=2)
    with pytest.raises(ValueError, match="GMS weight pool"):
        ModelRunner(cfg, weight_pool=object())


def test_partial_adapter_gets_rank_zero(tmp_path):
    """A PEFT adapter that targets q_proj only leaves rank 0 in the other
    three projections; fused block forms count against max_lora_rank."""
    import json
    from safetensors.torch import save_file
    cfg = PRESETS["tiny-llama"]
    r = 4
    g = torch.Generator().manual_seed(3)
    sd = {}
    for li in range(cfg.num_layers):
        stem = f"base_model.model.model.layers.{li}.self_attn.q_proj"
        sd[f"{stem}.lora_A.weight"] = torch.randn(
            r, cfg.hidden_size, generator=g) * 0.1
        sd[f"{stem}.lora_B.weight"] = torch.randn(
            cfg.num_q_heads * cfg.head_dim, r, generator=g) * 0.1
    save_file(sd, str(tmp_path / "adapter_model.safetensors"))
    (tmp_path / "adapter_config.json").write_text(json.dumps(
        {"r": r, "lora_alpha": 128.0, "target_modules": ["q_proj"]}))
    e = make_engine()
    e.load_lora("qonly", path=str(tmp_path))
    bank = e.lora_bank
    s = bank.slot("qonly")
    assert bank.targets["0.qkv"].host_ranks[s] == r
    for t in ("o", "gate_up", "down"):
        assert bank.targets[f"0.{t}"].host_ranks[s] == 0
        assert int(bank.targets[f"0.{t}"].ranks[s]) == 0
    out = run(e, [("q", PROMPT, "qonly"), ("b", PROMPT, None)])
    assert out["q"] != out["b"]
    # q+k+v at r = 4 is a rank-12 block form: above a rank-8 bank
    for proj, rows in (("k_proj", cfg.num_kv_heads * cfg.head_dim),
                       ("v_proj", cfg.num_kv_heads * cfg.head_dim)):
        for li in range(cfg.num_layers):
            stem = f"base_model.model.model.layers.{li}.self_attn.{proj}"
            sd[f"{stem}.lora_A.weight"] = torch.randn(
                r, cfg.hidden_size, generator=g) * 0.1
            sd[f"{stem}.lora_B.weight"] = torch.randn(rows, r,
                                                      generator=g) * 0.1
    save_file(sd, str(tmp_path / "adapter_model.safetensors"))
    with pytest.raises(ValueError, match="max_lora_rank"):
        e.load_lora("qkv", path=str(tmp_path))


# -- serving --------------------------------------------------------------
def _loop_run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


def test_worker_generate_with_lora(bank_engine):
    want = run(bank_engine, [("w", PROMPT, "ad1")], n=5)["w"]

    async def main():
        from dynamo_amd.runtime import DistributedRuntime, MemoryDiscovery
        from dynamo_amd.workers import WorkerService
        shared = MemoryDiscovery()
        rt = DistributedRuntime(shared)
        ws = WorkerService(load_two(make_engine()), rt)
        await ws.start()
        addr = rt.server.address

        async def gen(payload):
            toks = []
            async for ch in rt.client.call_stream(addr, "backend.generate",
                                             payload):
                toks += ch.get("token_ids", [])
            return toks

        base_payload = {"token_ids": PROMPT,
                        "stop_conditions": {"max_tokens": 5}}
        got = await gen(dict(base_payload, lora="ad1"))
        base = await gen(base_payload)
        # an unknown adapter is an error for that caller, not for the loop
        with pytest.raises(Exception, match="not loaded"):
            await gen(dict(base_payload, lora="nope"))
        again = await gen(dict(base_payload, lora="ad1"))
        await ws.stop()
        await rt.shutdown(drain=False)
        return got, base, again

    got, base, again = _loop_run(main())
    assert got == want and again == want
    assert base != want


def test_tp_command_carries_lora(bank_engine):
    from dynamo_amd.parallel.tp import apply_command
    want = run(bank_engine, [("t", PROMPT, "ad2")], n=4)["t"]
    e = load_two(make_engine())
    cmd = {"new": [{"request_id": "r1", "token_ids": PROMPT,
                    "sampling": {"max_tokens": 4}, "lora": "ad2"},
                   {"request_id": "r0", "token_ids": PROMPT,
                    "sampling": {"max_tokens": 4}}],
           "step": True}
    got = {"r0": [], "r1": []}
    outs = apply_command(e, cmd)
    while True:
        for so in outs:
            got[so.req_id].append(so.new_token)
        if not e.has_work():
            break
        outs = apply_command(e, {"step": True})
    assert e.requests["r1"].lora == "ad2" and e.requests["r0"].lora is None
    assert got["r1"] == want and got["r0"] != want


def test_tp_group_spec_carries_lora():
    """TPEngineGroup puts the adapter name into the "new" spec it
    broadcasts."""
    from dynamo_amd.models.layers import TPContext
    from dynamo_amd.parallel.tp import TPEngineGroup
    e = load_two(make_engine())
    grp = TPEngineGroup(e, TPContext(1, 0))
    grp.add_request("g1", PROMPT, SamplingParams(max_tokens=2), lora="ad1")
    grp.add_request("g0", PROMPT, SamplingParams(max_tokens=2))
    cmd = grp._pending_cmd(step=True)
    assert [r.get("lora") for r in cmd["new"]] == ["ad1", None]


def test_frontend_routes_adapter_model_to_its_worker():
    import httpx
    from dynamo_amd.frontend.openai import build_app
    from dynamo_amd.frontend.service import ModelManager
    from dynamo_amd.runtime import DistributedRuntime, MemoryDiscovery
    from dynamo_amd.workers import WorkerService

    async def main():
        shared = MemoryDiscovery()
        services = []
        for with_adapter in (False, True, False):
            rt = DistributedRuntime(shared)
            ws = WorkerService(make_engine(), rt)
            await ws.start()
            if with_adapter:
                r = await rt.client.call(rt.server.address,
                                         "backend.load_lora",
                                         {"name": "ad1", "rank": 4,
                                          "seed": 11})
                assert r["loras"] == ["ad1"]
            services.append((ws, rt))
        mgr = ModelManager(DistributedRuntime(shared))
        await mgr.start(watch_interval=0.2)
        client = httpx.AsyncClient(
            transport=httpx.ASGITransport(app=build_app(mgr)),
            base_url="http://t")
        models = (await client.get("/v1/models")).json()["data"]
        by_id = {m["id"]: m for m in models}
        assert by_id["ad1"]["parent"] == "tiny-llama"
        assert "parent" not in by_id["tiny-llama"]
        body = {"prompt": "hello adapters", "max_tokens": 5}
        outs = []
        for _ in range(3):      # every one must land on the adapter's worker
            r = await client.post("/v1/completions",
                                  json=dict(body, model="ad1"))
            assert r.status_code == 200, r.text
            outs.append(r.json()["choices"][0]["token_ids"])
        rb = await client.post("/v1/completions",
                               json=dict(body, model="tiny-llama"))
        assert rb.status_code == 200, rb.text
        served = [sum(1 for q in ws.engine.requests.values() if q.lora)
                  for ws, _ in services]
        await client.aclose()
        await mgr.stop()
        for ws, rt in services:
            await ws.stop()
            await rt.shutdown(drain=False)
        return outs, rb.json()["choices"][0]["token_ids"], served

    outs, base, served = _loop_run(main())
    assert served == [0, 3, 0]
    assert outs[0] == outs[1] == outs[2]
    assert outs[0] != base


def test_router_select_allowed():
    """KvRouter.select(allowed=...) only ever returns a listed instance."""
    from dynamo_amd.router import KvRouter, RouterConfig
    from dynamo_amd.runtime import DistributedRuntime, MemoryDiscovery
    from dynamo_amd.mocker import make_mock_engine
    from dynamo_amd.engine.config import ModelConfig
    from dynamo_amd.workers import WorkerService

    async def main():
        shared = MemoryDiscovery()
        services = []
        for _ in range(3):
            rt = DistributedRuntime(shared)
            ws = WorkerService(make_mock_engine(
                model=ModelConfig(name="mock-model", vocab_size=512)), rt)
            await ws.start()
            services.append((ws, rt))
        rrt = DistributedRuntime(shared)
        await rrt.start()
        router = KvRouter(rrt, "dynamo", "backend",
                          RouterConfig(mode="round_robin"))
        await router.start()
        ids = [i.instance_id for i in router.client.instances()]
        assert len(ids) == 3
        picks = {router.select([1, 2, 3], allowed={ids[1]})
                 for _ in range(6)}
        none = router.select([1, 2, 3], allowed=set())
        free = {router.select([1, 2, 3]) for _ in range(6)}
        await router.stop()
        for ws, rt in services:
            await ws.stop()
            await rt.shutdown(drain=False)
        await rrt.shutdown(drain=False)
        return ids, picks, none, free

    ids, picks, none, free = _loop_run(main())
    assert picks == {ids[1]}
    assert none is None
    assert free == set(ids)
