"""Logit processors (repetition / presence / frequency penalties, logit_bias,
min_p) without a GPU: the reference semantics against hand-computed rows, the
engine on tiny-llama through the torch-ref op path, TP lockstep over gloo, and
the HTTP front end's plumbing and validation."""
import asyncio
import math
import multiprocessing as mp
import os

import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS
from dynamo_amd.ops import torch_ref
from dynamo_amd.workers.service import make_sampling

NEUTRAL = (1.0, 0.0, 0.0, 0.0, 0.0)
INF = float("inf")


def _params(*rows):
    return torch.tensor(rows, dtype=torch.float32)


def _slots(*s):
    return torch.tensor(s, dtype=torch.int32)


# ---------------------------------------------------------------- semantics
#        token:   0     1     2    3     4    5    6    7
LOGITS = [2.0, -1.0, 0.5, 3.0, -2.0, 1.0, 0.0, 4.0]
# bank words (prompt bit | count << 1): 0 and 4 prompt only, 1 and 5 once in
# the output, 2 in the prompt and three times in the output, 3/6/7 unseen
WORDS = [1, 2, 7, 0, 1, 2, 0, 0]
# r = 2, presence = 0.5, frequency = 0.25, bias {5: +1.5}; by hand:
#   0: 2 / 2 = 1            (prompt only: no frequency / presence)
#   1: -1 * 2 = -2, - (0.25 * 1 + 0.5) = -2.75
#   2: 0.5 / 2 = 0.25, - (0.25 * 3 + 0.5) = -1
#   3: untouched
#   4: -2 * 2 = -4          (prompt only, negative logit)
#   5: 1 / 2 = 0.5, - 0.75 = -0.25, + 1.5 = 1.25
EXPECT = [1.0, -2.75, -1.0, 3.0, -4.0, 1.25, 0.0, 4.0]


def _bank():
    counts = torch.zeros(3, 8, dtype=torch.int32)
    counts[1] = torch.tensor(WORDS, dtype=torch.int32)
    return counts


def _bias(B, rows):
    """CSR from {row: {id: val}}."""
    off, ids, vals = [0], [], []
    for b in range(B):
        for k, v in rows.get(b, {}).items():
            ids.append(k)
            vals.append(v)
        off.append(len(ids))
    return (torch.tensor(off, dtype=torch.int32),
            torch.tensor(ids, dtype=torch.int32),
            torch.tensor(vals, dtype=torch.float32))


def test_reference_penalties_and_bias_by_hand():
    logits = torch.tensor([LOGITS, LOGITS], dtype=torch.float32)
    out = ops.apply_logit_processors(
        logits, _bank(), _slots(1, -1),
        _params((2.0, 0.5, 0.25, 0.0, 0.0), NEUTRAL), _bias(2, {0: {5: 1.5}}))
    assert out is logits
    assert logits[0].tolist() == EXPECT
    assert logits[1].tolist() == LOGITS


def test_reference_each_penalty_alone():
    def one(p):
        lg = torch.tensor([LOGITS], dtype=torch.float32)
        torch_ref.apply_logit_processors(lg, _bank(), _slots(1), _params(p))
        return lg[0].tolist()
    # repetition alone: every seen token, prompt or output
    assert one((2.0, 0, 0, 0, 0)) == [1.0, -2.0, 0.25, 3.0, -4.0, 0.5, 0.0, 4.0]
    # presence alone: output tokens only (1, 2, 5), once each
    assert one((1.0, 0.5, 0, 0, 0)) == [2.0, -1.5, 0.0, 3.0, -2.0, 0.5, 0.0, 4.0]
    # frequency alone: times the output count (1, 3, 1)
    assert one((1.0, 0, 0.25, 0, 0)) == [2.0, -1.25, -0.25, 3.0, -2.0, 0.75,
                                         0.0, 4.0]


def test_reference_min_p_uses_temperature():
    # max 4; T = 2, min_p = 0.25: drop l < 4 + 2 ln 0.25 = 1.2274 -> keeps
    # 3, 1.25 and 4. At T = 1 the cut is 2.6137 and 1.25 goes too.
    for temp, kept in ((2.0, {3, 5, 7}), (1.0, {3, 7})):
        lg = torch.tensor([EXPECT], dtype=torch.float32)
        torch_ref.apply_logit_processors(
            lg, None, _slots(-1), _params((1.0, 0, 0, 0.25, temp)))
        row = lg[0].tolist()
        assert {i for i, x in enumerate(row) if x != -INF} == kept
        assert all(row[i] == EXPECT[i] for i in kept)
    # a greedy row (T = 0) is not filtered
    lg = torch.tensor([EXPECT], dtype=torch.float32)
    torch_ref.apply_logit_processors(
        lg, None, _slots(-1), _params((1.0, 0, 0, 0.25, 0.0)))
    assert lg[0].tolist() == EXPECT


def test_reference_min_p_after_penalties_and_bias():
    # the max is taken after steps 1-3: the bias lifts token 6 to 6.0, so at
    # T = 1, min_p = 0.1 the cut is 6 + ln 0.1 = 3.697 and only 6 and 7 stay
    lg = torch.tensor([LOGITS], dtype=torch.float32)
    torch_ref.apply_logit_processors(
        lg, _bank(), _slots(1), _params((2.0, 0.5, 0.25, 0.1, 1.0)),
        _bias(1, {0: {6: 6.0}}))
    assert lg[0].tolist() == [-INF] * 6 + [6.0, 4.0]


def test_reference_neutral_row_bit_identical():
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(3, 8, generator=g)
    logits[1, 2] = -0.0
    before = logits.clone()
    torch_ref.apply_logit_processors(
        logits, _bank(), _slots(1, 1, -1), _params(NEUTRAL, NEUTRAL, NEUTRAL),
        _bias(3, {}))
    assert torch.equal(logits.view(torch.int32), before.view(torch.int32))


def test_reference_fold():
    counts = torch.zeros(3, 8, dtype=torch.int32)
    #            slot token prompt
    entries = [(1, 0, 1), (1, 4, 1), (1, 2, 1), (1, 2, 1), (1, 1, 0),
               (1, 2, 0), (1, 2, 0), (1, 2, 0), (1, 5, 0),
               (1, 8, 0), (3, 1, 0), (-1, 1, 1)]   # out of range: skipped
    e = torch.tensor(entries, dtype=torch.int32).t().contiguous()
    ops.penalty_fold(counts, e[0], e[1], e[2])
    assert counts[1].tolist() == WORDS
    assert not counts[0].any() and not counts[2].any()


def test_logit_bias_keys_normalise_and_out_of_vocab_raises():
    sp = SamplingParams(logit_bias={"17": 2, 3: -1.5})
    assert sp.logit_bias == {17: 2.0, 3: -1.5}
    assert all(type(k) is int for k in sp.logit_bias)
    # the sampling.__dict__ round trip TP ranks and replay use
    from dynamo_amd.parallel.tp import _make_sp
    import json
    back = _make_sp(json.loads(json.dumps(sp.__dict__)))
    assert back == sp
    assert SamplingParams().logit_bias == {}

    eng = make_engine()
    V = PRESETS["tiny-llama"].vocab_size
    with pytest.raises(ValueError, match="logit_bias"):
        eng.add_request("a", [1, 2, 3], SamplingParams(logit_bias={V: 1.0}))
    with pytest.raises(ValueError, match="logit_bias"):
        eng.add_request("b", [1, 2, 3], SamplingParams(logit_bias={-1: 1.0}))
    with pytest.raises(ValueError, match="prompt token"):
        eng.add_request("c", [1, V, 3], SamplingParams(presence_penalty=1.0))
    assert not eng.has_work()


# ------------------------------------------------------------------- engine
def make_engine(**kw):
    cfg = dict(model=PRESETS["tiny-llama"], device="cpu", max_num_seqs=8,
               max_batched_tokens=128, max_model_len=512, kv_pool_pages=64,
               page_size=16)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), seed=7)


def generate(engine, reqs):
    """reqs: [(prompt, SamplingParams)] -> one token list per request."""
    outs = {}
    for i, (p, sp) in enumerate(reqs):
        engine.add_request(f"r{i}", p, sp)
        outs[f"r{i}"] = []
    steps = 0
    while engine.has_work():
        for so in engine.step():
            outs[so.req_id].append(so.new_token)
        steps += 1
        assert steps < 2000
    return [outs[f"r{i}"] for i in range(len(reqs))]


PROMPTS = [list(range(10, 45)), [7] * 29]


@pytest.fixture(scope="module")
def plain():
    """32 greedy tokens of each prompt, no processors."""
    return [generate(make_engine(), [(p, SamplingParams(max_tokens=32))])[0]
            for p in PROMPTS]


def test_forced_token(plain):
    X = 5
    assert X not in plain[0][:8]
    out = generate(make_engine(), [(PROMPTS[0], SamplingParams(
        max_tokens=8, logit_bias={X: 100}))])[0]
    assert out == [X] * 8
    Y = plain[0][0]
    out = generate(make_engine(), [(PROMPTS[0], SamplingParams(
        max_tokens=8, logit_bias={Y: -100}))])[0]
    assert out[0] != Y


@pytest.mark.parametrize("which", [0, 1])
def test_presence_penalty_stops_repeats(plain, which):
    assert len(set(plain[which])) < 32, "the unpenalised run must repeat"
    out = generate(make_engine(), [(PROMPTS[which], SamplingParams(
        max_tokens=32, presence_penalty=1e4))])[0]
    assert len(out) == 32 and len(set(out)) == 32


def _penalised(n=16):
    return SamplingParams(max_tokens=n, frequency_penalty=1.5,
                          repetition_penalty=1.3, logit_bias={9: 3.0})


def test_batch_isolation(plain):
    other = [list(range(100, 140)), [3, 4, 5] * 9]
    dflt = lambda: SamplingParams(max_tokens=16)  # noqa: E731
    alone = generate(make_engine(), [(PROMPTS[0], _penalised())])[0]
    assert alone != plain[0][:16], "the penalties must change this request"
    neighbours = generate(make_engine(), [(other[0], dflt()),
                                          (other[1], dflt())])
    mixed = generate(make_engine(), [(other[0], dflt()),
                                     (PROMPTS[0], _penalised()),
                                     (other[1], dflt())])
    assert mixed[1] == alone
    assert [mixed[0], mixed[2]] == neighbours


def test_preemption_rebuilds_counts():
    """A pool of 7 pages holds both prompts (3 + 4 pages) but not their
    growth: the penalised request is preempted, comes back with a zeroed
    bank row and refolds its tokens."""
    p0 = list(range(100, 145))
    p1 = list(range(10, 45)) + list(range(10, 24))
    ref = generate(make_engine(), [(p1, _penalised(20))])[0]
    eng = make_engine(max_batched_tokens=32, kv_pool_pages=7,
                      enable_prefix_caching=False)
    r0 = eng.add_request("r0", p0, SamplingParams(max_tokens=6))
    r1 = eng.add_request("r1", p1, _penalised(20))
    out = []
    steps = 0
    while eng.has_work():
        out += [so.new_token for so in eng.step() if so.req_id == "r1"]
        steps += 1
        assert steps < 500
    assert r1.num_preemptions > 0
    assert out == ref
    # finished requests gave their rows back
    assert r0.penalty_slot == -1 and r1.penalty_slot == -1
    assert sorted(eng.penalties._free) == list(range(8))


def test_abort_releases_slot():
    eng = make_engine()
    req = eng.add_request("a", PROMPTS[0], _penalised())
    eng.step()
    assert req.penalty_slot >= 0
    eng.abort("a")
    assert req.penalty_slot == -1
    assert sorted(eng.penalties._free) == list(range(8))


def test_defaults_cost_nothing(monkeypatch):
    calls = []
    for name in ("apply_logit_processors", "penalty_fold"):
        monkeypatch.setattr(ops, name,
                            lambda *a, _n=name, **k: calls.append(_n))
    eng = make_engine()
    # min_p on a greedy request is neutral too
    generate(eng, [(PROMPTS[0], SamplingParams(max_tokens=4)),
                   (PROMPTS[1], SamplingParams(max_tokens=4, min_p=0.5)),
                   (PROMPTS[1], SamplingParams(max_tokens=4, temperature=0.8,
                                               top_p=0.9, seed=3))])
    assert calls == []
    assert eng.penalties.counts is None


def test_bias_and_min_p_allocate_no_bank():
    eng = make_engine()
    generate(eng, [(PROMPTS[0], SamplingParams(
        max_tokens=4, temperature=0.7, min_p=0.2, logit_bias={5: 1.0}))])
    assert eng.penalties.counts is None


def test_min_p_restricts_sampling():
    """At a high temperature a sampled request wanders; with min_p = 1 only
    the most likely token survives, so the output is the greedy one."""
    greedy = generate(make_engine(), [(PROMPTS[0], SamplingParams(
        max_tokens=12))])[0]
    hot = SamplingParams(max_tokens=12, temperature=5.0, seed=11)
    assert generate(make_engine(), [(PROMPTS[0], hot)])[0] != greedy
    hot_minp = SamplingParams(max_tokens=12, temperature=5.0, seed=11,
                              min_p=1.0)
    assert generate(make_engine(), [(PROMPTS[0], hot_minp)])[0] == greedy


def test_logprobs_come_from_processed_logits():
    eng = make_engine()
    eng.add_request("a", PROMPTS[0], SamplingParams(
        max_tokens=1, logprobs=2, logit_bias={5: 100.0}))
    so = [s for s in eng.step() if s.new_token is not None][0]
    assert so.new_token == 5
    assert so.logprobs["top"][0][0] == 5
    assert so.logprobs["token_logprob"] > -1e-3


# ----------------------------------------------------------------------- TP
TP_PROMPT = [7, 8, 9] * 20


def _tp_sampling():
    # string keys, as after a JSON round trip
    return SamplingParams(max_tokens=8, frequency_penalty=1.5,
                          logit_bias={"17": 6.0})


def _tp_cfg(**kw):
    return EngineConfig(model=PRESETS["tiny-llama"], device="cpu",
                        dtype="float32", max_num_seqs=4,
                        max_batched_tokens=256, max_model_len=512,
                        kv_pool_pages=128, page_size=16, **kw)


def _tp_rank(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dynamo_amd.parallel import TPEngineGroup, follower_loop
    from dynamo_amd.models.layers import TPContext
    tp = TPContext(world, rank, group=None)
    tp.control_group = dist.new_group(backend="gloo")
    eng = LLMEngine(_tp_cfg(tp_size=world, tp_rank=rank), tp=tp, seed=7)
    if rank == 0:
        group = TPEngineGroup(eng, tp)
        group.add_request("r0", TP_PROMPT, _tp_sampling())
        out = []
        steps = 0
        while group.has_work():
            out += [so.new_token for so in group.step()]
            steps += 1
            assert steps < 200
        group.shutdown()
        q.put(out)
    else:
        follower_loop(eng, tp)
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_tp2_matches_tp1_with_processors():
    eng = LLMEngine(_tp_cfg(), seed=7)
    tp1 = generate(eng, [(TP_PROMPT, _tp_sampling())])[0]
    unprocessed = generate(LLMEngine(_tp_cfg(), seed=7), [(
        TP_PROMPT, SamplingParams(max_tokens=8))])[0]
    assert tp1 != unprocessed
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_rank, args=(r, 2, 29641, q))
             for r in range(2)]
    for p in procs:
        p.start()
    tp2 = q.get(timeout=240)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert tp2 == tp1, f"TP2 {tp2} != TP1 {tp1}"


# ---------------------------------------------------------------- front end
def run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


@pytest.fixture
def seen_options(monkeypatch):
    """sampling_options of every payload a (mock) worker receives."""
    from dynamo_amd.workers import service as ws
    seen = []
    real = ws.make_sampling

    def spy(payload):
        seen.append(dict(payload.get("sampling_options") or {}))
        return real(payload)
    monkeypatch.setattr(ws, "make_sampling", spy)
    return seen


FIELDS = {"repetition_penalty": 1.2, "presence_penalty": 0.5,
          "frequency_penalty": -0.25, "min_p": 0.05,
          "logit_bias": {"11": 4.0, "12": -100}}


def test_fields_reach_the_worker(seen_options):
    import httpx
    from test_e2e_frontend import teardown, with_stack
    from dynamo_amd.frontend.openai import build_app

    async def main():
        shared, services, mgr, client = await with_stack(nworkers=1)
        r = await client.post("/v1/completions", json=dict(
            FIELDS, model="mock-model", prompt="hello", max_tokens=3))
        assert r.status_code == 200, r.text
        r = await client.post("/v1/chat/completions", json=dict(
            FIELDS, model="mock-model", max_tokens=3,
            messages=[{"role": "user", "content": "hi"}]))
        assert r.status_code == 200, r.text
        assert len(seen_options) == 2
        for so in list(seen_options):
            assert {k: so[k] for k in FIELDS} == FIELDS
            sp = make_sampling({"sampling_options": so})
            assert (sp.repetition_penalty, sp.presence_penalty,
                    sp.frequency_penalty, sp.min_p) == (1.2, 0.5, -0.25, 0.05)
            assert sp.logit_bias == {11: 4.0, 12: -100.0}
        # a request without the fields sends none of them
        r = await client.post("/v1/completions", json={
            "model": "mock-model", "prompt": "hello", "max_tokens": 3})
        assert r.status_code == 200
        assert not set(seen_options[-1]) & set(FIELDS)
        assert not make_sampling({"sampling_options": dict(
            seen_options[-1])}).has_logit_processors

        # --request-template defaults; an explicit value wins
        app = build_app(mgr, request_template={
            "model": "mock-model", "frequency_penalty": 0.75,
            "logit_bias": {"3": 1.0}})
        c2 = httpx.AsyncClient(transport=httpx.ASGITransport(app=app),
                               base_url="http://t")
        r = await c2.post("/v1/completions", json={"prompt": "hi",
                                                   "max_tokens": 2})
        assert r.status_code == 200, r.text
        assert seen_options[-1]["frequency_penalty"] == 0.75
        assert seen_options[-1]["logit_bias"] == {"3": 1.0}
        r = await c2.post("/v1/completions", json={
            "prompt": "hi", "max_tokens": 2, "frequency_penalty": 0.0})
        assert seen_options[-1]["frequency_penalty"] == 0.0
        await c2.aclose()
        await teardown(services, mgr, client)
    run(main())


BAD = [
    ("frequency_penalty", 2.5),
    ("frequency_penalty", -2.01),
    ("presence_penalty", 3),
    ("presence_penalty", -2.5),
    ("repetition_penalty", 0),
    ("repetition_penalty", -1.0),
    ("min_p", 1.5),
    ("min_p", -0.1),
    ("logit_bias", {str(i): 1.0 for i in range(301)}),
    ("logit_bias", {"5": 100.5}),
    ("logit_bias", {"5": -101}),
    ("logit_bias", {"abc": 1.0}),
    ("logit_bias", {"512": 1.0}),      # the mock model's vocabulary is 512
    ("logit_bias", {"-1": 1.0}),
]


def test_validation_answers_400(seen_options):
    from test_e2e_frontend import teardown, with_stack

    async def main():
        shared, services, mgr, client = await with_stack(nworkers=1)
        for field, value in BAD:
            for url, body in (
                    ("/v1/completions", {"prompt": "hi"}),
                    ("/v1/chat/completions",
                     {"messages": [{"role": "user", "content": "hi"}]})):
                r = await client.post(url, json=dict(
                    body, model="mock-model", max_tokens=2, **{field: value}))
                assert r.status_code == 400, (field, value, r.text)
                assert field in r.text
        assert seen_options == []
        # the edges of every range are accepted
        r = await client.post("/v1/completions", json={
            "model": "mock-model", "prompt": "hi", "max_tokens": 2,
            "frequency_penalty": 2, "presence_penalty": -2, "min_p": 1,
            "repetition_penalty": 0.01,
            "logit_bias": dict({str(i): 100 for i in range(299)},
                               **{"511": -100})})
        assert r.status_code == 200, r.text
        await teardown(services, mgr, client)
    run(main())


def test_replay_carries_the_fields():
    from dynamo_amd.tools.replay import _one

    class Client:
        def __init__(self):
            self.bodies = []

        async def post(self, url, json):
            self.bodies.append(json)

            class R:
                status_code = 200

                @staticmethod
                def json():
                    return {"usage": {"completion_tokens": 1}}
            return R()

    sp = SamplingParams(max_tokens=4, **dict(FIELDS))
    c = Client()
    results = []
    run(_one(c, "http://t", {"token_ids": [1, 2], "sampling": sp.__dict__},
             results))
    run(_one(c, "http://t", {"token_ids": [1, 2],
                             "sampling": {"temperature": 0.0}}, results))
    assert {k: c.bodies[0][k] for k in FIELDS} == {
        **FIELDS, "logit_bias": {11: 4.0, 12: -100.0}}
    assert not set(c.bodies[1]) & set(FIELDS)
    assert math.isclose(c.bodies[0]["temperature"], 0.0)


@pytest.mark.timeout(120)
def test_kserve_carries_and_validates_the_fields(seen_options):
    import grpc
    from dynamo_amd.frontend.kserve import MSG, SERVICE, make_grpc_server
    from test_e2e_frontend import teardown, with_stack

    def request(fp32=None, bias=None):
        req = MSG["ModelInferRequest"](model_name="mock-model", id="k1")
        t = req.inputs.add()
        t.name, t.datatype = "text_input", "BYTES"
        t.shape.append(1)
        t.contents.bytes_contents.append(b"hello kserve")
        mt = req.inputs.add()
        mt.name, mt.datatype = "max_tokens", "INT32"
        mt.shape.append(1)
        mt.contents.int_contents.append(3)
        for k, v in (fp32 or {}).items():
            f = req.inputs.add()
            f.name, f.datatype = k, "FP32"
            f.shape.append(1)
            f.contents.fp32_contents.append(v)
        if bias is not None:
            b = req.inputs.add()
            b.name, b.datatype = "logit_bias", "BYTES"
            b.shape.append(1)
            b.contents.bytes_contents.append(bias)
        return req

    async def main():
        shared, services, mgr, client = await with_stack(nworkers=1)
        server, port = make_grpc_server(mgr)
        await server.start()
        try:
            async with grpc.aio.insecure_channel(f"127.0.0.1:{port}") as ch:
                infer = ch.unary_unary(
                    f"/{SERVICE}/ModelInfer",
                    request_serializer=lambda m: m.SerializeToString(),
                    response_deserializer=MSG["ModelInferResponse"].FromString)
                await infer(request(
                    {"repetition_penalty": 1.5, "presence_penalty": 0.5,
                     "frequency_penalty": -0.25, "min_p": 0.125},
                    b'{"11": 4.0, "12": -100}'))
                so = seen_options[-1]
                assert (so["repetition_penalty"], so["presence_penalty"],
                        so["frequency_penalty"], so["min_p"]) == (
                            1.5, 0.5, -0.25, 0.125)
                assert make_sampling({"sampling_options": dict(so)}
                                     ).logit_bias == {11: 4.0, 12: -100.0}
                n = len(seen_options)
                for bad in (request({"frequency_penalty": 2.5}),
                            request({"min_p": 1.5}),
                            request(bias=b'{"512": 1.0}'),
                            request(bias=b"not json")):
                    with pytest.raises(grpc.aio.AioRpcError) as ei:
                        await infer(bad)
                    assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT
                assert len(seen_options) == n
        finally:
            await server.stop(grace=0.2)
            await teardown(services, mgr, client)
    run(main())
