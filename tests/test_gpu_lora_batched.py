"""Batched LoRA kernels (csrc/lora.hip: lora_shrink, lora_expand_add) and the
adapter-bank engine on the GPU.

Inputs are seeded bf16: x, y ~ N(0, 1), A, B ~ N(0, std). The accuracy
criterion has no fixed tolerance (as tests/test_gpu_skinny_gemm.py): on the
same tensors e_new = max|kernel - ref| must not exceed 2 * e_lib, where ref is
the float64 formula y + scale_s (x A_s^T) B_s^T on the bf16 inputs and e_lib is
the same error of the library expression the engine-activated path runs,
y + F.linear(F.linear(x, A), B) * scale, which rounds to bf16 three times where
the kernel rounds once.

Bank entries at r >= rank, and the whole of a slot no row names, are NaN in
every case here: anything read from them shows up as a non-finite output.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S_USED = 3                       # slots the rows name; slot 3 is never named
SLOT_PATTERN = (0, 2, -1, 1)     # row i -> SLOT_PATTERN[i % 4]
GUARD = 0x7B7B


def _slot_ranks(R, rank):
    """Per-slot true ranks: the case's rank, the full R, and half the rank
    (2, 24, 32: below one 16-byte piece, whole pieces, whole pieces), then the
    unnamed slot, whose rank says "read me" - only the gather protects it."""
    return [rank, R, max(1, rank // 2), R]


@functools.lru_cache(maxsize=None)
def _case(T, K, N, R, rank, std):
    """Seeded inputs, the float64 reference and the library result; shared
    and read-only."""
    g = torch.Generator(device=DEV)
    g.manual_seed(((T * 131 + K) * 131 + N) * 131 + R + rank + int(std * 1000))

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, device=DEV) * scale).to(
            torch.bfloat16)

    S = S_USED + 1
    x, y = rnd(T, K), rnd(T, N)
    A, B = rnd(S, R, K, scale=std), rnd(S, N, R, scale=std)
    rk = _slot_ranks(R, rank)
    for s in range(S_USED):
        A[s, rk[s]:] = float("nan")
        B[s, :, rk[s]:] = float("nan")
    A[S_USED] = float("nan")
    B[S_USED] = float("nan")
    ranks = torch.tensor(rk, dtype=torch.int32, device=DEV)
    scales = torch.tensor([2.0, 0.5, 1.25, 1.0], device=DEV)
    slots = torch.tensor([SLOT_PATTERN[i % 4] for i in range(T)],
                         dtype=torch.int32, device=DEV)
    ref = y.double().clone()
    lib = y.clone()
    for s in range(S_USED):
        rows = (slots == s).nonzero().flatten()
        if not rows.numel():
            continue
        As, Bs = A[s, :rk[s]], B[s, :, :rk[s]]
        xs, ys = x[rows], y[rows]
        ref[rows] = ys.double() + float(scales[s]) * (
            (xs.double() @ As.double().T) @ Bs.double().T)
        lib[rows] = ys + F.linear(F.linear(xs, As), Bs) * float(scales[s])
    return dict(x=x, y=y, bank=(A, B, ranks, scales), slots=slots, ref=ref,
                lib=lib)


def _kernel(c, y=None, t=None, rows=None):
    """Both kernels on (a row subset of) the case, on a copy of y."""
    x, slots = c["x"], c["slots"]
    y = c["y"].clone() if y is None else y
    if rows is not None:
        x, slots, y = (x[rows].contiguous(), slots[rows].contiguous(),
                       y[rows].contiguous())
    A, B, ranks, scales = c["bank"]
    if t is None:
        t = torch.empty(x.shape[0], A.shape[1], dtype=torch.float32,
                        device=DEV)
    ops.lora_shrink(t, x, A, slots, ranks)
    ops.lora_expand_add(y, t, B, slots, ranks, scales)
    return y


# K: 8 lanes of one wave; one wave + a ragged 8; 1.5 passes of the shrink
# kernel's 256 x 8 block step; the down projection's
KS = (64, 520, 3072, 28672)
NS = (8, 72, 1040)
RRS = ((8, 4), (64, 48), (64, 64))
TS = (1, 3, 16, 67)
# every K x N twice, walking T and (R, rank) at different strides so that each
# value meets each K and each N
SHAPES = sorted({(TS[(i + o) % 4], K, N) + RRS[(i + 2 * o) % 3]
                 for o in (0, 1)
                 for i, (K, N) in enumerate((K, N) for K in KS for N in NS)})


@pytest.mark.parametrize("std", [0.1, 0.02])
@pytest.mark.parametrize("T,K,N,R,rank", SHAPES)
def test_matches_reference(T, K, N, R, rank, std):
    c = _case(T, K, N, R, rank, std)
    out = _kernel(c)
    assert torch.isfinite(out.float()).all(), "read a NaN bank entry"
    e_lib = (c["lib"].double() - c["ref"]).abs().max().item()
    e_new = (out.double() - c["ref"]).abs().max().item()
    print(f"T={T} K={K} N={N} R={R} rank={rank} std={std}: "
          f"e_lib={e_lib:.6g} e_new={e_new:.6g}")
    assert e_new <= 2 * e_lib
    none = (c["slots"] < 0).nonzero().flatten()
    assert torch.equal(out[none], c["y"][none])
    if T > 1:
        assert not torch.equal(out[1], c["y"][1])


def test_shape_table_covers_every_edge():
    assert {s[0] for s in SHAPES} == set(TS)
    assert {s[1] for s in SHAPES} == set(KS)
    assert {s[2] for s in SHAPES} == set(NS)
    assert {s[3:] for s in SHAPES} == set(RRS)
    assert len(SHAPES) <= 24


@pytest.mark.parametrize("T,K,N,R,rank", [(3, 520, 72, 8, 4),
                                          (16, 3072, 1040, 64, 48)])
def test_writes_only_its_rows(T, K, N, R, rank):
    c = _case(T, K, N, R, rank, 0.1)
    pad = 4096                                     # int16 elements: 8 KiB
    ybuf = torch.full((pad + T * N + pad,), GUARD, dtype=torch.int16,
                      device=DEV)
    y = ybuf[pad:pad + T * N].view(torch.bfloat16).view(T, N)
    y.copy_(c["y"])
    tbuf = torch.full((pad + 2 * T * R + pad,), GUARD, dtype=torch.int16,
                      device=DEV)
    t = tbuf[pad:pad + 2 * T * R].view(torch.float32).view(T, R)
    _kernel(c, y=y, t=t)
    torch.cuda.synchronize()
    for buf, n in ((ybuf, T * N), (tbuf, 2 * T * R)):
        assert (buf[:pad] == GUARD).all() and (buf[pad + n:] == GUARD).all()
    assert torch.equal(y, _kernel(c))
    # t itself: rows without an adapter, and columns at r >= the slot's
    # rank, are not written
    rk = _slot_ranks(R, rank)
    traw = tbuf[pad:pad + 2 * T * R].view(T, 2 * R)
    for i, s in enumerate(c["slots"].tolist()):
        r = 0 if s < 0 else rk[s]
        assert (traw[i, 2 * r:] == GUARD).all(), f"t row {i} past rank {r}"


def test_row_invariant_and_deterministic():
    c = _case(16, 3072, 1040, 64, 48, 0.1)
    y16 = _kernel(c)
    assert torch.equal(y16, _kernel(c))
    for i in range(16):
        y1 = _kernel(c, rows=torch.tensor([i], device=DEV))
        assert torch.equal(y1[0], y16[i]), f"row {i} depends on its batch"
    perm = torch.tensor([5, 0, 11, 2, 15, 9, 1, 14, 3, 8, 13, 4, 7, 10, 6, 12],
                        device=DEV)
    assert torch.equal(_kernel(c, rows=perm), y16[perm])


def _precondition_calls():
    c = _case(3, 520, 72, 8, 4, 0.1)
    A, B, ranks, scales = c["bank"]
    x, y, slots = c["x"], c["y"].clone(), c["slots"]
    T, R = 3, 8
    t = torch.zeros(T, R, device=DEV)

    def off8(v):
        """The same values at a base address that is 8 mod 16."""
        buf = torch.empty(v.numel() + 8, dtype=v.dtype, device=DEV)
        out = buf[4 * 2 // v.element_size():][:v.numel()].view(v.shape)
        assert out.data_ptr() % 16 == 8
        return out.copy_(v)

    shrink, expand = ops.hip().lora_shrink, ops.hip().lora_expand_add
    return y, {
        "K % 8": lambda: shrink(t, x[:, :516].contiguous(),
                                A[:, :, :516].contiguous(), slots, ranks),
        "N % 8": lambda: expand(y[:, :68].contiguous(), t,
                                B[:, :68].contiguous(), slots, ranks, scales),
        "R % 8": lambda: shrink(t[:, :4].contiguous(), x,
                                A[:, :4].contiguous(), slots, ranks),
        "x misaligned": lambda: shrink(t, off8(x), A, slots, ranks),
        "A misaligned": lambda: shrink(t, x, off8(A), slots, ranks),
        "y misaligned": lambda: expand(off8(y), t, B, slots, ranks, scales),
        "x strided": lambda: shrink(t, c["x"].repeat(1, 2)[:, :520], A, slots,
                                    ranks),
        "y strided": lambda: expand(y.repeat(1, 2)[:, :72], t, B, slots, ranks,
                                    scales),
        "slots int64": lambda: shrink(t, x, A, slots.long(), ranks),
        "slots short": lambda: expand(y, t, B, slots[:2], ranks, scales),
        "T = 0": lambda: shrink(t[:0], x[:0], A, slots[:0], ranks),
    }, t


@pytest.mark.parametrize("name", [
    "K % 8", "N % 8", "R % 8", "x misaligned", "A misaligned", "y misaligned",
    "x strided", "y strided", "slots int64", "slots short", "T = 0"])
def test_preconditions_raise_before_launch(name):
    y, calls, t = _precondition_calls()
    y0 = y.clone()
    with pytest.raises(RuntimeError):
        calls[name]()
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and not t.any(), "launched despite the raise"


def test_cpu_tensors_do_not_reach_the_kernel():
    c = _case(3, 520, 72, 8, 4, 0.1)
    A, B, ranks, scales = c["bank"]
    with pytest.raises(RuntimeError):
        ops.hip().lora_shrink(torch.zeros(3, 8), c["x"].cpu(), A.cpu(),
                              c["slots"].cpu(), ranks.cpu())


# -- engine ---------------------------------------------------------------
PROMPTS = [list(range(10, 150)), list(range(300, 350)), [7] * 200,
           list(range(500, 590))]
MIX = [None, "ad1", "ad2", "ad1"]


def make_engine(max_loras=2, **kw):
    cfg = EngineConfig(model=PRESETS["tiny-llama-gpu"], device="cuda:0",
                       max_num_seqs=8, max_batched_tokens=512,
                       max_model_len=2048, page_size=64, kv_pool_pages=256,
                       enable_prefix_caching=False, max_loras=max_loras,
                       max_lora_rank=16, **kw)
    e = LLMEngine(cfg, seed=7)
    if max_loras:
        e.load_lora("ad1", rank=8, seed=11)
        e.load_lora("ad2", rank=16, seed=12)
    return e


def generate(engine, prompts, loras, tag, max_tokens=8):
    outs = {}
    for i, (p, lo) in enumerate(zip(prompts, loras)):
        kw = {"lora": lo} if lo else {}
        engine.add_request(f"{tag}{i}", p, SamplingParams(max_tokens=max_tokens),
                           **kw)
        outs[f"{tag}{i}"] = []
    steps = 0
    while engine.has_work():
        for so in engine.step():
            outs[so.req_id].append(so.new_token)
        steps += 1
        assert steps < 1000
    return [outs[f"{tag}{i}"] for i in range(len(prompts))]


@pytest.fixture(scope="module")
def graph_engine():
    return make_engine()


@pytest.fixture(scope="module")
def mixed_tokens(graph_engine):
    return generate(graph_engine, PROMPTS, MIX, "m")


def test_engine_mixed_batch_matches_alone_and_eager(graph_engine,
                                                    mixed_tokens):
    e = graph_engine
    assert e.graph_runner is not None and e.graph_runner.use_graphs
    assert (4, True) in e.graph_runner.graphs
    alone = [generate(e, [p], [lo], f"a{i}-")[0]
             for i, (p, lo) in enumerate(zip(PROMPTS, MIX))]
    assert mixed_tokens == alone
    eager = generate(make_engine(enable_hip_graphs=False), PROMPTS, MIX, "e")
    assert mixed_tokens == eager
    # same prompt, different adapter -> different tokens
    same = generate(e, [PROMPTS[0]] * 3, [None, "ad1", "ad2"], "s")
    assert same[0] != same[1] and same[0] != same[2] and same[1] != same[2]


def test_engine_adapter_mix_change_replays_same_graph(graph_engine,
                                                      mixed_tokens):
    e = graph_engine
    generate(e, PROMPTS, MIX, "w")               # bucket 4 with adapters
    n = len(e.graph_runner.graphs)
    other = generate(e, PROMPTS, ["ad2", None, "ad1", "ad2"], "o")
    assert len(e.graph_runner.graphs) == n, "a new adapter mix captured anew"
    want = [generate(e, [p], [lo], f"oa{i}-")[0] for i, (p, lo) in
            enumerate(zip(PROMPTS, ["ad2", None, "ad1", "ad2"]))]
    assert other == want
    # loading and unloading an adapter keeps the captured graphs
    keys = set(e.graph_runner.graphs)
    e.unload_lora("ad2")
    e.load_lora("ad2", rank=16, seed=12)
    assert set(e.graph_runner.graphs) == keys
    assert generate(e, PROMPTS, MIX, "r") == mixed_tokens


def test_engine_base_only_batch_is_the_plain_engine():
    e = make_engine()
    base = generate(e, PROMPTS, [None] * 4, "b")
    assert e.graph_runner.graphs and all(
        not has_lora for _, has_lora in e.graph_runner.graphs)
    plain = generate(make_engine(max_loras=0), PROMPTS, [None] * 4, "p")
    assert base == plain
