"""Split-KV multi-query paged attention (csrc/attention_multiquery.hip): the
kernel against the fp64 reference of tests/attention_cases.py (NaN page
tails, diagonal needles, future lures; |out - ref| <= TAU * A[row]), and the
engine's opt-in route against the CPU torch_ref forward of the same model.

The scratch is sized for max_ctx 1100: chunk 512, wave slab 128, 3 chunks.
G = 2 / 4 / 7, 8, 16 launch 1 / 2 / 4 column tiles. Measured on MI355X: worst
err / (TAU * A) 0.717 (the bound is 1.0); engine step max |logit - cpu|
0.01172 with the switch off and 0.01172 with it on.
"""
import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.engine import EngineConfig, LLMEngine, SamplingParams
from dynamo_amd.engine.config import PRESETS
from tests import attention_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HKV = 2
MAX_CTX = 1100
# (q_len, ctx) per sequence; q_len is clipped per G to MQ_MAX_COLS // G
SPECS = (
    # no history; row 0 sees one token; whole columns masked in most slabs
    ((1, 1), (2, 2), (8, 8)),
    # the run straddles a 32-token group, a page, a 64-token tile, a slab
    ((4, 33), (3, 64), (8, 65), (2, 130), (1, 129)),
    # the run straddles the chunk edge: early rows get an empty chunk 1,
    # late rows a 1-3-token chunk
    ((4, 513), (8, 515), (5, 512), (1, 600)),
    # three chunks; mixed lengths in one launch
    ((8, 1030), (2, 1025), (3, 40)),
)


@pytest.mark.parametrize("si", range(len(SPECS)))
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "fp8"))
@pytest.mark.parametrize("ps", (32, 64))
@pytest.mark.parametrize("G", (2, 4, 7, 8, 16))
def test_kernel_matches_fp64_reference(G, ps, fp8, si):
    cap = min(ops.MQ_MAX_Q, ops.MQ_MAX_COLS // G)
    spec = tuple((min(ql, cap), ctx) for ql, ctx in SPECS[si])
    max_q = max(ql for ql, _ in spec)
    case = ac.build_prefill_case(G, HKV, ps, spec, v_transposed=True, fp8=fp8)
    ref, A = ac.prefill_reference(case)

    # the torch_ref path of the op is within the bound, so the inputs are
    # within the reference's reach (float8 cannot be indexed on the CPU; the
    # bf16 copy holds the same values)
    kc, vc = ((case.kcache.to(torch.bfloat16), case.vcache.to(torch.bfloat16))
              if fp8 else (case.kcache, case.vcache))
    cpu = ops.paged_attention_multiquery(
        case.q, kc, vc, case.page_table, case.seq_q_start, case.seq_q_len,
        case.seq_ctx_len, case.scale, None, max_q)
    ac.assert_attention_close(cpu, ref, A, ac.TAU, what="torch_ref")

    assert ops.multiquery_ready([ql for ql, _ in spec], G * HKV, HKV, ac.HD,
                                ps, True, case.kcache.dtype)
    scratch = ops.MultiQueryScratch(case.q.shape[0] + 3, G * HKV, ac.HD,
                                    MAX_CTX, DEV)
    assert (scratch.chunk_tokens, scratch.chunks) == (512, 3)
    scratch.partial.fill_(float("nan"))
    scratch.ml.fill_(float("nan"))
    q, kc, vc, pt, st, ln, cx = case.device_args(DEV)
    got = ops.paged_attention_multiquery(q, kc, vc, pt, st, ln, cx, case.scale,
                                         scratch, max_q)
    torch.cuda.synchronize()
    worst = ac.assert_attention_close(got, ref, A, ac.TAU, what="multiquery")
    print(f"multiquery G{G} ps{ps} fp8={fp8} spec{si}: err/(TAU*A) {worst:.3f}")


def test_binding_rejects_what_the_kernel_cannot_do():
    case = ac.build_prefill_case(8, HKV, 64, ((4, 70),), v_transposed=True)
    scratch = ops.MultiQueryScratch(8, 8 * HKV, ac.HD, MAX_CTX, DEV)
    q, kc, vc, pt, st, ln, cx = case.device_args(DEV)
    with pytest.raises(RuntimeError, match="q_len"):
        ops.paged_attention_multiquery(q, kc, vc, pt, st, ln, cx, case.scale,
                                       scratch, 9)
    with pytest.raises(RuntimeError, match="d-major"):
        ops.paged_attention_multiquery(
            q, kc, vc.transpose(2, 3).contiguous(), pt, st, ln, cx,
            case.scale, scratch, 4)


# -- engine route ---------------------------------------------------------
def _engine(device):
    cfg = EngineConfig(model=PRESETS["tiny-llama-gpu"], device=device,
                       max_num_seqs=4, max_batched_tokens=71,
                       max_model_len=1024, kv_pool_pages=32, page_size=64,
                       enable_prefix_caching=False, enable_hip_graphs=False)
    return LLMEngine(cfg, seed=3)


def _copy_weights(dst, src):
    for d, s in zip(dst.modules(), src.modules()):
        for name, val in vars(s).items():
            if isinstance(val, torch.Tensor):
                setattr(d, name, val.to(getattr(d, name).device))


def _chunk_step_logits(e):
    """A 70-token prefill of a 75-token prompt, then the step that carries
    its 5-token chunk and one decode row -> (meta, logits of both rows).
    The decode row's sampled tokens are overwritten so that every engine
    sees the same inputs."""
    sp = SamplingParams(max_tokens=8, ignore_eos=True)
    e.add_request("dec", [(5 * i + 1) % 1000 for i in range(20)], sp)
    e.step()
    dec = e.scheduler.running[0]
    dec.output_tokens[-1] = 11
    e.add_request("chunk", [(7 * i + 3) % 1000 for i in range(75)], sp)
    e.step()                                    # decode row + 70 tokens
    dec.output_tokens[-1] = 13
    sched = e.scheduler.schedule()
    assert [s.n_new for s in sched.decodes] == [1]
    assert [s.n_new for s in sched.prefills] == [5]
    with torch.inference_mode():
        ids, meta = e.runner.prepare(sched)
        h = e.runner.model.forward(ids, e.runner.kv_pool, meta)
        logits = e.runner.model.compute_logits(h[meta.logits_rows]).float()
    assert logits.shape[0] == 2
    return meta, logits.cpu()


def test_engine_route_matches_cpu_forward():
    ops.set_multiquery_attn(False)
    try:
        off = _engine(DEV)
        meta_off, lg_off = _chunk_step_logits(off)
        assert meta_off.prefill_multiquery is None
        assert off.runner.multiquery_scratch is None
        cpu = _engine("cpu")
        _copy_weights(cpu.runner.model, off.runner.model)
        _, lg_cpu = _chunk_step_logits(cpu)

        ops.set_multiquery_attn(True)
        on = _engine(DEV)
        _copy_weights(on.runner.model, off.runner.model)
        meta_on, lg_on = _chunk_step_logits(on)
        assert meta_on.prefill_multiquery is not None
        assert meta_on.prefill_multiquery[0] == 5
        assert meta_on.prefill_tiles is None

        # both GPU paths carry the same bf16 roundings in another order: the
        # switch-on path may be twice as far from the CPU forward as the
        # switch-off path is
        d_off = float((lg_off - lg_cpu).abs().max())
        d_on = float((lg_on - lg_cpu).abs().max())
        print(f"max |logit - cpu|: switch off {d_off:.5f}, on {d_on:.5f}")
        assert torch.isfinite(lg_on).all()
        assert d_on <= 2 * d_off

        # a 9-token chunk is past MQ_MAX_Q: the prefill kernel's step
        on.add_request("nine", list(range(100, 109)),
                       SamplingParams(max_tokens=2))
        sched = on.scheduler.schedule()
        assert 9 in [s.n_new for s in sched.prefills]
        _, meta9 = on.runner.prepare(sched)
        assert meta9.prefill_multiquery is None
        assert meta9.prefill_tiles is not None
    finally:
        ops.set_multiquery_attn(None)
