"""MoE kernels and `MoEMLP.forward` against fp64 references, on cases where a
misrouted, dropped or unwritten token is an O(1) error.

Cases, references, bounds and mutations live in tests/moe_cases.py;
tests/test_moe_reference_cpu.py shows on the CPU that each bound rejects each
mutation. Here:

* grouped GEMM, tile mode and seg (device-offset) mode, over every case:
  `y` is the first T rows of a [T + 1, N] NaN buffer, every row must be
  finite and within |out - ref| <= 2^-8 |ref| + 2^-12 A, the guard row must
  stay NaN; a tile list without one expert leaves exactly its rows NaN; seg
  mode with max_tokens = T, T + 40 and an expert window whose offsets do not
  start at 0 (rows outside stay NaN); tile and seg mode are bit-equal; T = 0
  returns in both modes. `<2>` (N < 16384), `<4>` (N >= 16384) and, in a
  child process with DYNAMO_MOE_MFMA=0, the VALU kernel.
* gating: every (E, K, T) of the case module, ties, -inf, +-200 included.
* block: the bmm, seg, host-tile (EP) and per-expert-loop routes of
  `MoEMLP.forward` against the fp64 block reference, the routes against each
  other, and graph replay of the bmm and seg routes with changing routings.

Measured on MI355X, worst case per path of this module (the bounds are 1.0
and were never widened; nothing failed on the unchanged kernels):

    grouped GEMM, max err / (2^-8 |ref| + 2^-12 A)
    MOE_RATIO mfma2  0.8525   moe_gemm_mfma_kernel<2>, tiles + seg + window
    MOE_RATIO mfma4  0.8699   moe_gemm_mfma_kernel<4>, tiles + seg + window
    MOE_RATIO valu   0.8525   moe_gemm_kernel, DYNAMO_MOE_MFMA=0 child

    block, max err / (tau_blk * S_row), tau_blk = 0.04958
    bmm 0.178   seg 0.207   seg (DYNAMO_MOE_BMM=0) 0.178   loop 0.250
    EP host tiles 0.171   graph replay bmm 0.152   graph replay seg 0.152
    routes against each other: at most 0.072 tau_blk (bound 2)

The GEMM ratios are the one bf16 output rounding: the fp32 stand-in of the
CPU module shows 0.87 on the same cases.
"""
import os
import subprocess
import sys

import pytest
import torch

from dynamo_amd import ops
from dynamo_amd.models import mixtral
from dynamo_amd.models.layers import TPContext, linear
from dynamo_amd.models.mixtral import MoEMLP
from tests import moe_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

GEMM_PARAMS = mc.gemm_params()
GEMM_IDS = [mc.gemm_id(p) for p in GEMM_PARAMS]


def _gemm_path(N):
    """Name of the kernel moe.hip dispatches to (D % 32 == 0 throughout)."""
    env = os.environ.get("DYNAMO_MOE_MFMA")
    if env is not None and env.startswith("0"):
        return "valu"
    return "mfma4" if N >= 16384 else "mfma2"


def _record(path, worst):
    print(f"MOE_RATIO {path} {worst:.4f}")


def _nan_buffer(T, N):
    """-> (y, guard): y the first T rows of a [T + 1, N] NaN buffer."""
    buf = torch.full((T + 1, N), NAN, dtype=torch.bfloat16, device=DEV)
    return buf[:T], buf[T]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _check_rows(y, guard, case, written, what):
    """Rows in `written` are finite and within the bound, all other rows and
    the guard row are still NaN. Returns the worst ratio."""
    torch.cuda.synchronize()
    assert bool(guard.isnan().all()), f"{what}: guard row written"
    yc = y.float().cpu()
    mask = torch.zeros(case.T, dtype=torch.bool)
    mask[torch.tensor(written, dtype=torch.long)] = True
    assert bool(yc[~mask].isnan().all()), (
        f"{what}: wrote rows outside its tiles: "
        f"{(~yc.isnan().all(-1) & ~mask).nonzero().flatten().tolist()[:8]}")
    return mc.assert_gemm_close(yc[mask], case.ref[mask], case.A[mask], what)


def _tiles_t(tiles):
    return _i32(tiles).view(-1, 3)


# --------------------------------------------------------------------------
# grouped GEMM
# --------------------------------------------------------------------------
@pytest.mark.parametrize("p", GEMM_PARAMS, ids=GEMM_IDS)
def test_grouped_gemm(p):
    _, counts, D, N = p
    case = mc.build_gemm_case(counts, D, N)
    T, E = case.T, case.E
    path = _gemm_path(N)
    x, w = case.x.to(DEV), case.w.to(DEV)
    rows = list(range(T))
    worst = 0.0

    # tile mode, the host tile list
    tiles = ops.build_moe_tiles(list(counts))
    y_tile, guard = _nan_buffer(T, N)
    ops.hip().moe_grouped_gemm(y_tile, x, w, _tiles_t(tiles))
    worst = max(worst, _check_rows(y_tile, guard, case, rows, f"{path} tiles"))

    # tile mode without the tiles of the largest segment: its rows stay NaN
    skip = max(range(E), key=lambda e: counts[e])
    kept = [t for t in tiles if t[0] != skip]
    kept_rows = [r for r in rows if case.expert_of_row[r] != skip]
    y, guard = _nan_buffer(T, N)
    ops.hip().moe_grouped_gemm(y, x, w, _tiles_t(kept))
    worst = max(worst, _check_rows(y, guard, case, kept_rows,
                                   f"{path} tiles without expert {skip}"))

    # seg mode: max_tokens exact, then oversized (surplus m-tiles must exit)
    seg = _i32(case.seg_start)
    for max_tokens in (T, T + 40):
        y, guard = _nan_buffer(T, N)
        ops.hip().moe_grouped_gemm_seg(y, x, w, seg, max_tokens)
        worst = max(worst, _check_rows(y, guard, case, rows,
                                       f"{path} seg max_tokens={max_tokens}"))
        # same kernel body, same m-tiles: bit-equal to tile mode
        assert torch.equal(y, y_tile), f"{path}: seg != tiles"

    # seg mode over an expert window that does not start at row 0, with only
    # the window's weights (what an expert-parallel rank would pass)
    first = next(e for e in range(E) if counts[e])
    lo = first + 1
    if lo < E:
        hi = E - 1 if E - lo >= 2 else E
        assert case.seg_start[lo] > 0
        win_rows = list(range(case.seg_start[lo], case.seg_start[hi]))
        y, guard = _nan_buffer(T, N)
        ops.hip().moe_grouped_gemm_seg(
            y, x, w[lo:hi].contiguous(), _i32(case.seg_start[lo:hi + 1]), T)
        worst = max(worst, _check_rows(y, guard, case, win_rows,
                                       f"{path} seg window [{lo}, {hi})"))
    _record(path, worst)


@pytest.mark.parametrize("D,N", [(640, 136), (128, 16384)])
def test_grouped_gemm_no_tokens(D, N):
    """T = 0: ntiles == 0 / max_tokens == 0 return without a launch."""
    E = 3
    x = torch.empty(0, D, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(E, N, D, dtype=torch.bfloat16, device=DEV)
    y, guard = _nan_buffer(0, N)
    ops.hip().moe_grouped_gemm(
        y, x, w, torch.empty(0, 3, dtype=torch.int32, device=DEV))
    ops.hip().moe_grouped_gemm_seg(y, x, w, _i32([0] * (E + 1)), 0)
    torch.cuda.synchronize()
    assert y.shape == (0, N) and bool(guard.isnan().all())


def test_grouped_gemm_valu_subprocess():
    """DYNAMO_MOE_MFMA is read once per process: a child pytest with
    DYNAMO_MOE_MFMA=0 runs the `<2>`-sized cases on the VALU kernel."""
    env = dict(os.environ, DYNAMO_MOE_MFMA="0")
    out = subprocess.run(
        [sys.executable, "-m", "pytest", "tests/test_gpu_moe.py", "-q", "-s",
         "-k", "test_grouped_gemm and nt2_", "-m", "gpu",
         "-p", "no:cacheprovider"],
        capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    paths = set()
    for line in out.stdout.splitlines():
        if "MOE_RATIO" in line:      # pass the child's measurements on
            line = line[line.index("MOE_RATIO"):]
            print(line)
            paths.add(line.split()[1])
    assert out.returncode == 0, out.stdout[-3000:]
    assert " passed" in out.stdout and "no tests ran" not in out.stdout
    assert paths == {"valu"}, paths


# --------------------------------------------------------------------------
# gating
# --------------------------------------------------------------------------
@pytest.mark.parametrize("E,K,T", mc.gating_params())
def test_topk_gating(E, K, T):
    logits, kinds = mc.gating_logits(E, K, T)
    topw, topi = ops.topk_gating(logits.to(DEV), K)
    torch.cuda.synchronize()
    assert topw.dtype == torch.float32 and topi.dtype == torch.int32
    mc.assert_gating_matches(topw, topi, logits, K, what=f"gpu {kinds}")


# --------------------------------------------------------------------------
# block: MoEMLP.forward
# --------------------------------------------------------------------------
class _Rank(TPContext):
    """One of two expert-parallel "ranks" in one process: the all-reduce is
    the identity and the test sums the partial outputs."""

    def __init__(self, rank):
        super().__init__(tp_size=2, tp_rank=rank)

    def all_reduce(self, x):
        return x


@pytest.fixture(scope="module")
def moe():
    m = MoEMLP(mc.block_config(), TPContext(), DEV, torch.bfloat16)
    mc.load_block_weights(m)
    return m


@pytest.fixture(scope="module")
def moe_ep():
    half = mc.BLK_E // 2
    ranks = []
    for r in range(2):
        m = MoEMLP(mc.block_config(moe_ep=True), _Rank(r), DEV, torch.bfloat16)
        assert m.ep and m.e0 == r * half and m.El == half
        mc.load_block_weights(m, r * half, (r + 1) * half)
        ranks.append(m)
    return ranks


class _Calls:
    """Counts the grouped-GEMM / bmm calls MoEMLP.forward makes, so a test
    knows which route it ran."""

    def __init__(self, monkeypatch):
        self.n = {"seg": 0, "tiles": 0, "bmm": 0}
        for key, mod, name in (("seg", ops, "moe_grouped_gemm_seg"),
                               ("tiles", ops, "moe_grouped_gemm"),
                               ("bmm", torch, "bmm")):
            monkeypatch.setattr(mod, name, self._wrap(key, getattr(mod, name)))

    def _wrap(self, key, fn):
        def counted(*a, **kw):
            self.n[key] += 1
            return fn(*a, **kw)
        return counted

    def route(self):
        live = {k for k, v in self.n.items() if v}
        assert len(live) <= 1 and all(v in (0, 2) for v in self.n.values())
        return live.pop() if live else "loop"


def _set_bmm(monkeypatch, on):
    if on:
        monkeypatch.delenv("DYNAMO_MOE_BMM", raising=False)
    else:
        monkeypatch.setenv("DYNAMO_MOE_BMM", "0")


def _block_ref(m, x):
    """fp64 reference from the router logits of the block's own call."""
    logits = linear(x, m.router).float()
    return mc.block_reference(x.cpu(), logits)


def _forward(m, x):
    with torch.no_grad():
        out = m.forward(x)
    torch.cuda.synchronize()
    return out


def _run_ep(ranks, x):
    return sum(_forward(m, x).double() for m in ranks)


def _record_block(route, T, worst):
    print(f"MOE_BLOCK_RATIO {route} T{T} {worst:.4f}")


@pytest.mark.parametrize("route,bmm_on,T", [
    ("bmm", True, 1), ("bmm", True, 16), ("bmm", True, 64),
    ("seg", True, 65), ("seg", True, 256),
    ("seg", False, 1), ("seg", False, 16), ("seg", False, 64),
    ("loop", True, 257),
], ids=lambda v: str(v))
def test_block_route(moe, monkeypatch, route, bmm_on, T):
    assert mixtral.ops is ops
    _set_bmm(monkeypatch, bmm_on)
    x = mc.block_x(T).to(DEV)
    ref = _block_ref(moe, x)
    calls = _Calls(monkeypatch)
    out = _forward(moe, x)
    assert calls.route() == route
    _record_block(route + ("" if bmm_on else "_bmm0"), T,
                  mc.assert_block_close(out, ref, what=f"{route} T={T}"))


@pytest.mark.parametrize("T", [5, 64])
def test_block_route_ep_tiles(moe_ep, monkeypatch, T):
    """Two expert-parallel ranks, each with its half of the experts: the
    host-tile route; every (token, expert) pair is computed on one rank."""
    _set_bmm(monkeypatch, True)
    x = mc.block_x(T).to(DEV)
    ref = _block_ref(moe_ep[0], x)
    calls = _Calls(monkeypatch)
    out = _run_ep(moe_ep, x)
    assert calls.n == {"seg": 0, "tiles": 4, "bmm": 0}
    _record_block("ep_tiles", T,
                  mc.assert_block_close(out, ref, what=f"ep tiles T={T}"))


@pytest.mark.parametrize("T", [1, 16, 64])
def test_block_routes_agree(moe, moe_ep, monkeypatch, T):
    """bmm, seg and (at T = 64, where the EP route also runs) host tiles
    compute the same block: pairwise within 2 * tau_blk * S_row."""
    x = mc.block_x(T).to(DEV)
    ref = _block_ref(moe, x)
    outs = {}
    _set_bmm(monkeypatch, True)
    outs["bmm"] = _forward(moe, x)
    _set_bmm(monkeypatch, False)
    outs["seg"] = _forward(moe, x)
    if T == 64:
        outs["ep_tiles"] = _run_ep(moe_ep, x)
    s_row = ref.abs().amax(dim=-1, keepdim=True)
    names = sorted(outs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            diff = (outs[a].double().cpu() - outs[b].double().cpu()).abs()
            worst = float((diff / s_row).max()) / mc.tau_blk()
            print(f"MOE_BLOCK_AGREE {a}-{b} T{T} {worst:.4f}")
            assert worst <= 2.0, f"{a} vs {b}: {worst:.3f} tau_blk"


@pytest.mark.parametrize("route,bmm_on", [("bmm", True), ("seg", False)])
def test_block_graph_replay(moe, monkeypatch, route, bmm_on):
    """The routing is computed on the device inside the captured graph: each
    replay with another x must route afresh, not repeat the captured one."""
    T = 16
    _set_bmm(monkeypatch, bmm_on)
    calls = _Calls(monkeypatch)
    xs = [mc.block_x(T, variant=v).to(DEV) for v in range(4)]
    picks = [ops.topk_gating(linear(x, moe.router).float(), mc.BLK_K)[1].cpu()
             for x in xs]
    for i in range(len(xs)):
        for j in range(i + 1, len(xs)):
            assert not torch.equal(picks[i], picks[j]), "routings must differ"
    eager = [_forward(moe, x) for x in xs]
    refs = [_block_ref(moe, x) for x in xs]
    assert calls.n[route] == 2 * len(xs) and sum(calls.n.values()) == 2 * len(xs)

    static_x = xs[0].clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()                  # warm up on a side stream
    with torch.cuda.stream(s), torch.no_grad():
        moe.forward(static_x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        static_out = moe.forward(static_x)
    for v in (1, 2, 3):                      # the capture saw variant 0
        static_x.copy_(xs[v])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager[v]), (
            f"{route}: replay {v} differs from the eager output")
        _record_block(f"graph_{route}", T, mc.assert_block_close(
            static_out, refs[v], what=f"graph {route} replay {v}"))
