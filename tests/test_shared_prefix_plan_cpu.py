"""ops.shared_prefix_plan: the work items of the shared-prefix decode
attention kernel, on small hand-written page lists. chunk 64, page 32 (two
pages per chunk), G = 16, so an item holds R = 4 member rows."""
import pytest
import torch

from dynamo_amd import ops

CHUNK, PS, G = 64, 32, 16
R = ops.SP_MAX_COLS // G

# (page lists, ctx lens, expected items (rows, t_begin, t_end) or None)
CASES = {
    "pair sharing 2 chunks": (
        [[1, 2, 3, 4, 5], [1, 2, 3, 4, 6]], [150, 140],
        [((0, 1), 0, 128), ((0,), 128, -1), ((1,), 128, -1)]),
    "R + 1 members split into two prefix items": (
        [[1, 2, 10 + i] for i in range(R + 1)], [70 + i for i in range(R + 1)],
        [((0, 1, 2, 3), 0, 64), ((4,), 0, 64)]
        + [((i,), 64, -1) for i in range(R + 1)]),
    "a run of 1.5 chunks rounds down to 1": (
        [[1, 2, 3, 7], [1, 2, 3, 8]], [100, 120],
        [((0, 1), 0, 64), ((0,), 64, -1), ((1,), 64, -1)]),
    "ctx == run caps the prefix one chunk lower": (
        [[1, 2, 3, 4], [1, 2, 3, 4, 5]], [128, 150],
        [((0, 1), 0, 64), ((0,), 64, -1), ((1,), 64, -1)]),
    "a singleton and a ctx-0 row stay ungrouped": (
        [[1, 2, 3], [9, 10, 11], [1, 2, 4], []], [70, 80, 90, 0],
        [((0, 2), 0, 64), ((0,), 64, -1), ((2,), 64, -1), ((1,), 0, -1),
         ((3,), 0, -1)]),
    "no common first chunk": ([[1, 2, 3], [4, 5, 6]], [70, 70], None),
    "a common chunk that holds the decoded token": (
        [[1, 2], [1, 2]], [64, 64], None),
}


@pytest.mark.parametrize("name", CASES)
def test_plan(name):
    pages, ctxs, want = CASES[name]
    cap = len(pages) + len(pages) // 2
    plan = ops.shared_prefix_plan(pages, ctxs, CHUNK, PS, G, cap)
    if want is None:
        assert plan is None
        return
    rows, rng, max_members = plan
    assert rows.shape == (cap, R) and rng.shape == (cap, 2)
    assert rows.dtype == rng.dtype == torch.int32
    got = []
    for w in range(cap):
        members = tuple(r for r in rows[w].tolist() if r >= 0)
        assert rows[w].tolist() == list(members) + [-1] * (R - len(members))
        if members:
            got.append((members, int(rng[w, 0]), int(rng[w, 1])))
    assert sorted(got) == sorted(want)
    assert max_members == max(len(m) for m, _, _ in want)
    # every (row, chunk) below ctx is written by exactly one item
    for b, ctx in enumerate(ctxs):
        for c0 in range(0, ctx, CHUNK):
            writers = [m for m, t0, t1 in got
                       if b in m and t0 <= c0 < (ctx if t1 < 0 else t1)]
            assert len(writers) == 1, (b, c0, writers)


def test_switch_is_off_by_default(monkeypatch):
    monkeypatch.delenv("DYNAMO_SHARED_PREFIX_ATTN", raising=False)
    monkeypatch.setattr(ops, "_shared_prefix_override", None)
    assert not ops.shared_prefix_attn_enabled()
    monkeypatch.setenv("DYNAMO_SHARED_PREFIX_ATTN", "1")
    assert ops.shared_prefix_attn_enabled()
    ops.set_shared_prefix_attn(False)
    assert not ops.shared_prefix_attn_enabled()
