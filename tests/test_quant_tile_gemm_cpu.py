"""The tiled quantised GEMM's tables, switch and defaults, without a GPU."""
import pytest
import torch

from dynamo_amd import envs, ops
from dynamo_amd.ops import Fp8Weight, Mxfp4Weight

FMTS = ("fp8", "mxfp4")
SKINNY_MAX = {"fp8": ops.FP8_GEMM_MAX_M, "mxfp4": ops.MXFP4_GEMM_MAX_M}


@pytest.mark.parametrize("fmt", FMTS)
def test_tables(fmt):
    points, kstep = ops.TILE_GEMM_CONFIGS[fmt], ops.TILE_GEMM_KSTEP[fmt]
    assert points[0][2] == 1 and points[0][4] == 1   # takes every K % KSTEP
    assert all(bm in (64, 128) and wn * wk <= 8 and nt % 2 == 0
               for bm, wn, wk, nt, u in points)
    for (N, K), entries in ops.TILE_GEMM_SHAPES[fmt].items():
        assert [m for m, _ in entries] == sorted(m for m, _ in entries)
        for _, p in entries:
            assert p in points
            assert K % (p[2] * kstep * p[4]) == 0 and N % 16 == 0
    lo, hi = ops.TILE_GEMM_MIN_M[fmt], ops.TILE_GEMM_MAX_M[fmt]
    assert 17 <= lo <= SKINNY_MAX[fmt] + 1 <= hi
    for N, K in [(48, 2 * kstep), (10240, 8192), (8192, 28672)]:
        assert ops.tile_gemm_config(fmt, lo - 1, N, K) is None
        assert ops.tile_gemm_config(fmt, hi + 1, N, K) is None
        for M in (lo, hi):
            p = ops.tile_gemm_config(fmt, M, N, K)
            assert p in points and K % (p[2] * kstep * p[4]) == 0
    assert ops.tile_gemm_config(fmt, lo, 48, 3 * kstep) == points[0]
    assert ops.tile_gemm_config(fmt, lo, 40, 2 * kstep) is None
    assert ops.tile_gemm_config(fmt, lo, 48, kstep + 32) is None


def test_switch_defaults_off(monkeypatch):
    assert "DYNAMO_QUANT_TILE_GEMM" in envs.ENV_VARS
    monkeypatch.delenv("DYNAMO_QUANT_TILE_GEMM", raising=False)
    monkeypatch.setattr(ops, "_tile_gemm_override", None)
    assert not ops.tile_gemm_enabled()
    monkeypatch.setenv("DYNAMO_QUANT_TILE_GEMM", "1")
    assert ops.tile_gemm_enabled()
    ops.set_tile_gemm(False)
    assert not ops.tile_gemm_enabled()
    ops.set_tile_gemm(None)
    assert ops.tile_gemm_enabled()


@pytest.mark.parametrize("on", [False, True])
def test_cpu_paths_are_untouched(on, monkeypatch):
    monkeypatch.setattr(ops, "_tile_gemm_override", on)
    w = torch.ones(48, 512, dtype=torch.bfloat16)
    x = torch.ones(80, 512, dtype=torch.bfloat16)
    assert ops.fp8_linear_path(x, Fp8Weight.from_tensor(w)) == ("torch", None)
    assert ops.mxfp4_linear_path(x, Mxfp4Weight.from_tensor(w)) == (
        "torch", None)
