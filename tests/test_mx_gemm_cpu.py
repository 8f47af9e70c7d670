"""The MXFP8 activation format (ops/mxfp8.py) and the mx GEMM's dispatch
tables, without a GPU."""
import pytest
import torch

from dynamo_amd import envs, ops
from dynamo_amd.ops import mxfp8


def _rows():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(16, 256, generator=g)
    x[3] = 0
    x[5] *= 2.0 ** 20
    x[7] *= 2.0 ** -20
    x[9, :32] = 0                  # one zero block in a live row
    x[11] *= 2.0 ** -125           # e clamps at -126
    x[13, 1::2] *= 2.0 ** -12      # e4m3 subnormals next to a normal amax
    return x.to(torch.bfloat16)


def test_quantiser_error_bound():
    x = _rows()
    xq, xs = mxfp8.quantize_mxfp8_rows(x)
    assert xq.dtype == torch.float8_e4m3fn and xq.shape == x.shape
    assert xs.dtype == torch.uint8 and xs.shape == (16, 8)
    dq = mxfp8.dequantize_mxfp8_rows(xq, xs, torch.float64)
    e = xs.double() - 127
    bound = torch.maximum(x.double().abs() / 16,
                          (2.0 ** (e - 10)).repeat_interleave(32, dim=1))
    assert ((x.double() - dq).abs() <= bound).all()
    codes = xq.float()
    assert not codes.isnan().any() and codes.abs().max() <= 448
    assert 1 <= int(xs.min()) and int(xs.max()) <= 254


def test_quantiser_exact_cases():
    # powers of two within 2^16 of their block's largest, and zero blocks
    exps = torch.arange(256).view(1, 256) % 16 - 8
    x = torch.cat([2.0 ** exps, -(2.0 ** (exps + 40)), torch.zeros(1, 256)])
    xq, xs = mxfp8.quantize_mxfp8_rows(x.to(torch.bfloat16))
    assert torch.equal(mxfp8.dequantize_mxfp8_rows(xq, xs), x)
    assert (xs[2] == 127).all() and (xq[2].float() == 0).all()
    with pytest.raises(ValueError):
        mxfp8.quantize_mxfp8_rows(torch.zeros(2, 48))


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_dispatch_tables(fmt, monkeypatch):
    assert "DYNAMO_MX_GEMM" in envs.ENV_VARS
    monkeypatch.delenv("DYNAMO_MX_GEMM", raising=False)
    monkeypatch.setattr(ops, "_mx_gemm_override", None)
    assert not ops.mx_gemm_enabled()
    monkeypatch.setenv("DYNAMO_MX_GEMM", "1")
    assert ops.mx_gemm_enabled()
    points, lo = ops.MX_GEMM_CONFIGS[fmt], ops.MX_GEMM_MIN_M[fmt]
    assert lo >= 1 and len(set(points)) == len(points)
    for bm, bn, wm, wn in points:
        assert bm % (16 * wm) == 0 and bn % (32 * wn) == 0 and wm * wn <= 8
    for (N, K), entries in ops.MX_GEMM_SHAPES[fmt].items():
        assert N % 16 == 0 and K % ops.MX_GEMM_KSTEP == 0
        assert [m for m, _ in entries] == sorted(m for m, _ in entries)
        assert all(p in points for _, p in entries)
    assert ops.mx_gemm_config(fmt, lo, 48, 128) in points
    assert ops.mx_gemm_config(fmt, lo - 1, 48, 128) is None
    assert ops.mx_gemm_config(fmt, lo, 40, 128) is None
    assert ops.mx_gemm_config(fmt, lo, 48, 192) is None
    # CPU calls are unchanged whatever the switch says
    holder = ops.Fp8Weight if fmt == "fp8" else ops.Mxfp4Weight
    w = holder.from_tensor(torch.randn(48, 128).to(torch.bfloat16))
    x = torch.randn(lo, 128).to(torch.bfloat16)
    path = ops.fp8_linear_path if fmt == "fp8" else ops.mxfp4_linear_path
    assert path(x, w) == ("torch", None)
    y_on = ops.linear(x, w)
    ops.set_mx_gemm(False)
    assert path(x, w) == ("torch", None)
    assert torch.equal(ops.linear(x, w), y_on)
