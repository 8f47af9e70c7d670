"""ops.linear_silu_mul without a GPU, and the Python copies of the GEMM
configuration tables' GLU-capable entries (csrc/skinny_gemm_impl.h)."""
import os
import re

import torch
import torch.nn.functional as F

from dynamo_amd import ops
from dynamo_amd.ops import torch_ref

HEADER = os.path.join(os.path.dirname(ops.__file__), os.pardir, "csrc",
                      "skinny_gemm_impl.h")


def _header_table(name):
    """The (WPB, U, NT) entries of `#define name(X) ...` in the header."""
    src = open(HEADER).read()
    text = src[src.index("#define " + name + "(X)"):]
    lines = []
    for line in text.split("\n"):
        lines.append(line)
        if not line.rstrip().endswith("\\"):
            break
    return [tuple(map(int, m)) for m in
            re.findall(r"X\((\d+), (\d+), (\d+)\)", "\n".join(lines))]


def test_linear_silu_mul_on_cpu_is_the_reference():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 64, generator=g)
    w = torch.randn(96, 64, generator=g) * 0.1
    for xx, ww in ((x, w), (x.bfloat16(), w.bfloat16())):
        assert ops.fused_glu_config(xx, ww) is None
        y = ops.linear_silu_mul(xx, ww)
        assert y.shape == (5, 48)
        assert torch.equal(y, torch_ref.silu_mul(F.linear(xx, ww)))
    for holder in (ops.Fp8Weight, ops.Mxfp4Weight):
        wq = holder.from_tensor(w.bfloat16())
        xb = x.bfloat16()
        assert ops.fused_glu_config(xb, wq) is None
        assert torch.equal(ops.linear_silu_mul(xb, wq),
                           torch_ref.silu_mul(ops.linear(xb, wq)))


def test_switch_and_override(monkeypatch):
    monkeypatch.delenv("DYNAMO_FUSED_GLU", raising=False)
    ops.set_fused_glu(None)
    try:
        assert ops.fused_glu_enabled()
        monkeypatch.setenv("DYNAMO_FUSED_GLU", "0")
        assert not ops.fused_glu_enabled()
        ops.set_fused_glu(True)
        assert ops.fused_glu_enabled()
        ops.set_fused_glu(False)
        monkeypatch.delenv("DYNAMO_FUSED_GLU")
        assert not ops.fused_glu_enabled()
    finally:
        ops.set_fused_glu(None)
    from dynamo_amd import envs
    assert "DYNAMO_FUSED_GLU" in envs.ENV_VARS


def test_python_tables_agree_on_glu_capable_entries():
    tables = {
        "bf16_plain": _header_table("SKINNY_GEMM_CONFIGS"),
        "bf16_coalesced": _header_table("SKINNY_GEMM_COAL_CONFIGS"),
        "fp8": _header_table("FP8_GEMM_CONFIGS"),
        "mxfp4": _header_table("MXFP4_GEMM_CONFIGS"),
    }
    assert len(tables["bf16_coalesced"]) == 13 and len(tables["fp8"]) == 10
    assert tables["fp8"] == list(ops.FP8_GEMM_CONFIGS)
    assert tables["mxfp4"] == list(ops.MXFP4_GEMM_CONFIGS)
    # known points of the Python copy of the rule
    assert ops.glu_capable("bf16_coalesced", (1, 2, 2, True, True))
    assert not ops.glu_capable("bf16_coalesced", (8, 1, 4))
    assert not ops.glu_capable("fp8", (1, 1, 1))
    assert ops.glu_capable("mxfp4", (2, 1, 8))
    assert not any(ops.glu_capable("bf16_plain", c)
                   for c in tables["bf16_plain"])
    # what ships for gate/up can be fused
    assert ops.glu_capable("bf16_coalesced",
                           ops.SKINNY_GEMM_SHAPES[(57344, 8192)])
    for fmt, shapes in (("fp8", ops.FP8_GEMM_SHAPES),
                        ("mxfp4", ops.MXFP4_GEMM_SHAPES)):
        assert all(ops.glu_capable(fmt, c) for c in shapes[(57344, 8192)])
    # the header's rule itself, through the built extension (it loads
    # without a GPU): every entry of every table
    glu = ops.hip().skinny_gemm_glu_configs()
    for fmt, table in tables.items():
        assert set(glu[fmt]) == {c for c in table if ops.glu_capable(fmt, c)}
