// Rope arithmetic shared by the kernels that must agree bit for bit
// (torch-free): rope_append_unit_kernel<0, *> (rope.hip, bf16 pages) and the
// fused prologue of
// paged_decode_mfma_swapped_dmajor_rope (attention_decode_impl.h). This is the
// one copy of the expressions; a kernel that writes its own is a different
// rounding waiting to happen.
#pragma once
#include "common.h"

namespace rope {

// One rope unit: 8 NeoX pairs (x1[i], x2[i]) = (head[i0 + i], head[half + i0
// + i]) of one head, the optional bias added in fp32 first, rotated by
// (c, s) = cos_sin[pos][i0 + i], cos_sin[pos][half + i0 + i] and rounded to
// bf16. `a * c - b * s` leaves the compiler two ways to contract (which
// product is rounded before the fused multiply-add), and it picks by
// context: written through a helper, rope_append_unit_kernel came out with
// the other one and the flagship's tokens changed. So the contraction is
// spelled out, in the form that kernel has always had: the a-products are
// rounded, the b-products fused.
DEVINL void rotate8(const short8& x1, const short8& x2, bool has_bias,
                    const short8& b1, const short8& b2, const float4v& c0,
                    const float4v& c1, const float4v& s0, const float4v& s1,
                    short8& o1, short8& o2) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const float c = (i < 4) ? c0[i] : c1[i - 4];
    const float s = (i < 4) ? s0[i] : s1[i - 4];
    float a = bf16_to_f32(x1[i]);
    float b = bf16_to_f32(x2[i]);
    if (has_bias) {
      a += bf16_to_f32(b1[i]);
      b += bf16_to_f32(b2[i]);
    }
    const float ac = a * c;
    const float as = a * s;
    o1[i] = f32_to_bf16(__builtin_fmaf(-b, s, ac));   // a * c - b * s
    o2[i] = f32_to_bf16(__builtin_fmaf(b, c, as));    // b * c + a * s
  }
}

// 8 v elements plus their bias, rounded to bf16.
DEVINL short8 add_bias8(short8 v, const short8& bv) {
#pragma unroll
  for (int e = 0; e < 8; e++)
    v[e] = f32_to_bf16(bf16_to_f32(v[e]) + bf16_to_f32(bv[e]));
  return v;
}

}  // namespace rope
