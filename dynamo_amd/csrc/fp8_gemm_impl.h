// W8A16 decode weight GEMM and weight dequantisation for MI355X/gfx950,
// shared by the production binding (fp8_gemm.hip) and the standalone sweep
// tool (benchmarks/skinny_sweep.hip).
//
//   y[M <= 64, N] = bf16( (x[M, K] @ bf16(Wq[N, K])^T, fp32 accumulate)
//                         * scale[n] )
//
// x bf16, Wq OCP e4m3 bytes, one fp32 scale per output row of W. Every finite
// e4m3 code is exact in bf16, so the conversion loses nothing; the scale is
// applied once, in fp32, in the epilogue.
//
// The kernel is skinny_gemm_coal_kernel (skinny_gemm_impl.h) with half the
// bytes per k. One load instruction reads 8 rows x 128 B (8 consecutive
// lanes cover one full cache line of a row), which is now 128 k per row;
// two instructions cover a 16-row x 128-k block = four MFMA steps.
// ds_bpermute (LDS crossbar, no LDS memory) moves each 8 B slice to the lane
// the MFMA B operand wants. Which k a step sums is free as long as A and B
// agree, so the order is chosen to make the register of the slice a
// compile-time constant: step s of destination lane (n = lane & 15,
// c = lane >> 4) takes dwords 2(s&1), 2(s&1)+1 of load (n >> 3), lane
// 8(n & 7) + c + 4(s >> 1), i.e. k = 16c + 64(s >> 1) + 8(s & 1) + 0..7 of
// the 128-k block, and the A fragment of that step is read from the same k
// (16 rows x four 32 B runs: full 128 B lines of x as well).
//
// M > 16 runs MT = ceil(M/16) accumulator tiles per column tile on the same
// converted W registers: W is read once whatever M is. The WPB waves of a
// block own a K/WPB slice each and reduce through LDS in a fixed order (no
// atomics): results are run-to-run bit-identical and row m does not depend
// on M. U = 128-k steps in flight per wave; requires K % (WPB*128*U) == 0.
#pragma once

#include "common.h"

namespace fp8gemm {

typedef __attribute__((ext_vector_type(4))) int int4v;

template <int NTL>
DEVINL int4v ldw(const unsigned char* p) {
  if constexpr (NTL)
    return __builtin_nontemporal_load(reinterpret_cast<const int4v*>(p));
  else
    return *reinterpret_cast<const int4v*>(p);
}

// 8 packed e4m3 bytes -> 8 bf16 (MFMA B fragment): v_cvt_pk_f32_fp8, then
// keep the upper half of each fp32 (v_perm_b32). An e4m3 value has 3 mantissa
// bits, so the truncation is exact.
#if !defined(__HIP_DEVICE_COMPILE__)
// host pass only parses kernel bodies; device builtins are unavailable
DEVINL bf16x8 e4m3x8_to_bf16x8(int, int) { return bf16x8{}; }
#else
DEVINL bf16x8 e4m3x8_to_bf16x8(int w0, int w1) {
  const float2v f[4] = {__builtin_amdgcn_cvt_pk_f32_fp8(w0, false),
                        __builtin_amdgcn_cvt_pk_f32_fp8(w0, true),
                        __builtin_amdgcn_cvt_pk_f32_fp8(w1, false),
                        __builtin_amdgcn_cvt_pk_f32_fp8(w1, true)};
  unsigned int out[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float lo = f[i].x, hi = f[i].y;   // k, k + 1
    out[i] = __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo),
                                   0x07060302u);
  }
  return *reinterpret_cast<bf16x8*>(out);
}
#endif

// Rows >= M read row 0 and tile columns >= N read column N-1 (clamped
// addresses); neither is stored.
template <int WPB, int U, int NT, int MT, int NTL>
__global__ __launch_bounds__(WPB * 64) void fp8_skinny_gemm_kernel(
    const short* __restrict__ x,           // [M, K] bf16 row-major
    const unsigned char* __restrict__ w,   // [N, K] e4m3 row-major
    const float* __restrict__ scale,       // [N]
    short* __restrict__ y,                 // [M, N] bf16 row-major
    int M, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;       // 0..WPB-1 = k-slice
  const int lr = lane & 15;
  const int lg = lane >> 4;
  const int n0 = (blockIdx.x * NT) * 16;  // first col of this block's tiles
  if (n0 >= N) return;

  const int kw = K / WPB;                 // K per wave
  const int k0 = wid * kw;
  const int dsteps = kw / 128;

  const short* xp[MT];
#pragma unroll
  for (int m = 0; m < MT; m++) {
    const int row = m * 16 + lr;
    xp[m] = x + (size_t)(row < M ? row : 0) * K + k0 + lg * 16;
  }
  const unsigned char* wp[NT][2];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int col = n0 + t * 16 + h * 8 + (lane >> 3);
      wp[t][h] = w + (size_t)(col < N ? col : N - 1) * K + k0 + (lane & 7) * 16;
    }
  const int src0 = (8 * (lr & 7) + lg) * 4;   // byte address of source lane
  const bool hi = lr >= 8;

  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int m = 0; m < MT; m++) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  // x of step s: k = 16 lg + 64 (s >> 1) + 8 (s & 1) of the 128-k block
  bf16x8 abuf[U][MT][4];
  int4v rbuf[NT][U][2];
  auto load_x = [&](bf16x8 (&a)[MT][4], int d) {
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int s = 0; s < 4; s++)
        a[m][s] = *reinterpret_cast<const bf16x8*>(
            xp[m] + d * 128 + 64 * (s >> 1) + 8 * (s & 1));
  };
#pragma unroll
  for (int u = 0; u < U; u++) {
    load_x(abuf[u], u);
#pragma unroll
    for (int t = 0; t < NT; t++) {
      rbuf[t][u][0] = ldw<NTL>(wp[t][0] + u * 128);
      rbuf[t][u][1] = ldw<NTL>(wp[t][1] + u * 128);
    }
  }

  auto consume = [&](const bf16x8 (&a)[MT][4], const int4v& v0,
                     const int4v& v1, f32x4 (&c)[MT]) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
      int b[2];
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int r = 2 * (s & 1) + j;
        const int t0 = __builtin_amdgcn_ds_bpermute(src0 + (s >> 1) * 16, v0[r]);
        const int t1 = __builtin_amdgcn_ds_bpermute(src0 + (s >> 1) * 16, v1[r]);
        b[j] = hi ? t1 : t0;
      }
      const bf16x8 bf = e4m3x8_to_bf16x8(b[0], b[1]);
#pragma unroll
      for (int m = 0; m < MT; m++)
        c[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m][s], bf, c[m],
                                                       0, 0, 0);
    }
  };

  for (int d = U; d < dsteps; d += U) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      bf16x8 a[MT][4];
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int s = 0; s < 4; s++) a[m][s] = abuf[u][m][s];
      load_x(abuf[u], d + u);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int4v r0 = rbuf[t][u][0], r1 = rbuf[t][u][1];
        rbuf[t][u][0] = ldw<NTL>(wp[t][0] + (d + u) * 128);
        rbuf[t][u][1] = ldw<NTL>(wp[t][1] + (d + u) * 128);
        consume(a, r0, r1, acc[t]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int t = 0; t < NT; t++)
      consume(abuf[u], rbuf[t][u][0], rbuf[t][u][1], acc[t]);

  // Cross-wave reduction, one M tile at a time so the LDS footprint does
  // not grow with MT: waves 1..WPB-1 park their accumulators, wave 0 sums
  // them in wave order.
  __shared__ f32x4 red[WPB > 1 ? (WPB - 1) * NT * 64 : 1];
  if (WPB > 1) {
#pragma unroll
    for (int m = 0; m < MT; m++) {
      if (m > 0) __syncthreads();
      if (wid > 0) {
#pragma unroll
        for (int t = 0; t < NT; t++)
          red[((wid - 1) * NT + t) * 64 + lane] = acc[t][m];
      }
      __syncthreads();
      if (wid == 0) {
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
          for (int r = 0; r < WPB - 1; r++) {
            f32x4 o = red[(r * NT + t) * 64 + lane];
            acc[t][m].x += o.x; acc[t][m].y += o.y;
            acc[t][m].z += o.z; acc[t][m].w += o.w;
          }
      }
    }
    if (wid > 0) return;
  }
  // C layout: lane holds y[16 m + lg*4 + i][tilecol + lr], i = 0..3.
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int col = n0 + t * 16 + lr;
    if (col >= N) continue;
    const float sc = scale[col];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int row = m * 16 + lg * 4 + i;
        if (row < M)
          y[(size_t)row * N + col] = f32_to_bf16(acc[t][m][i] * sc);
      }
  }
}

// out[n, k] = bf16_rne(float(wq[n, k]) * scale[n]); one thread converts
// 16 consecutive k (one 16 B load, two 16 B stores). Requires K % 16 == 0.
__global__ __launch_bounds__(256) void fp8_dequant_kernel(
    short* __restrict__ out, const unsigned char* __restrict__ wq,
    const float* __restrict__ scale, long long N, long long K) {
  const long long chunks = K / 16;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * chunks) return;
  const long long row = i / chunks;
  const float sc = scale[row];
  const int4v v = *reinterpret_cast<const int4v*>(wq + i * 16);
  short8 o[2];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float2v lo = __builtin_amdgcn_cvt_pk_f32_fp8(v[j], false);
    const float2v hi = __builtin_amdgcn_cvt_pk_f32_fp8(v[j], true);
    o[j >> 1][(j & 1) * 4 + 0] = f32_to_bf16(lo.x * sc);
    o[j >> 1][(j & 1) * 4 + 1] = f32_to_bf16(lo.y * sc);
    o[j >> 1][(j & 1) * 4 + 2] = f32_to_bf16(hi.x * sc);
    o[j >> 1][(j & 1) * 4 + 3] = f32_to_bf16(hi.y * sc);
  }
#else
  (void)sc; (void)v;
  o[0] = short8{}; o[1] = short8{};
#endif
  short8* op = reinterpret_cast<short8*>(out + i * 16);
  op[0] = o[0];
  op[1] = o[1];
}

// The (WPB, U, NT) points the binding can launch, each for MT = 1..4.
// (1, 1, *) accept every K % 128 == 0.
#define FP8_GEMM_CONFIGS(X)                                                 \
  X(1, 1, 1) X(1, 1, 2) X(1, 2, 2) X(2, 1, 4) X(2, 2, 2)                     \
  X(4, 1, 2) X(4, 2, 2) X(4, 1, 4) X(8, 1, 2) X(8, 2, 2)

}  // namespace fp8gemm
