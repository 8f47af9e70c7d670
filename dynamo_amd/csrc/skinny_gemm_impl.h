// Skinny-M (decode-regime) weight GEMM for MI355X/gfx950, shared by the
// production binding (skinny_gemm.hip) and the standalone sweep tool
// (benchmarks/skinny_sweep.hip), which picks (WPB, U, NT) per shape. Two
// kernels: the plain register-streaming one (kept as the reference the
// other must match bit for bit, and as a recorded negative) and the
// row-coalesced one that production runs.
//
//   y[M <= 16, N] = x[M, K] @ W[N, K]^T, bf16 in / bf16 out, fp32 accumulate.
//
// At M <= 16 the GEMM is pure W streaming: every W byte is read once per
// call by exactly one wave. mfma_f32_16x16x32_bf16 with A = x, B = W^T;
// per-lane operand layout (lr = lane & 15, lg = lane >> 4):
//   A-frag: x[lr][k0 + lg*8 .. +8]        one 16 B load, contiguous K
//   B-frag: W[n0 + lr][k0 + lg*8 .. +8]   one 16 B load, contiguous K
// so both operands go straight from global memory to VGPRs: no LDS staging,
// no transpose. A wave owns NT 16-column tiles and a K/WPB slice; U steps of
// loads are in flight per wave. The WPB waves of a block reduce their fp32
// accumulators through LDS in a fixed order (no atomics), so results are
// run-to-run bit-identical and row m does not depend on M.
//
// NTL = 1 loads W with the non-temporal policy (global_load_dwordx4 ... nt):
// W is read once, keeping it out of the caches' way. x stays on the default
// policy: every block re-reads it and it must stay L2-resident. Measured
// cache-cold (benchmarks/skinny_sweep.hip): nt LOSES 3-25 % with this
// kernel's 16 B-per-row access and GAINS 5-12 % with the row-coalesced
// kernel below, which is the one production runs.
#pragma once

#include "common.h"

namespace skinny {

template <int NTL>
DEVINL bf16x8 ldw(const short* p) {
  if constexpr (NTL)
    return __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p));
  else
    return *reinterpret_cast<const bf16x8*>(p);
}

// Requires K % (WPB*32*U) == 0, 1 <= M <= 16, N >= 1. Rows >= M read row 0
// and tile columns >= N read column N-1 (clamped addresses); neither is
// stored.
template <int WPB, int U, int NT, int NTL>
__global__ __launch_bounds__(WPB * 64) void skinny_gemm_kernel(
    const short* __restrict__ x,   // [M, K] bf16 row-major
    const short* __restrict__ w,   // [N, K] bf16 row-major
    short* __restrict__ y,         // [M, N] bf16 row-major
    int M, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;       // 0..WPB-1 = k-slice
  const int lr = lane & 15;
  const int lg = lane >> 4;
  const int n0 = (blockIdx.x * NT) * 16;  // first col of this block's tiles
  if (n0 >= N) return;

  const int kw = K / WPB;                 // K per wave
  const int k0 = wid * kw;
  const int steps = kw / 32;

  const int ar = lr < M ? lr : 0;
  const short* xp = x + (size_t)ar * K + k0 + lg * 8;
  const short* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int col = n0 + t * 16 + lr;
    wp[t] = w + (size_t)(col < N ? col : N - 1) * K + k0 + lg * 8;
  }

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16x8 abuf[U];
  bf16x8 bbuf[NT][U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    abuf[u] = *reinterpret_cast<const bf16x8*>(xp + u * 32);
#pragma unroll
    for (int t = 0; t < NT; t++) bbuf[t][u] = ldw<NTL>(wp[t] + u * 32);
  }

  for (int s = U; s < steps; s += U) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      bf16x8 a = abuf[u];
      abuf[u] = *reinterpret_cast<const bf16x8*>(xp + (s + u) * 32);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        bf16x8 b = bbuf[t][u];
        bbuf[t][u] = ldw<NTL>(wp[t] + (s + u) * 32);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int t = 0; t < NT; t++)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(abuf[u], bbuf[t][u],
                                                       acc[t], 0, 0, 0);

  // Cross-wave reduction: waves 1..WPB-1 park their accumulators in LDS,
  // wave 0 sums them in wave order and writes bf16.
  __shared__ f32x4 red[WPB > 1 ? (WPB - 1) * NT * 64 : 1];
  if (WPB > 1) {
    if (wid > 0) {
#pragma unroll
      for (int t = 0; t < NT; t++)
        red[((wid - 1) * NT + t) * 64 + lane] = acc[t];
    }
    __syncthreads();
    if (wid > 0) return;
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < WPB - 1; r++) {
        f32x4 o = red[(r * NT + t) * 64 + lane];
        acc[t].x += o.x; acc[t].y += o.y; acc[t].z += o.z; acc[t].w += o.w;
      }
  }
  // C layout: lane holds y[lg*4 + i][tilecol + lr], i = 0..3.
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int col = n0 + t * 16 + lr;
    if (col >= N) continue;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int row = lg * 4 + i;
      if (row < M)
        y[(size_t)row * N + col] = f32_to_bf16(acc[t][i]);
    }
  }
}

// Row-coalesced variant: the production kernel. The kernel above reads
// 16 rows x 64 B per load instruction, 16 B per row per quarter-wave. Here
// one instruction reads 8 rows x 128 B (8 consecutive lanes cover one full
// cache line of a row), two instructions cover a
// 16-row x 64-k block = two MFMA steps, and ds_bpermute (LDS crossbar, no
// LDS memory) moves each 16 B slice to the lane the MFMA B operand wants:
// dest lane (n = lane & 15, c = lane >> 4) of step s takes row n, k-chunk
// 4s + c from load (n >> 3), lane 8 (n & 7) + 4s + c. x loads, the order of
// the MFMAs and the reduction are those of skinny_gemm_kernel, so the result
// is bit-identical to it at equal WPB. U2 = 64-k double steps in flight;
// requires K % (WPB*64*U2) == 0. WPB = 1 sums all of K in order in one
// accumulator, which is what hipBLASLt's MT256x16x64 kernel does.
template <int WPB, int U2, int NT, int NTL>
__global__ __launch_bounds__(WPB * 64) void skinny_gemm_coal_kernel(
    const short* __restrict__ x, const short* __restrict__ w,
    short* __restrict__ y, int M, int N, int K) {
  typedef __attribute__((ext_vector_type(4))) int int4v;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int lr = lane & 15;
  const int lg = lane >> 4;
  const int n0 = (blockIdx.x * NT) * 16;
  if (n0 >= N) return;

  const int kw = K / WPB;
  const int k0 = wid * kw;
  const int dsteps = kw / 64;

  const int ar = lr < M ? lr : 0;
  const short* xp = x + (size_t)ar * K + k0 + lg * 8;
  const short* wp[NT][2];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int col = n0 + t * 16 + h * 8 + (lane >> 3);
      wp[t][h] = w + (size_t)(col < N ? col : N - 1) * K + k0 + (lane & 7) * 8;
    }
  const int src0 = (8 * (lr & 7) + lg) * 4;   // byte address of source lane
  const bool hi = lr >= 8;

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16x8 abuf[U2][2];
  bf16x8 rbuf[NT][U2][2];
#pragma unroll
  for (int u = 0; u < U2; u++) {
    abuf[u][0] = *reinterpret_cast<const bf16x8*>(xp + u * 64);
    abuf[u][1] = *reinterpret_cast<const bf16x8*>(xp + u * 64 + 32);
#pragma unroll
    for (int t = 0; t < NT; t++) {
      rbuf[t][u][0] = ldw<NTL>(wp[t][0] + u * 64);
      rbuf[t][u][1] = ldw<NTL>(wp[t][1] + u * 64);
    }
  }

  auto consume = [&](const bf16x8 (&a)[2], const bf16x8& r0, const bf16x8& r1,
                     f32x4& c) {
    const int4v v0 = *reinterpret_cast<const int4v*>(&r0);
    const int4v v1 = *reinterpret_cast<const int4v*>(&r1);
#pragma unroll
    for (int s = 0; s < 2; s++) {
      int4v b;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int t0 = __builtin_amdgcn_ds_bpermute(src0 + s * 16, v0[j]);
        const int t1 = __builtin_amdgcn_ds_bpermute(src0 + s * 16, v1[j]);
        b[j] = hi ? t1 : t0;
      }
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a[s], *reinterpret_cast<const bf16x8*>(&b), c, 0, 0, 0);
    }
  };

  for (int d = U2; d < dsteps; d += U2) {
#pragma unroll
    for (int u = 0; u < U2; u++) {
      bf16x8 a[2] = {abuf[u][0], abuf[u][1]};
      abuf[u][0] = *reinterpret_cast<const bf16x8*>(xp + (d + u) * 64);
      abuf[u][1] = *reinterpret_cast<const bf16x8*>(xp + (d + u) * 64 + 32);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        bf16x8 r0 = rbuf[t][u][0], r1 = rbuf[t][u][1];
        rbuf[t][u][0] = ldw<NTL>(wp[t][0] + (d + u) * 64);
        rbuf[t][u][1] = ldw<NTL>(wp[t][1] + (d + u) * 64);
        consume(a, r0, r1, acc[t]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U2; u++)
#pragma unroll
    for (int t = 0; t < NT; t++)
      consume(abuf[u], rbuf[t][u][0], rbuf[t][u][1], acc[t]);

  __shared__ f32x4 red[WPB > 1 ? (WPB - 1) * NT * 64 : 1];
  if (WPB > 1) {
    if (wid > 0) {
#pragma unroll
      for (int t = 0; t < NT; t++)
        red[((wid - 1) * NT + t) * 64 + lane] = acc[t];
    }
    __syncthreads();
    if (wid > 0) return;
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < WPB - 1; r++) {
        f32x4 o = red[(r * NT + t) * 64 + lane];
        acc[t].x += o.x; acc[t].y += o.y; acc[t].z += o.z; acc[t].w += o.w;
      }
  }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int col = n0 + t * 16 + lr;
    if (col >= N) continue;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int row = lg * 4 + i;
      if (row < M)
        y[(size_t)row * N + col] = f32_to_bf16(acc[t][i]);
    }
  }
}

// The (WPB, U2, NT) points of the row-coalesced kernel the binding can launch.
#define SKINNY_GEMM_COAL_CONFIGS(X)                                         \
  X(8, 1, 2) X(8, 1, 4) X(8, 2, 2) X(4, 2, 2) X(8, 2, 4) X(2, 2, 8)          \
  X(1, 4, 2) X(1, 2, 4) X(1, 4, 4) X(1, 8, 2) X(1, 2, 2) X(1, 1, 8) X(1, 2, 8)

// The (WPB, U, NT) points the sweep measures and the binding can launch.
#define SKINNY_GEMM_CONFIGS(X)                                              \
  X(4, 4, 2) X(4, 4, 4) X(4, 2, 4) X(2, 4, 4) X(2, 8, 4)                    \
  X(1, 8, 4) X(1, 4, 8) X(2, 4, 8) X(4, 8, 2) X(2, 2, 8) X(4, 8, 4)          \
  X(8, 4, 2) X(16, 4, 2) X(16, 2, 2) X(8, 4, 1) X(16, 4, 1) X(8, 2, 4)

}  // namespace skinny
