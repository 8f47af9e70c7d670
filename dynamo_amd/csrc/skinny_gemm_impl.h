// Skinny-M (decode-regime) weight GEMM and fp8 / mxfp4 weight dequantisation for
// MI355X/gfx950, shared by the production binding (skinny_gemm.hip) and the
// standalone sweep tool (benchmarks/skinny_sweep.hip), which picks
// (WPB, U, NT) per shape. One kernel, four weight formats:
//
//   Bf16Plain, Bf16Coal: y[M <= 16, N] = x[M, K] @ W[N, K]^T
//   Fp8Coal (W8A16):     y[M <= 64, N] = (x[M, K] @ bf16(Wq[N, K])^T) * scale[n]
//   Mxfp4Coal (W4A16):   y[M <= 16 MXFP4_GEMM_MAX_MT, N] = x[M, K] @ W_eff^T
//
// x and y bf16, fp32 accumulate. Fp8Coal: Wq holds OCP e4m3 bytes with one
// fp32 scale per output row of W. Every finite e4m3 code is exact in bf16, so
// the conversion loses nothing; the scale is applied once, in fp32, in the
// epilogue. Mxfp4Coal: OCP microscaling FP4, two e2m1 codes per byte (even k
// in the low nibble) and one e8m0 scale byte per 32 consecutive k of a row;
// W_eff = e2m1(code) * 2^(scale - 127) is exact in bf16 (ops/mxfp4_weights.py
// keeps the scale byte in [27, 227] so it is a normal number), the scale is
// applied by the conversion, and there is no epilogue scale.
//
// At these M the GEMM is pure W streaming: every W byte is read once per call
// by exactly one wave. mfma_f32_16x16x32_bf16 with A = x, B = W^T; per-lane
// operand layout (lr = lane & 15, lg = lane >> 4):
//   A-frag: x[lr][k .. k+8]        one 16 B load, contiguous K
//   B-frag: W[n0 + lr][k .. k+8]   8 bf16, contiguous K
// so x goes straight from global memory to VGPRs, and no format stages W in
// LDS memory or transposes it. A wave owns NT 16-column tiles and a K/WPB
// slice; U pipeline steps of loads are in flight per wave. M > 16 runs
// MT = ceil(M/16) accumulator tiles per column tile on the same B fragments:
// W is read once whatever M is. The WPB waves of a block reduce their fp32
// accumulators through LDS in a fixed order (no atomics), so results are
// run-to-run bit-identical and row m does not depend on M. WPB = 1 sums all
// of K in order in one accumulator, which is what hipBLASLt's MT256x16x64
// kernel does for gate/up.
//
// A format says how a wave loads W and how a lane gets its B fragment:
//
// Bf16Plain (kept as the reference Bf16Coal must match bit for bit, and as a
// recorded negative): the lane loads its own B fragment, k = 8 lg, so one
// instruction reads 16 rows x 64 B, 16 B per row per quarter-wave. One
// 32-k MFMA step per pipeline step.
//
// Bf16Coal (production): one instruction reads 8 rows x 128 B (8 consecutive
// lanes cover one full cache line of a row), two instructions cover a 16-row
// x 64-k block = two MFMA steps, and ds_bpermute (LDS crossbar, no LDS
// memory) moves each 16 B slice to the lane the MFMA B operand wants: dest
// lane (n = lr, c = lg) of step s takes row n, k-chunk 4s + c from load
// (n >> 3), lane 8 (n & 7) + 4s + c. x loads, the order of the MFMAs and the
// reduction are those of Bf16Plain, so the result is bit-identical to it at
// equal WPB.
//
// Fp8Coal (production): Bf16Coal with half the bytes per k. A 128 B line of a
// row is now 128 k; two instructions cover a 16-row x 128-k block = four MFMA
// steps, and ds_bpermute moves 8 B slices. Which k a step sums is free as
// long as A and B agree, so the order is chosen to make the register of the
// slice a compile-time constant: step s of dest lane (n, c) takes dwords
// 2(s&1), 2(s&1)+1 of load (n >> 3), lane 8(n & 7) + c + 4(s >> 1), i.e.
// k = 16c + 64(s >> 1) + 8(s & 1) + 0..7 of the 128-k block, and the A
// fragment of that step is read from the same k (16 rows x four 32 B runs:
// full 128 B lines of x as well).
//
// Mxfp4Coal: Fp8Coal with half the bytes per k again. A 128 B line of a row
// is 256 k; two instructions cover a 16-row x 256-k block = eight MFMA steps,
// a source lane's 16 B are exactly one MX block, and ds_bpermute moves one
// dword (8 codes = one B fragment): step s of dest lane (n, c) takes dword
// s & 3 of load (n >> 3), lane 8(n & 7) + c + 4(s >> 2), i.e.
// k = 32(c + 4(s >> 2)) + 8(s & 3) + 0..7 of the 256-k block. Its scale is
// byte c + 4(s >> 2) of the 8 scale bytes of row n for the block: the dest
// lane loads those 8 B itself per step and column tile, on the default cache
// policy (16 lanes x 4 read the same 16 lines), and four
// v_cvt_scalef32_pk_bf16_fp4 turn the dword into the fragment.
//
// NTL = 1 loads W with the non-temporal policy (global_load_dwordx4 ... nt):
// W is read once, keeping it out of the caches' way. x stays on the default
// policy: every block re-reads it and it must stay L2-resident. Measured
// cache-cold (benchmarks/skinny_sweep.hip): nt LOSES 3-25 % with Bf16Plain's
// 16 B-per-row access and GAINS 5-12 % with the row-coalesced one.
#pragma once

#include "common.h"
#include <type_traits>

namespace skinny {

typedef __attribute__((ext_vector_type(4))) int int4v;   // one 16 B W load

template <int NTL>
DEVINL int4v ldw(const void* p) {
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

// 8 packed e2m1 codes (k in nibble order, low nibble first) times 2^(e8m0
// byte - 127) -> 8 bf16: v_cvt_scalef32_pk_bf16_fp4 converts the two codes of
// one byte (op_sel picks the byte) and scales by the fp32 operand, here
// exactly the power of two.
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
#if !defined(__HIP_DEVICE_COMPILE__)
DEVINL bf16x8 e2m1x8_to_bf16x8(unsigned int, unsigned int) { return bf16x8{}; }
#else
DEVINL bf16x8 e2m1x8_to_bf16x8(unsigned int w, unsigned int e8m0) {
  const float sc = __uint_as_float(e8m0 << 23);
  const bf16x2 f[4] = {__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0),
                       __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1),
                       __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2),
                       __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3)};
  return *reinterpret_cast<const bf16x8*>(f);
}
#endif

// ---- weight formats --------------------------------------------------------
// KSTEP: k per pipeline step. LOADS: W load instructions per step and column
// tile; load h of a lane reads 16 B at row w_row(lane, h) of the tile,
// k offset w_k(lane). FRAGS: MFMA steps per pipeline step; step s sums
// k = x_k(lane) + x_step(s) + 0..7 per lane, and b_frag(s, r, sel) is its B
// fragment out of the step's loaded registers r, sel = sel(lane) being what
// b_frag needs of the lane. The kernel evaluates it once, ahead of the loop:
// derived inside b_frag it is computed for the loop and again for the drain,
// 2 more VGPRs, which took Fp8Coal <1, 1, 2, MT 4> from 3 waves/SIMD to 2.
// SCALED: the epilogue multiplies by scale[col]. WPACK: k per welem; w_k
// counts welems.
// BLOCK_SCALED: scale is [N, K / 32] bytes; per step and column tile the lane
// loads the Aux (8 B: the step's 8 block scales of row lane & 15) alongside
// W, and b_frag gets it. The other formats' Aux is empty.
struct NoAux {};
struct Bf16Plain {
  typedef short welem;
  typedef float scale_t;
  typedef NoAux Aux;
  struct Sel {};
  static constexpr int KSTEP = 32, LOADS = 1, FRAGS = 1, WPACK = 1;
  static constexpr bool SCALED = false, BLOCK_SCALED = false;
  static DEVINL int w_row(int lane, int) { return lane & 15; }
  static DEVINL int w_k(int lane) { return (lane >> 4) * 8; }
  static DEVINL int x_k(int lane) { return (lane >> 4) * 8; }
  static constexpr int x_step(int) { return 0; }
  static DEVINL Sel sel(int) { return {}; }
  static DEVINL bf16x8 b_frag(int, const int4v (&r)[1], Sel, Aux) {
    return *reinterpret_cast<const bf16x8*>(&r[0]);
  }
};

// The row-coalesced formats: load h covers rows 8h .. 8h+7 of the tile. Dest
// lane (n, c) takes from load n >> 3, lane 8 (n & 7) + c + 4 * chunk, chunk
// counting the 16 B k-chunks past c; ds_bpermute takes the source lane as a
// byte address.
DEVINL int coal_w_row(int lane, int h) { return h * 8 + (lane >> 3); }
struct CoalSel { int src; bool hi; };
DEVINL CoalSel coal_sel(int lane) {
  return {(8 * (lane & 7) + (lane >> 4)) * 4, (lane & 15) >= 8};
}
DEVINL int coal_take(CoalSel l, int chunk, const int4v (&r)[2], int dword) {
  const int t0 = __builtin_amdgcn_ds_bpermute(l.src + chunk * 16, r[0][dword]);
  const int t1 = __builtin_amdgcn_ds_bpermute(l.src + chunk * 16, r[1][dword]);
  return l.hi ? t1 : t0;
}

struct Bf16Coal {
  typedef short welem;
  typedef float scale_t;
  typedef NoAux Aux;
  typedef CoalSel Sel;
  static constexpr int KSTEP = 64, LOADS = 2, FRAGS = 2, WPACK = 1;
  static constexpr bool SCALED = false, BLOCK_SCALED = false;
  static DEVINL int w_row(int lane, int h) { return coal_w_row(lane, h); }
  static DEVINL int w_k(int lane) { return (lane & 7) * 8; }
  static DEVINL int x_k(int lane) { return (lane >> 4) * 8; }
  static constexpr int x_step(int s) { return 32 * s; }
  static DEVINL Sel sel(int lane) { return coal_sel(lane); }
  static DEVINL bf16x8 b_frag(int s, const int4v (&r)[2], Sel l, Aux) {
    int4v b;
#pragma unroll
    for (int j = 0; j < 4; j++) b[j] = coal_take(l, s, r, j);
    return *reinterpret_cast<const bf16x8*>(&b);
  }
};

struct Fp8Coal {
  typedef unsigned char welem;
  typedef float scale_t;
  typedef NoAux Aux;
  typedef CoalSel Sel;
  static constexpr int KSTEP = 128, LOADS = 2, FRAGS = 4, WPACK = 1;
  static constexpr bool SCALED = true, BLOCK_SCALED = false;
  static DEVINL int w_row(int lane, int h) { return coal_w_row(lane, h); }
  static DEVINL int w_k(int lane) { return (lane & 7) * 16; }
  static DEVINL int x_k(int lane) { return (lane >> 4) * 16; }
  static constexpr int x_step(int s) { return 64 * (s >> 1) + 8 * (s & 1); }
  static DEVINL Sel sel(int lane) { return coal_sel(lane); }
  static DEVINL bf16x8 b_frag(int s, const int4v (&r)[2], Sel l, Aux) {
    return e4m3x8_to_bf16x8(coal_take(l, s >> 1, r, 2 * (s & 1)),
                            coal_take(l, s >> 1, r, 2 * (s & 1) + 1));
  }
};

typedef __attribute__((ext_vector_type(2))) unsigned int uint2v;
struct Mxfp4Coal {
  typedef unsigned char welem;   // two e2m1 codes
  typedef unsigned char scale_t; // e8m0, [N, K / 32]
  typedef uint2v Aux;
  struct Sel { CoalSel c; int shift; };
  static constexpr int KSTEP = 256, LOADS = 2, FRAGS = 8, WPACK = 2;
  static constexpr bool SCALED = false, BLOCK_SCALED = true;
  static DEVINL int w_row(int lane, int h) { return coal_w_row(lane, h); }
  static DEVINL int w_k(int lane) { return (lane & 7) * 16; }   // welems
  static DEVINL int x_k(int lane) { return (lane >> 4) * 32; }
  static constexpr int x_step(int s) { return 128 * (s >> 2) + 8 * (s & 3); }
  static DEVINL Sel sel(int lane) { return {coal_sel(lane), (lane >> 4) * 8}; }
  static DEVINL bf16x8 b_frag(int s, const int4v (&r)[2], Sel l, Aux a) {
    return e2m1x8_to_bf16x8(coal_take(l.c, s >> 2, r, s & 3),
                            (a[s >> 2] >> l.shift) & 0xffu);
  }
};

// Requires K % (WPB * F::KSTEP * U) == 0, 1 <= M <= 16 MT, N >= 1. Rows >= M
// read row 0 and tile columns >= N read column N-1 (clamped addresses);
// neither is stored. scale is read only if F::SCALED ([N]) or
// F::BLOCK_SCALED ([N, K / 32]).
//
// GLU = 1 fuses the SwiGLU activation of a gate/up projection: w is [2I, K],
// gate rows first and up rows second, N = 2I, and y is [M, I] =
// silu(gate) * up. NT must be even. A block owns NT/2 column tiles of y; its
// weight tiles 0 .. NT/2-1 are their gate rows and NT/2 .. NT-1 the matching
// up rows at + I, so the lane that holds gate column j in acc[t] holds up
// column I + j in acc[t + NT/2]. The K loop and the reduction are those of
// GLU = 0; the epilogue rounds both sums to bf16 as the plain one does and
// applies silu_mul_bf16, so y has the bits of silu_mul_kernel on the plain
// kernel's result. Requires I % 16 == 0.
template <class F, int WPB, int U, int NT, int MT, int NTL, int GLU = 0>
__global__ __launch_bounds__(WPB * 64) void skinny_gemm_kernel(
    const short* __restrict__ x,               // [M, K] bf16 row-major
    const typename F::welem* __restrict__ w,   // [N, K] row-major
    const typename F::scale_t* __restrict__ scale,
    short* __restrict__ y,                     // [M, N] bf16 row-major
    int M, int N, int K) {
  static_assert(!GLU || NT % 2 == 0, "GLU pairs gate and up tiles");
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;       // 0..WPB-1 = k-slice
  const int lr = lane & 15;
  const int lg = lane >> 4;
  constexpr int NTO = GLU ? NT / 2 : NT;  // column tiles of y per block
  const int NO = GLU ? N / 2 : N;         // columns of y
  const int n0 = (blockIdx.x * NTO) * 16; // first col of this block's tiles
  if (n0 >= NO) return;

  const int kw = K / WPB;                 // K per wave
  const int k0 = wid * kw;
  const int steps = kw / F::KSTEP;

  const short* xp[MT];
#pragma unroll
  for (int m = 0; m < MT; m++) {
    const int row = m * 16 + lr;
    xp[m] = x + (size_t)(row < M ? row : 0) * K + k0 + F::x_k(lane);
  }
  const typename F::welem* wp[NT][F::LOADS];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int h = 0; h < F::LOADS; h++) {
      int col = n0 + (t % NTO) * 16 + F::w_row(lane, h);
      col = col < NO ? col : NO - 1;
      if (GLU && t >= NTO) col += NO;   // the up row of that column
      wp[t][h] = w + (size_t)col * (K / F::WPACK) +
                 k0 / F::WPACK + F::w_k(lane);
    }
  const typename F::scale_t* sp[NT];
  if constexpr (F::BLOCK_SCALED) {
#pragma unroll
    for (int t = 0; t < NT; t++) {
      int col = n0 + (t % NTO) * 16 + lr;
      col = col < NO ? col : NO - 1;
      if (GLU && t >= NTO) col += NO;
      sp[t] = scale + ((size_t)col * K + k0) / 32;
    }
  }

  const typename F::Sel sel = F::sel(lane);

  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int m = 0; m < MT; m++) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16x8 abuf[U][MT][F::FRAGS];
  int4v rbuf[NT][U][F::LOADS];
  typename F::Aux auxbuf[NT][U];
  auto load_x = [&](bf16x8 (&a)[MT][F::FRAGS], int d) {
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int s = 0; s < F::FRAGS; s++)
        a[m][s] = *reinterpret_cast<const bf16x8*>(xp[m] + d * F::KSTEP +
                                                   F::x_step(s));
  };
  auto load_w = [&](int4v (&r)[F::LOADS], typename F::Aux& ax, int t, int d) {
#pragma unroll
    for (int h = 0; h < F::LOADS; h++)
      r[h] = ldw<NTL>(wp[t][h] + d * (F::KSTEP / F::WPACK));
    if constexpr (F::BLOCK_SCALED)
      ax = *reinterpret_cast<const typename F::Aux*>(sp[t] +
                                                     d * (F::KSTEP / 32));
  };
  auto consume = [&](const bf16x8 (&a)[MT][F::FRAGS],
                     const int4v (&r)[F::LOADS], typename F::Aux ax,
                     f32x4 (&c)[MT]) {
#pragma unroll
    for (int s = 0; s < F::FRAGS; s++) {
      const bf16x8 b = F::b_frag(s, r, sel, ax);
#pragma unroll
      for (int m = 0; m < MT; m++)
        c[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m][s], b, c[m],
                                                       0, 0, 0);
    }
  };

  // U steps in flight: each main-loop step takes its registers, issues the
  // loads of step d + u into them and then runs the MFMAs of the taken ones.
#pragma unroll
  for (int u = 0; u < U; u++) {
    load_x(abuf[u], u);
#pragma unroll
    for (int t = 0; t < NT; t++) load_w(rbuf[t][u], auxbuf[t][u], t, u);
  }
  for (int d = U; d < steps; d += U) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      bf16x8 a[MT][F::FRAGS];
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int s = 0; s < F::FRAGS; s++) a[m][s] = abuf[u][m][s];
      load_x(abuf[u], d + u);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        int4v r[F::LOADS];
#pragma unroll
        for (int h = 0; h < F::LOADS; h++) r[h] = rbuf[t][u][h];
        const typename F::Aux ax = auxbuf[t][u];
        load_w(rbuf[t][u], auxbuf[t][u], t, d + u);
        consume(a, r, ax, acc[t]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int t = 0; t < NT; t++)
      consume(abuf[u], rbuf[t][u], auxbuf[t][u], acc[t]);

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
  if constexpr (GLU) {
#pragma unroll
    for (int t = 0; t < NTO; t++) {
      const int col = n0 + t * 16 + lr;
      if (col >= NO) continue;
      float sg = 1.f, su = 1.f;
      if constexpr (F::SCALED) { sg = scale[col]; su = scale[col + NO]; }
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int row = m * 16 + lg * 4 + i;
          if (row < M) {
            float g = acc[t][m][i], u = acc[t + NTO][m][i];
            if constexpr (F::SCALED) { g *= sg; u *= su; }
            y[(size_t)row * NO + col] =
                silu_mul_bf16(f32_to_bf16(g), f32_to_bf16(u));
          }
        }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int col = n0 + t * 16 + lr;
    if (col >= N) continue;
    float sc = 1.f;
    if constexpr (F::SCALED) sc = scale[col];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int row = m * 16 + lg * 4 + i;
        if (row < M) {
          float v = acc[t][m][i];
          if constexpr (F::SCALED) v *= sc;
          y[(size_t)row * N + col] = f32_to_bf16(v);
        }
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

// out[n, k] = bf16(W_eff[n, k]); one thread converts one 32-k MX block (one
// 16 B load, one scale byte, four 16 B stores). Requires K % 32 == 0.
__global__ __launch_bounds__(256) void mxfp4_dequant_kernel(
    short* __restrict__ out, const unsigned char* __restrict__ q,
    const unsigned char* __restrict__ scale, long long blocks) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= blocks) return;
  const unsigned int e = scale[i];
  const int4v v = *reinterpret_cast<const int4v*>(q + i * 16);
  bf16x8* op = reinterpret_cast<bf16x8*>(out + i * 32);
#pragma unroll
  for (int j = 0; j < 4; j++) op[j] = e2m1x8_to_bf16x8((unsigned int)v[j], e);
}

// The (WPB, U, NT) points the sweep measures and the binding can launch, per
// format; U counts steps of F::KSTEP k.
#define SKINNY_GEMM_CONFIGS(X) /* Bf16Plain */                              \
  X(4, 4, 2) X(4, 4, 4) X(4, 2, 4) X(2, 4, 4) X(2, 8, 4)                    \
  X(1, 8, 4) X(1, 4, 8) X(2, 4, 8) X(4, 8, 2) X(2, 2, 8) X(4, 8, 4)          \
  X(8, 4, 2) X(16, 4, 2) X(16, 2, 2) X(8, 4, 1) X(16, 4, 1) X(8, 2, 4)

#define SKINNY_GEMM_COAL_CONFIGS(X) /* Bf16Coal */                          \
  X(8, 1, 2) X(8, 1, 4) X(8, 2, 2) X(4, 2, 2) X(8, 2, 4) X(2, 2, 8)          \
  X(1, 4, 2) X(1, 2, 4) X(1, 4, 4) X(1, 8, 2) X(1, 2, 2) X(1, 1, 8) X(1, 2, 8)

// Fp8Coal, each for MT = 1..4. (1, 1, *) accept every K % 128 == 0.
#define FP8_GEMM_CONFIGS(X)                                                 \
  X(1, 1, 1) X(1, 1, 2) X(1, 2, 2) X(2, 1, 4) X(2, 2, 2)                     \
  X(4, 1, 2) X(4, 2, 2) X(4, 1, 4) X(8, 1, 2) X(8, 2, 2)

// Mxfp4Coal, each for MT = 1..MXFP4_GEMM_MAX_MT. (1, 1, *) accept every
// K % 256 == 0. With FRAGS = 8 the A fragments alone are 32 U MT VGPRs:
// MT = 2 (M <= 32) is the largest at which no point of the table uses
// scratch; at MT = 3 and 4 (8, 1, 4) spills 60 and 220 B per lane and most
// others run 1 wave/SIMD out of AGPR copies (profiles/README.md, "MXFP4
// weights").
#define MXFP4_GEMM_CONFIGS(X)                                               \
  X(1, 1, 1) X(1, 1, 2) X(1, 2, 2) X(2, 1, 2) X(2, 1, 4) X(4, 1, 2)          \
  X(4, 1, 4) X(4, 1, 8) X(8, 1, 2) X(8, 1, 4) X(2, 1, 8)
#define MXFP4_GEMM_MAX_MT 2

// Whether point (WPB, U, NT) of format F's table has a GLU = 1 form: the
// row-coalesced formats at even NT, but for Bf16Coal (8, 1, 4), the one point
// whose GLU form would run fewer waves per SIMD than its plain twin (136
// against 99 VGPRs, 3 against 4 waves). ops/__init__.py keeps a copy.
template <class F>
constexpr bool glu_capable(int wpb, int u, int nt) {
  if (std::is_same<F, Bf16Plain>::value || nt % 2) return false;
  return !(std::is_same<F, Bf16Coal>::value && wpb == 8 && u == 1 && nt == 4);
}

}  // namespace skinny
