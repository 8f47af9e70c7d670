// The main loop of the tiled W8A16 / W4A16 GEMM for MI355X/gfx950, shared by
// the dense kernel (quant_tile_gemm.hip) and the expert-grouped one
// (moe_tile_gemm.hip). A block of WN x WK waves owns BM rows x WN NT 16
// columns; the design - W streams, x through two XOR-swizzled LDS stages,
// order of sums, cross-slice reduction - is described at the head of
// quant_tile_gemm.hip. What a kernel brings:
//
//   the row source  a policy `Rows` that names, per thread, the x row behind
//                   each of its copy passes: valid(i) and ptr(i) for row
//                   cr + i RPP of the slab, i < RP = BM / RPP, where ptr
//                   points at the thread's chunk (cc 8) of that row's k = 0.
//                   An invalid row is zero-filled and never dereferenced.
//   the W slab      w / scale already offset to the weight the block reads,
//                   NO = columns of y, n0 = the wave's first column.
//   the epilogue    tile_gemm_mainloop returns true in the waves of k-slice
//                   0 with the finished accumulators (C layout: acc[t][m][i]
//                   is slab row 16 m + lg 4 + i, column n0 + 16 t + lr; GLU:
//                   tiles t >= NT / 2 are the up tiles of t - NT / 2) and
//                   false in the others, which have nothing more to do.
//
// Every thread of the block must call it: it holds the block's barriers.
#pragma once

#include "skinny_gemm_impl.h"

namespace qtile {

using skinny::int4v;

template <class F, int BM, int WK>
constexpr int kLdsBytes = 2 * WK * BM * F::KSTEP * 2;   // two x stages

// The x copy's geometry: thread tid takes 16 B chunk cc = tid % CPR of slab
// rows cr + RPP i, cr = tid / CPR, in every k-slice.
template <class F, int BM, int WN, int WK>
struct CopyGeom {
  static constexpr int T = WN * WK * 64;
  static constexpr int CPR = F::KSTEP / 8;   // 16 B chunks per slab row
  static constexpr int RPP = T / CPR;        // rows per copy pass
  static constexpr int RP = BM / RPP;        // rows per thread and slice
  static constexpr int CP = WK * RP;         // copy passes per step
  static_assert(T % CPR == 0 && BM % RPP == 0, "a pass stays in one slice");
};

// Built without the packed fp32 VALU forms, as moe_decode.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// Rows m0 .. m0 + BM - 1 of x [M, K]; rows >= M are invalid.
template <class F, int BM, int WN, int WK>
struct DenseRows {
  using G = CopyGeom<F, BM, WN, WK>;
  const short* xc;   // only dereferenced for rows < M
  int left;          // M - (the thread's first row)
  int K;
  DEVINL DenseRows(const short* x, int m0, int M, int K_) : K(K_) {
    const int cr = threadIdx.x / G::CPR, cc = threadIdx.x % G::CPR;
    xc = x + (size_t)(m0 + cr) * K + cc * 8;
    left = M - m0 - cr;
  }
  DEVINL bool valid(int i) const { return i * G::RPP < left; }
  DEVINL const short* ptr(int i) const {
    return xc + (size_t)(i * G::RPP) * K;
  }
};

// Requires K % (WK * F::KSTEP * U) == 0, kLdsBytes of LDS at `lds`. Tile
// columns >= NO read column NO - 1.
template <class F, int BM, int WN, int WK, int NT, int U, int NTL, int GLU,
          class Rows>
DEVINL bool tile_gemm_mainloop(
    f32x4 (&acc)[NT][BM / 16], const Rows& rows,
    const typename F::welem* __restrict__ w,       // [N, K / WPACK]
    const typename F::scale_t* __restrict__ scale, // block scales, if any
    int NO, int K, int n0, char* lds) {
  static_assert(!GLU || NT % 2 == 0, "GLU pairs gate and up tiles");
  static_assert(BM % 16 == 0 && WN * WK <= 8, "at most 512 threads");
  using G = CopyGeom<F, BM, WN, WK>;
  constexpr int MT = BM / 16;
  constexpr int RB = F::KSTEP * 2;          // bytes per slab row
  constexpr int SLAB = BM * RB;             // one k-slice of one stage
  constexpr int STAGE = WK * SLAB;
  constexpr int CPR = G::CPR, RPP = G::RPP, CP = G::CP;
  static_assert(kLdsBytes<F, BM, WK> <= 160 * 1024, "gfx950 LDS");
  static_assert((WK - 1) * WN * NT * MT * 1024 <= kLdsBytes<F, BM, WK>,
                "the parked accumulators fit the x stages");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wn = wid % WN;                // column group
  const int wk = wid / WN;                // k-slice
  const int lr = lane & 15;
  constexpr int NTO = GLU ? NT / 2 : NT;  // column tiles of y per wave

  const int kw = K / WK;                  // K per k-slice
  const int steps = kw / F::KSTEP;

  const typename F::welem* wp[NT][F::LOADS];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int h = 0; h < F::LOADS; h++) {
      int col = n0 + (t % NTO) * 16 + F::w_row(lane, h);
      col = col < NO ? col : NO - 1;
      if (GLU && t >= NTO) col += NO;   // the up row of that column
      wp[t][h] = w + (size_t)col * (K / F::WPACK) +
                 (wk * kw) / F::WPACK + F::w_k(lane);
    }
  const typename F::scale_t* sp[NT];
  if constexpr (F::BLOCK_SCALED) {
#pragma unroll
    for (int t = 0; t < NT; t++) {
      int col = n0 + (t % NTO) * 16 + lr;
      col = col < NO ? col : NO - 1;
      if (GLU && t >= NTO) col += NO;
      sp[t] = scale + ((size_t)col * K + wk * kw) / 32;
    }
  }
  const typename F::Sel sel = F::sel(lane);

#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int m = 0; m < MT; m++) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- the x copy: chunk cc of rows cr + RPP * pass ----
  const int cr = tid / CPR, cc = tid % CPR;
  auto fetch_x = [&](int4v (&v)[CP], int d) {
#pragma unroll
    for (int c = 0; c < CP; c++) {
      const int sl = (c * RPP) / BM;
      v[c] = int4v{0, 0, 0, 0};
      if (rows.valid(c % G::RP))
        v[c] = *reinterpret_cast<const int4v*>(rows.ptr(c % G::RP) + sl * kw +
                                               d * F::KSTEP);
    }
  };
  auto store_x = [&](const int4v (&v)[CP], int stage) {
#pragma unroll
    for (int c = 0; c < CP; c++) {
      const int row = cr + (c * RPP) % BM, sl = (c * RPP) / BM;
      *reinterpret_cast<int4v*>(lds + stage * STAGE + sl * SLAB + row * RB +
                                ((cc ^ (row & 15)) << 4)) = v[c];
    }
  };

  int4v rbuf[NT][U][F::LOADS];
  typename F::Aux auxbuf[NT][U];
  auto load_w = [&](int4v (&r)[F::LOADS], typename F::Aux& ax, int t, int d) {
#pragma unroll
    for (int h = 0; h < F::LOADS; h++)
      r[h] = skinny::ldw<NTL>(wp[t][h] + d * (F::KSTEP / F::WPACK));
    if constexpr (F::BLOCK_SCALED)
      ax = *reinterpret_cast<const typename F::Aux*>(sp[t] +
                                                     d * (F::KSTEP / 32));
  };
  // A fragment of (m, s): one ds_read_b128 at row 16 m + lr, whose
  // r & 15 is lr. x_k / 8 and x_step(s) / 8 have no bit in common.
  const char* abase = lds + wk * SLAB + lr * RB;
  const int ach = F::x_k(lane) / 8;
  auto consume = [&](int stage, const int4v (&r)[NT][F::LOADS],
                     const typename F::Aux (&ax)[NT]) {
#pragma unroll
    for (int s = 0; s < F::FRAGS; s++) {
      bf16x8 b[NT];
#pragma unroll
      for (int t = 0; t < NT; t++) b[t] = F::b_frag(s, r[t], sel, ax[t]);
      const char* ap = abase + stage * STAGE +
                       (((ach + F::x_step(s) / 8) ^ lr) << 4);
#pragma unroll
      for (int m = 0; m < MT; m++) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap + m * 16 * RB);
#pragma unroll
        for (int t = 0; t < NT; t++)
          acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[t],
                                                              acc[t][m],
                                                              0, 0, 0);
      }
    }
  };

  int4v xv[CP];
  fetch_x(xv, 0);
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int t = 0; t < NT; t++) load_w(rbuf[t][u], auxbuf[t][u], t, u);
  store_x(xv, 0);
  __syncthreads();
  for (int d = 0; d < steps; d += U) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int step = d + u;
      const int stage = step & 1;
      const bool more = step + 1 < steps;
      if (more) fetch_x(xv, step + 1);
      int4v r[NT][F::LOADS];
      typename F::Aux ax[NT];
#pragma unroll
      for (int t = 0; t < NT; t++) {
#pragma unroll
        for (int h = 0; h < F::LOADS; h++) r[t][h] = rbuf[t][u][h];
        ax[t] = auxbuf[t][u];
        if (step + U < steps) load_w(rbuf[t][u], auxbuf[t][u], t, step + U);
      }
      consume(stage, r, ax);
      if (more) store_x(xv, stage ^ 1);
      // step's reads of `stage` are done before step + 1 overwrites it
      __syncthreads();
    }
  }

  // Cross-slice reduction in wave order; the x stages are free: the loop's
  // last barrier follows every read of them.
  if constexpr (WK > 1) {
    f32x4* red = reinterpret_cast<f32x4*>(lds);
    if (wk > 0) {
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int m = 0; m < MT; m++)
          red[((((wk - 1) * WN + wn) * NT + t) * MT + m) * 64 + lane] =
              acc[t][m];
    }
    __syncthreads();
    if (wk > 0) return false;
#pragma unroll
    for (int r = 0; r < WK - 1; r++)
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int m = 0; m < MT; m++) {
          const f32x4 o = red[(((r * WN + wn) * NT + t) * MT + m) * 64 + lane];
          acc[t][m].x += o.x; acc[t][m].y += o.y;
          acc[t][m].z += o.z; acc[t][m].w += o.w;
        }
  }
  return true;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace qtile
