// Tiled W8A16 / W4A16 GEMM for MI355X/gfx950: the quantised weight formats of
// skinny_gemm_impl.h (Fp8Coal, Mxfp4Coal) at the M the skinny-M kernel does
// not take - larger decode batches, mixed steps, short prefills.
//   fp8_tile_gemm:   y[M,N] = bf16((x[M,K] @ bf16(wq[N,K])^T) * scale[n])
//   mxfp4_tile_gemm: y[M,N] = x[M,K] @ W_eff[N,K]^T
// x/y bf16, fp32 accumulate, any M >= 1; `glu` as in skinny_gemm.hip.
//
// The skinny kernel holds every A fragment of a pipeline step in VGPRs
// (32 U MT registers for mxfp4) and every block re-reads all of x from L2.
// Here x goes through LDS once per block and an A fragment lives for one
// group of MFMAs, so MT = BM / 16 is bounded by the accumulators alone.
//
// Work split. A block is WN x WK waves and owns BM rows x WN NT 16 columns of
// y. Wave (wn, wk) owns NT column tiles and k-slice wk of K (the skinny
// kernel's WPB): it streams its W rows exactly as the skinny kernel does -
// the formats' row-coalesced 16 B loads, U steps in flight, ds_bpermute to
// the B-fragment lane, convert - and runs MT MFMAs per converted fragment.
// blockIdx.x = column block * mtiles + M tile: the M tiles of one W slab are
// neighbours in launch order, so the slab's second read hits L2.
//
// x through LDS. Per pipeline step the block copies the [BM, KSTEP] slab of
// each of its WK k-slices: thread `tid` takes 16 B chunk tid % CPR of row
// tid / CPR (+ RPP per pass), CPR = KSTEP / 8 chunks per row, so a wave's
// global loads run along full rows. Two stages: the loads of step d + 1 are
// issued before the MFMAs of step d, stored to the other stage after them,
// and one barrier ends the step. Rows >= M are zero-filled and never
// stored; nothing past x + M K is read.
//
// Swizzle. Chunk c of slab row r lives at byte r RB + ((c ^ (r & 15)) << 4),
// RB = 2 KSTEP (256 B fp8, 512 B mxfp4); the XOR touches the low four bits
// of c, so a chunk stays in its 256 B half-row. On paper:
//  - A read, MFMA step s: lane (lr, lg) reads chunk c = (x_k + x_step(s)) / 8
//    of row 16 m + lr. The 16 lanes of one lg share c and have r & 15 = lr,
//    so their slots are c ^ lr, lr = 0..15: all 16 16 B slots of a 256 B bank
//    row, each once. Any aligned 8 of those lanes (lr = 8 h .. 8 h + 7) cover
//    (c ^ lr) & 7 = all 8 slots of a 128 B half. So a ds_read_b128 is
//    conflict-free whether the LDS serves 16 or 8 consecutive lanes per
//    cycle. Unswizzled the 16 rows are RB apart: one slot, a 16-way conflict.
//  - Copy store: 16 consecutive lanes hold chunks c0 .. c0 + 15 (c0 = 0 or
//    16) of one row r: slots (c ^ r) & 15 are a permutation of 0..15.
//
// Order of sums. Per (column tile, M tile) one accumulator takes the MFMAs of
// steps ascending and s = 0..FRAGS-1 within a step: the skinny kernel's
// order, so a WK = 1 point has the bits of the skinny kernel at WPB = 1. The
// A fragment is shared by the wave's NT column tiles, which does not change
// any accumulator's order. WK > 1: waves wk > 0 park their accumulators in
// LDS (the x stages, free by then) and wave wk = 0 adds them in wave order.
// No atomics: row m of y does not depend on M or BM and runs are
// bit-reproducible.
#include "skinny_gemm_impl.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace qtile {

using skinny::int4v;

// Built without the packed fp32 VALU forms, as moe_decode.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

template <class F, int BM, int WK>
constexpr int kLdsBytes = 2 * WK * BM * F::KSTEP * 2;   // two x stages

// Requires K % (WK * F::KSTEP * U) == 0, M >= 1, N % 16 == 0 (N % 32 if
// GLU), gridDim.x = column blocks * mtiles, kLdsBytes of dynamic LDS. Tile
// columns >= N read column N - 1 and are not stored.
template <class F, int BM, int WN, int WK, int NT, int U, int NTL, int GLU>
__global__ __launch_bounds__(WN * WK * 64) void quant_tile_gemm_kernel(
    const short* __restrict__ x,               // [M, K] bf16 row-major
    const typename F::welem* __restrict__ w,   // [N, K / WPACK] row-major
    const typename F::scale_t* __restrict__ scale,
    short* __restrict__ y,                     // [M, N] ([M, N / 2] if GLU)
    int M, int N, int K, int mtiles) {
  static_assert(!GLU || NT % 2 == 0, "GLU pairs gate and up tiles");
  static_assert(BM % 16 == 0 && WN * WK <= 8, "at most 512 threads");
  constexpr int MT = BM / 16;
  constexpr int T = WN * WK * 64;
  constexpr int RB = F::KSTEP * 2;          // bytes per slab row
  constexpr int SLAB = BM * RB;             // one k-slice of one stage
  constexpr int STAGE = WK * SLAB;
  constexpr int CPR = F::KSTEP / 8;         // 16 B chunks per slab row
  constexpr int RPP = T / CPR;              // rows per copy pass
  constexpr int CP = WK * BM / RPP;         // copy passes per step
  static_assert(T % CPR == 0 && BM % RPP == 0, "a pass stays in one slice");
  static_assert(kLdsBytes<F, BM, WK> <= 160 * 1024, "gfx950 LDS");
  static_assert((WK - 1) * WN * NT * MT * 1024 <= kLdsBytes<F, BM, WK>,
                "the parked accumulators fit the x stages");
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wn = wid % WN;                // column group
  const int wk = wid / WN;                // k-slice
  const int lr = lane & 15;
  const int lg = lane >> 4;
  constexpr int NTO = GLU ? NT / 2 : NT;  // column tiles of y per wave
  const int NO = GLU ? N / 2 : N;         // columns of y
  const int m0 = (blockIdx.x % mtiles) * BM;
  // first column of this wave's tiles; a wave past N works on clamped
  // columns (it must keep the block's barriers) and stores nothing
  const int n0 = ((blockIdx.x / mtiles) * WN + wn) * NTO * 16;

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

  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int m = 0; m < MT; m++) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- the x copy: chunk cc of rows cr + RPP * pass ----
  const int cr = tid / CPR, cc = tid % CPR;
  // only dereferenced for rows < M
  const short* xc = x + (size_t)(m0 + cr) * K + cc * 8;
  auto fetch_x = [&](int4v (&v)[CP], int d) {
#pragma unroll
    for (int c = 0; c < CP; c++) {
      const int rr = (c * RPP) % BM, sl = (c * RPP) / BM;
      v[c] = int4v{0, 0, 0, 0};
      if (m0 + cr + rr < M)
        v[c] = *reinterpret_cast<const int4v*>(xc + (size_t)rr * K + sl * kw +
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
    if (wk > 0) return;
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

  // C layout: lane holds y[m0 + 16 m + lg*4 + i][tilecol + lr], i = 0..3.
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
          const int row = m0 + m * 16 + lg * 4 + i;
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
        const int row = m0 + m * 16 + lg * 4 + i;
        if (row < M) {
          float v = acc[t][m][i];
          if constexpr (F::SCALED) v *= sc;
          y[(size_t)row * N + col] = f32_to_bf16(v);
        }
      }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// The (BM, WN, WK, NT, U) points the bindings can launch; U counts steps of
// F::KSTEP k. The first of each accepts every K % KSTEP == 0. Every point has
// an even NT and so a GLU form. ops/__init__.py keeps a copy.
#define FP8_TILE_GEMM_CONFIGS(X)                                            \
  X(64, 4, 1, 2, 1) X(128, 4, 1, 2, 2) X(64, 4, 2, 2, 2)                    \
  X(128, 4, 2, 2, 1) X(128, 8, 1, 2, 2) X(64, 2, 2, 2, 2) X(64, 2, 4, 2, 1)
#define MXFP4_TILE_GEMM_CONFIGS(X)                                          \
  X(64, 4, 1, 2, 1) X(128, 4, 1, 2, 1) X(64, 4, 2, 2, 1)                    \
  X(128, 8, 1, 2, 1) X(64, 8, 1, 2, 2) X(64, 2, 2, 2, 1) X(64, 1, 2, 2, 1)

}  // namespace qtile

namespace {

struct TileArgs {
  const short* x;
  const void* w;
  const void* scale;
  short* y;
  int M, N, K;
  int64_t bm, wn, wk, nt, u;
  bool glu;
  int nontemporal;   // < 0: non-temporal W loads iff there is one M tile
};

TileArgs check_args(const char* name, int64_t k_per_step,
                    const torch::Tensor& y, const torch::Tensor& x,
                    const torch::Tensor& w, const torch::Tensor& scale,
                    int64_t bm, int64_t wn, int64_t wk, int64_t nt, int64_t u,
                    bool glu, int64_t nontemporal, int64_t w_pack,
                    bool block_scaled) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && y.is_cuda() && scale.is_cuda(),
              name, ": tensors must be on the GPU");
  TORCH_CHECK(x.dtype() == torch::kBFloat16 && y.dtype() == torch::kBFloat16,
              name, ": x and y must be bf16");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && y.dim() == 2 &&
                  scale.dim() == (block_scaled ? 2 : 1),
              name, ": x [M,K], w [N,K], scale [N] or [N,K/32], y [M,N]");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && y.is_contiguous() &&
                  scale.is_contiguous(),
              name, ": tensors must be contiguous");
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) * w_pack == K && y.size(0) == M &&
                  y.size(1) == (glu ? N / 2 : N) && scale.size(0) == N &&
                  (!block_scaled || scale.size(1) * 32 == K),
              name, ": shape mismatch");
  TORCH_CHECK(M >= 1 && M < (1 << 24), name, ": needs 1 <= M < 2^24, got ",
              M);
  TORCH_CHECK(N >= 16 && N % 16 == 0 && N < (1 << 27), name,
              ": needs N % 16 == 0, got ", N);
  TORCH_CHECK(!glu || (N % 32 == 0 && nt % 2 == 0), name,
              ": the fused SwiGLU form needs N % 32 == 0 and an even NT, got "
              "N = ", N, ", NT = ", nt);
  TORCH_CHECK(bm > 0 && wn > 0 && wk > 0 && nt > 0 && u > 0, name,
              ": bad configuration");
  const int64_t kstep = wk * k_per_step * u;
  TORCH_CHECK(K >= kstep && K < (1 << 30) && K % kstep == 0, name,
              ": needs K % ", kstep, " == 0, got ", K);
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
                  (uintptr_t)w.data_ptr() % 16 == 0,
              name, ": x and w must be 16 B aligned");
  TORCH_CHECK(!block_scaled || (uintptr_t)scale.data_ptr() % 8 == 0, name,
              ": scale must be 8 B aligned");
  return {(const short*)x.data_ptr(), w.data_ptr(), scale.data_ptr(),
          (short*)y.data_ptr(), (int)M, (int)N, (int)K, bm, wn, wk, nt, u,
          glu, (int)nontemporal};
}

template <class F, int BM, int WN, int WK, int NT, int U, int NTL, int GLU>
void launch(const TileArgs& a, int mtiles, int64_t blocks) {
  constexpr int lds = qtile::kLdsBytes<F, BM, WK>;
  auto* kern = qtile::quant_tile_gemm_kernel<F, BM, WN, WK, NT, U, NTL, GLU>;
  if constexpr (lds > 65536) {
    static const hipError_t once = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)once;
  }
  kern<<<(unsigned)blocks, WN * WK * 64, lds,
         at::cuda::getCurrentHIPStream()>>>(
      a.x, (const typename F::welem*)a.w, (const typename F::scale_t*)a.scale,
      a.y, a.M, a.N, a.K, mtiles);
}

template <class F, int BM, int WN, int WK, int NT, int U>
void launch_point(const char* name, const TileArgs& a) {
  const int mtiles = (a.M + BM - 1) / BM;
  const int64_t cols = WN * NT * 16;
  const int64_t blocks = (a.N + cols - 1) / cols * mtiles;
  TORCH_CHECK(blocks < (1ll << 31), name, ": problem too large");
  const bool nt = a.nontemporal < 0 ? mtiles == 1 : a.nontemporal != 0;
  if (a.glu) {
    if constexpr (NT % 2 == 0) {
      if (nt) launch<F, BM, WN, WK, NT, U, 1, 1>(a, mtiles, blocks);
      else launch<F, BM, WN, WK, NT, U, 0, 1>(a, mtiles, blocks);
    } else {
      TORCH_CHECK(false, name, ": no fused SwiGLU kernel at an odd NT");
    }
  } else if (nt) {
    launch<F, BM, WN, WK, NT, U, 1, 0>(a, mtiles, blocks);
  } else {
    launch<F, BM, WN, WK, NT, U, 0, 0>(a, mtiles, blocks);
  }
}

typedef std::vector<std::tuple<int, int, int, int, int>> PointList;

#define TILE_CASE(BM, WN, WK, NT, U)                                         \
  if (a.bm == BM && a.wn == WN && a.wk == WK && a.nt == NT && a.u == U)      \
    return launch_point<Format, BM, WN, WK, NT, U>(name, a);
#define TILE_ENTRY(BM, WN, WK, NT, U) {BM, WN, WK, NT, U},
#define TILE_DISPATCH(NAME, F, TABLE)                                        \
  void NAME(const char* name, const TileArgs& a) {                           \
    using Format = F;                                                        \
    TABLE(TILE_CASE)                                                         \
    TORCH_CHECK(false, name, ": no kernel for (BM, WN, WK, NT, U) = (",      \
                a.bm, ", ", a.wn, ", ", a.wk, ", ", a.nt, ", ", a.u, ")");   \
  }                                                                          \
  PointList NAME##_configs() { return {TABLE(TILE_ENTRY)}; }
TILE_DISPATCH(launch_fp8, skinny::Fp8Coal, FP8_TILE_GEMM_CONFIGS)
TILE_DISPATCH(launch_mxfp4, skinny::Mxfp4Coal, MXFP4_TILE_GEMM_CONFIGS)
#undef TILE_DISPATCH
#undef TILE_ENTRY
#undef TILE_CASE

}  // namespace

// The launchers use the current stream and neither allocate nor synchronise,
// so they can run inside a captured graph.
void fp8_tile_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor wq,
                   torch::Tensor scale, int64_t bm, int64_t wn, int64_t wk,
                   int64_t nt, int64_t u, bool glu, int64_t nontemporal) {
  const char* name = "fp8_tile_gemm";
  TORCH_CHECK(wq.dtype() == at::kFloat8_e4m3fn, name,
              ": wq must be float8_e4m3fn");
  TORCH_CHECK(scale.dtype() == torch::kFloat32, name, ": scale must be fp32");
  launch_fp8(name, check_args(name, skinny::Fp8Coal::KSTEP, y, x, wq, scale,
                              bm, wn, wk, nt, u, glu, nontemporal, 1, false));
  HIP_CHECK_KERNEL();
}

void mxfp4_tile_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor q,
                     torch::Tensor scale, int64_t bm, int64_t wn, int64_t wk,
                     int64_t nt, int64_t u, bool glu, int64_t nontemporal) {
  const char* name = "mxfp4_tile_gemm";
  TORCH_CHECK(q.dtype() == torch::kUInt8 && scale.dtype() == torch::kUInt8,
              name, ": q and scale must be uint8");
  launch_mxfp4(name, check_args(name, skinny::Mxfp4Coal::KSTEP, y, x, q,
                                scale, bm, wn, wk, nt, u, glu, nontemporal,
                                skinny::Mxfp4Coal::WPACK, true));
  HIP_CHECK_KERNEL();
}

std::map<std::string, PointList> tile_gemm_configs() {
  return {{"fp8", launch_fp8_configs()}, {"mxfp4", launch_mxfp4_configs()}};
}
