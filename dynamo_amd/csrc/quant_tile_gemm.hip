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
//
// The main loop lives in quant_tile_gemm_impl.h, with the source of the x
// rows as a policy; moe_tile_gemm.hip runs it over expert segments.
#include "quant_tile_gemm_impl.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace qtile {

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// The identity instantiation of quant_tile_gemm_impl.h's main loop: slab row
// r is row m0 + r of x. Requires K % (WK * F::KSTEP * U) == 0, M >= 1,
// N % 16 == 0 (N % 32 if GLU), gridDim.x = column blocks * mtiles, kLdsBytes
// of dynamic LDS. Tile columns >= N read column N - 1 and are not stored.
template <class F, int BM, int WN, int WK, int NT, int U, int NTL, int GLU>
__global__ __launch_bounds__(WN * WK * 64) void quant_tile_gemm_kernel(
    const short* __restrict__ x,               // [M, K] bf16 row-major
    const typename F::welem* __restrict__ w,   // [N, K / WPACK] row-major
    const typename F::scale_t* __restrict__ scale,
    short* __restrict__ y,                     // [M, N] ([M, N / 2] if GLU)
    int M, int N, int K, int mtiles) {
  constexpr int MT = BM / 16;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int lane = threadIdx.x & 63;
  const int wn = (threadIdx.x >> 6) % WN;  // column group
  const int lr = lane & 15;
  const int lg = lane >> 4;
  constexpr int NTO = GLU ? NT / 2 : NT;  // column tiles of y per wave
  const int NO = GLU ? N / 2 : N;         // columns of y
  const int m0 = (blockIdx.x % mtiles) * BM;
  // first column of this wave's tiles; a wave past N works on clamped
  // columns (it must keep the block's barriers) and stores nothing
  const int n0 = ((blockIdx.x / mtiles) * WN + wn) * NTO * 16;

  f32x4 acc[NT][MT];
  const DenseRows<F, BM, WN, WK> rows(x, m0, M, K);
  if (!tile_gemm_mainloop<F, BM, WN, WK, NT, U, NTL, GLU>(
          acc, rows, w, scale, NO, K, n0, lds))
    return;

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
