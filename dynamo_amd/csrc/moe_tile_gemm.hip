// Routed MoE above the decode kernels' 64 tokens, for MI355X/gfx950: fp8
// (W8A16) and mxfp4 (W4A16) expert weights, T <= 4096 tokens, top-K <= 8 of
// E <= 64 experts. The contract is moe_decode.hip's - a pair is p = t K + j,
// pair_of lists the pairs grouped by expert in ascending p, expert e owns
// sorted positions seg_start[e] .. seg_start[e + 1] - 1 - and moe_combine of
// that file ends the chain. Two things are new.
//
// Route for many pairs (moe_route_tiled). moe_route_kernel is one block with
// one thread per pair. Here blocks of 512 pairs:
//   moe_tile_hist_kernel   hist[b][e] = pairs of expert e in block b
//   moe_tile_place_kernel  every block sums hist over the blocks (total[e])
//                          and over the blocks before it (before[e]), scans
//                          total over the experts, and places pair p of
//                          expert e at seg_start[e] + before[e] + (pairs of e
//                          in earlier waves of the block) + (in earlier lanes
//                          of p's wave): the number of pairs q < p of e plus
//                          the pairs of experts below e. Counts only; no
//                          atomic's arrival order decides a position, so
//                          pair_of equals a stable argsort element for
//                          element. Block 0 also writes seg_start and, from
//                          the same scan, the tile map of the GEMM's BM:
//                          tile_expert[i], tile_row0[i] for the BM-row tiles
//                          of the non-empty segments in ascending expert and
//                          row order, and ntiles. At most P / BM + min(E, P)
//                          tiles exist, which is how the host sizes the map.
//
// Expert-grouped tiled GEMM (moe_tile_gemm_kernel). The main loop is the
// dense tiled kernel's (quant_tile_gemm_impl.h: W streamed by the formats'
// row-coalesced loads, x through two XOR-swizzled LDS stages, MT = BM / 16
// MFMAs per converted B fragment, fixed-order k-slice reduction). The work
// split: grid.x = column blocks x max_tiles, blockIdx.x = column block *
// max_tiles + tile, so the tiles of one expert's W slab are neighbours in
// launch order and the slab's re-reads hit L2. A block reads (e, row0) of its
// tile and returns before any barrier if tile >= ntiles (blockIdx and device
// data only: block-uniform); an idle expert has no tile, so its codes and
// scales are never read. W and the scales are offset by e. The x copy is the
// dense one with a row indirection that each thread resolves once, ahead of
// the k loop: slab row r is x row pair_of[row0 + r] / topk (gather) or sorted
// row row0 + r (direct); rows at or past the segment's end are zero-filled,
// never looked up in pair_of and never stored.
// Epilogues, as in moe_decode.hip:
//   PLAIN     y[row0 + r, col] = bf16(acc * scale)
//   GLU       silu_mul_bf16(bf16(gate), bf16(up)): the bits of silu_mul on PLAIN
//   WEIGHTED  part[pair_of[row0 + r], col] = acc * scale * topw[pair], fp32
// Order of sums: the dense kernel's, so a sorted row's bits depend on neither
// its segment's size nor its tile nor BM, and equal fp8_tile_gemm /
// mxfp4_tile_gemm of that row with w[e] at the same WK.
//
// Resource usage (-Rpass-analysis=kernel-resource-usage) is listed in
// profiles/README.md, "Routed MoE, tiled": no instantiation uses scratch.
#include "quant_tile_gemm_impl.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <map>
#include <string>

namespace moe_tile {

constexpr int MAX_T = 4096, MAX_TOPK = 8, MAX_E = 64;
constexpr int ROUTE_THREADS = 512, ROUTE_WAVES = ROUTE_THREADS / 64;
enum Epilogue { PLAIN = 0, GLU = 1, WEIGHTED = 2 };

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// The thread's expert (clamped into [0, E); -1 past P) and, in whist, the
// pairs of every expert per wave of this block. LDS integer atomics: a count
// does not depend on arrival order. Ends on a barrier.
DEVINL int block_hist(const int* __restrict__ topi, int P, int E,
                      int (&whist)[ROUTE_WAVES][MAX_E]) {
  const int tid = threadIdx.x;
  for (int i = tid; i < ROUTE_WAVES * MAX_E; i += ROUTE_THREADS)
    (&whist[0][0])[i] = 0;
  __syncthreads();
  const int p = blockIdx.x * ROUTE_THREADS + tid;
  int e = -1;
  if (p < P) {
    e = topi[p];
    e = e < 0 ? 0 : (e >= E ? E - 1 : e);
    atomicAdd(&whist[tid >> 6][e], 1);
  }
  __syncthreads();
  return e;
}

__global__ __launch_bounds__(ROUTE_THREADS) void moe_tile_hist_kernel(
    const int* __restrict__ topi, int* __restrict__ hist, int P, int E) {
  __shared__ int whist[ROUTE_WAVES][MAX_E];
  block_hist(topi, P, E, whist);
  if (threadIdx.x < E) {
    int c = 0;
    for (int v = 0; v < ROUTE_WAVES; v++) c += whist[v][threadIdx.x];
    hist[blockIdx.x * E + threadIdx.x] = c;
  }
}

// hist [gridDim.x, E] as moe_tile_hist_kernel wrote it. tile_expert and
// tile_row0 hold at least P / BM + min(E, P) entries; only the first ntiles
// are written.
__global__ __launch_bounds__(ROUTE_THREADS) void moe_tile_place_kernel(
    const int* __restrict__ topi, const int* __restrict__ hist,
    int* __restrict__ seg_start, int* __restrict__ pair_of,
    int* __restrict__ tile_expert, int* __restrict__ tile_row0,
    int* __restrict__ ntiles, int P, int E, int BM) {
  __shared__ int whist[ROUTE_WAVES][MAX_E];
  __shared__ int base[MAX_E];      // seg_start[e] + pairs of e in blocks before
  __shared__ int sstart[MAX_E];    // seg_start[e]
  __shared__ int tstart[MAX_E + 1];  // first tile of e; [E] = ntiles
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int e = block_hist(topi, P, E, whist);
  if (wid == 0) {
    int total = 0, before = 0;
    if (lane < E)
      for (int b = 0; b < (int)gridDim.x; b++) {
        const int h = hist[b * E + lane];
        total += h;
        before += b < (int)blockIdx.x ? h : 0;
      }
    const int nt = (total + BM - 1) / BM;
    int incl = total, tincl = nt;
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64), to = __shfl_up(tincl, off, 64);
      if (lane >= off) { incl += o; tincl += to; }
    }
    if (lane < E) {
      base[lane] = incl - total + before;
      sstart[lane] = incl - total;
      tstart[lane] = tincl - nt;
      if (blockIdx.x == 0) seg_start[lane] = incl - total;
    }
    if (lane == E - 1) {
      tstart[E] = tincl;
      if (blockIdx.x == 0) { seg_start[E] = incl; ntiles[0] = tincl; }
    }
  }
  __syncthreads();
  int rank = 0;
  for (int j = 0; j < 64; j++) {
    const int ej = __shfl(e, j, 64);
    rank += (j < lane && ej == e) ? 1 : 0;
  }
  if (e >= 0) {
    int pos = base[e] + rank;
    for (int v = 0; v < wid; v++) pos += whist[v][e];
    pair_of[pos] = blockIdx.x * ROUTE_THREADS + tid;
  }
  if (blockIdx.x == 0)
    for (int t = tid; t < tstart[E]; t += ROUTE_THREADS) {
      // the last expert whose first tile is <= t: the empty ones before it
      // share its tstart, the ones after it start past t
      int te = 0;
      while (te + 1 < E && tstart[te + 1] <= t) te++;
      tile_expert[t] = te;
      tile_row0[t] = sstart[te] + (t - tstart[te]) * BM;
    }
}

// Slab row r of tile (row0, cnt rows): x row pair_of[row0 + r] / topk
// (gather) or sorted row row0 + r; rows r >= cnt are invalid and their
// pair_of entry is not read.
template <class F, int BM, int WN, int WK>
struct SegmentRows {
  using G = qtile::CopyGeom<F, BM, WN, WK>;
  const short* p[G::RP];
  int left;          // cnt - (the thread's first slab row)
  DEVINL SegmentRows(const short* a, const int* pair_of, int row0, int cnt,
                     int K, int topk, int gather) {
    const int cr = threadIdx.x / G::CPR, cc = threadIdx.x % G::CPR;
    left = cnt - cr;
#pragma unroll
    for (int i = 0; i < G::RP; i++) {
      p[i] = a;
      if (i * G::RPP < left) {
        const int pos = row0 + cr + i * G::RPP;
        const int row = gather ? pair_of[pos] / topk : pos;
        p[i] = a + (size_t)row * K + cc * 8;
      }
    }
  }
  DEVINL bool valid(int i) const { return i * G::RPP < left; }
  DEVINL const short* ptr(int i) const { return p[i]; }
};

// Requires K % (WK * F::KSTEP * U) == 0, N % 16 == 0 (N % 32 for GLU),
// gridDim.x = column blocks * max_tiles, kLdsBytes of dynamic LDS, the route
// outputs of moe_tile_place_kernel at this BM. w is [E, N, K / WPACK], scale
// [E, N] (fp8) or [E, N, K / 32] (mxfp4). Tile columns >= N read column
// N - 1 and are not stored.
template <class F, int BM, int WN, int WK, int NT, int U, int EPI>
__global__ __launch_bounds__(WN * WK * 64) void moe_tile_gemm_kernel(
    const short* __restrict__ a,          // gather: x [T, K]; direct: [P, K]
    const typename F::welem* __restrict__ w,
    const typename F::scale_t* __restrict__ scale,
    const int* __restrict__ seg_start,    // [E + 1]
    const int* __restrict__ pair_of,      // [P]
    const float* __restrict__ topw,       // [P] fp32, WEIGHTED only
    const int* __restrict__ tile_expert, const int* __restrict__ tile_row0,
    const int* __restrict__ ntiles,
    void* __restrict__ out, int N, int K, int topk, int gather,
    int max_tiles) {
  constexpr bool kGlu = EPI == GLU;
  constexpr int MT = BM / 16;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tile = blockIdx.x % max_tiles;
  if (tile >= ntiles[0]) return;          // block-uniform, before any barrier
  const int e = tile_expert[tile];
  const int row0 = tile_row0[tile];
  const int left = seg_start[e + 1] - row0;
  const int cnt = left < BM ? left : BM;  // >= 1 by the tile map

  const int lane = threadIdx.x & 63;
  const int wn = (threadIdx.x >> 6) % WN;
  const int lr = lane & 15;
  const int lg = lane >> 4;
  constexpr int NTO = kGlu ? NT / 2 : NT;
  const int NO = kGlu ? N / 2 : N;
  const int n0 = ((blockIdx.x / max_tiles) * WN + wn) * NTO * 16;

  const size_t erow = (size_t)e * N;      // the expert's first weight row
  const typename F::scale_t* escale =
      scale + (F::BLOCK_SCALED ? erow * (K / 32) : erow);
  f32x4 acc[NT][MT];
  const SegmentRows<F, BM, WN, WK> rows(a, pair_of, row0, cnt, K, topk,
                                        gather);
  if (!qtile::tile_gemm_mainloop<F, BM, WN, WK, NT, U, 0, kGlu>(
          acc, rows, w + erow * (K / F::WPACK), escale, NO, K, n0, lds))
    return;

  // The row scales of this lane's columns (fp8), gate tiles then up tiles.
  float sc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    sc[t] = 1.f;
    if constexpr (F::SCALED) {
      int col = n0 + (t % NTO) * 16 + lr;
      col = col < NO ? col : NO - 1;
      if (kGlu && t >= NTO) col += NO;
      sc[t] = escale[col];
    }
  }
  // C layout: lane holds slab row 16 m + lg*4 + i, column tilecol + lr.
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = m * 16 + lg * 4 + i;
      if (r >= cnt) continue;
      if constexpr (EPI == WEIGHTED) {
        const int p = pair_of[row0 + r];
        const float wt = topw[p];
        float* part = reinterpret_cast<float*>(out) + (size_t)p * N;
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const int col = n0 + t * 16 + lr;
          if (col < N) part[col] = acc[t][m][i] * sc[t] * wt;
        }
      } else {
        short* y = reinterpret_cast<short*>(out) + (size_t)(row0 + r) * NO;
#pragma unroll
        for (int t = 0; t < NTO; t++) {
          const int col = n0 + t * 16 + lr;
          if (col >= NO) continue;
          if constexpr (kGlu)
            y[col] = silu_mul_bf16(
                f32_to_bf16(acc[t][m][i] * sc[t]),
                f32_to_bf16(acc[t + NTO][m][i] * sc[t + NTO]));
          else
            y[col] = f32_to_bf16(acc[t][m][i] * sc[t]);
        }
      }
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// The (BM, WN, WK, NT, U) points the bindings can launch, each with the three
// epilogues: BM in {32, 64, 128} times the dense kernel's (WN, WK, NT, U)
// points that fit (mxfp4 (4, 2, 2, 1) at BM = 128 would need 256 KB of LDS).
// U counts steps of F::KSTEP k; the first point of every BM accepts every
// K % F::KSTEP == 0. ops/__init__.py keeps a copy.
#define MOE_TILE_FP8_CONFIGS(X)                                             \
  X(32, 4, 1, 2, 1) X(64, 4, 1, 2, 1) X(128, 4, 1, 2, 1)                     \
  X(32, 4, 2, 2, 2) X(64, 4, 2, 2, 2) X(128, 4, 2, 2, 2)                     \
  X(32, 8, 1, 2, 2) X(64, 8, 1, 2, 2) X(128, 8, 1, 2, 2)
#define MOE_TILE_MXFP4_CONFIGS(X)                                           \
  X(32, 4, 1, 2, 1) X(64, 4, 1, 2, 1) X(128, 4, 1, 2, 1)                     \
  X(32, 4, 2, 2, 1) X(64, 4, 2, 2, 1)                                        \
  X(32, 8, 1, 2, 1) X(64, 8, 1, 2, 1) X(128, 8, 1, 2, 1)

}  // namespace moe_tile

namespace {

bool i32_vec(const torch::Tensor& t) {
  return t.is_cuda() && t.dtype() == torch::kInt32 && t.is_contiguous() &&
         t.dim() == 1;
}

struct TiledArgs {
  const short* a;
  const void* wq;
  const void* scale;
  const int* seg_start;
  const int* pair_of;
  const float* topw;
  const int* tile_expert;
  const int* tile_row0;
  const int* ntiles;
  void* out;
  int N, K, topk, gather, max_tiles;
};

template <class F, int BM, int WN, int WK, int NT, int U, int EPI>
void launch(const char* name, const TiledArgs& r) {
  constexpr int lds = qtile::kLdsBytes<F, BM, WK>;
  auto* kern = moe_tile::moe_tile_gemm_kernel<F, BM, WN, WK, NT, U, EPI>;
  if constexpr (lds > 65536) {
    static const hipError_t once = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)once;
  }
  const int NO = EPI == moe_tile::GLU ? r.N / 2 : r.N;
  constexpr int cols = WN * (EPI == moe_tile::GLU ? NT / 2 : NT) * 16;
  const int64_t blocks = (int64_t)((NO + cols - 1) / cols) * r.max_tiles;
  TORCH_CHECK(blocks < (1ll << 31), name, ": problem too large");
  kern<<<(unsigned)blocks, WN * WK * 64, lds,
         at::cuda::getCurrentHIPStream()>>>(
      r.a, (const typename F::welem*)r.wq, (const typename F::scale_t*)r.scale,
      r.seg_start, r.pair_of, r.topw, r.tile_expert, r.tile_row0, r.ntiles,
      r.out, r.N, r.K, r.topk, r.gather, r.max_tiles);
}

template <class F>
void dispatch(const char* name, const TiledArgs& r, int64_t epilogue,
              int64_t bm, int64_t wn, int64_t wk, int64_t nt, int64_t u) {
#define MOE_TILE_CASE(BM, WN, WK, NT, U)                                     \
  if (bm == BM && wn == WN && wk == WK && nt == NT && u == U) {              \
    if (epilogue == moe_tile::GLU)                                           \
      return launch<F, BM, WN, WK, NT, U, moe_tile::GLU>(name, r);           \
    if (epilogue == moe_tile::WEIGHTED)                                      \
      return launch<F, BM, WN, WK, NT, U, moe_tile::WEIGHTED>(name, r);      \
    return launch<F, BM, WN, WK, NT, U, moe_tile::PLAIN>(name, r);           \
  }
  if constexpr (std::is_same<F, skinny::Fp8Coal>::value) {
    MOE_TILE_FP8_CONFIGS(MOE_TILE_CASE)
  } else {
    MOE_TILE_MXFP4_CONFIGS(MOE_TILE_CASE)
  }
#undef MOE_TILE_CASE
  TORCH_CHECK(false, name, ": no kernel for (BM, WN, WK, NT, U) = (", bm,
              ", ", wn, ", ", wk, ", ", nt, ", ", u, ")");
}

// The checks and the launch of moe_tiled_gemm_fp8 / _mxfp4; the callers have
// checked the dtypes of wq and scale.
template <class F>
void tiled_quant(const char* name, torch::Tensor out, torch::Tensor a,
                 torch::Tensor wq, torch::Tensor scale,
                 torch::Tensor seg_start, torch::Tensor pair_of,
                 torch::Tensor tile_expert, torch::Tensor tile_row0,
                 torch::Tensor ntiles, c10::optional<torch::Tensor> topw,
                 int64_t topk, bool gather, int64_t epilogue, int64_t bm,
                 int64_t wn, int64_t wk, int64_t nt, int64_t u) {
  TORCH_CHECK(epilogue >= 0 && epilogue <= 2, name, ": bad epilogue");
  const bool glu = epilogue == moe_tile::GLU;
  const bool weighted = epilogue == moe_tile::WEIGHTED;
  TORCH_CHECK(a.is_cuda() && wq.is_cuda() && scale.is_cuda() && out.is_cuda() &&
                  i32_vec(seg_start) && i32_vec(pair_of) &&
                  i32_vec(tile_expert) && i32_vec(tile_row0) &&
                  i32_vec(ntiles),
              name, ": tensors must be on the GPU, the route's outputs "
              "contiguous int32 vectors");
  TORCH_CHECK(a.dtype() == torch::kBFloat16 &&
                  out.dtype() == (weighted ? torch::kFloat32
                                           : torch::kBFloat16),
              name, ": a bf16, out bf16 (fp32 if weighted)");
  TORCH_CHECK(a.dim() == 2 && wq.dim() == 3 && out.dim() == 2 &&
                  scale.dim() == (F::BLOCK_SCALED ? 3 : 2),
              name, ": a [rows, K], codes [E, N, K / ", F::WPACK,
              "], scale [E, N", F::BLOCK_SCALED ? ", K / 32]" : "]",
              ", out [P, cols]");
  TORCH_CHECK(a.is_contiguous() && wq.is_contiguous() &&
                  scale.is_contiguous() && out.is_contiguous(),
              name, ": tensors must be contiguous");
  const int64_t P = pair_of.size(0), E = wq.size(0), N = wq.size(1),
                K = wq.size(2) * F::WPACK;
  TORCH_CHECK(topk >= 1 && topk <= moe_tile::MAX_TOPK && P >= 1 &&
                  P % topk == 0 && P / topk <= moe_tile::MAX_T && E >= 1 &&
                  E <= moe_tile::MAX_E && seg_start.size(0) == E + 1,
              name, ": needs T <= ", moe_tile::MAX_T, ", topk <= 8, E <= 64 "
              "and seg_start [E + 1]");
  const int64_t T = P / topk;
  TORCH_CHECK((bm == 32 || bm == 64 || bm == 128) && wn > 0 && wk > 0 &&
                  nt > 0 && u > 0, name, ": bad configuration");
  const int64_t max_tiles = P / bm + std::min(E, P);
  TORCH_CHECK(tile_expert.size(0) >= max_tiles &&
                  tile_row0.size(0) >= max_tiles && ntiles.size(0) == 1,
              name, ": the tile map needs P / BM + min(E, P) = ", max_tiles,
              " entries and ntiles [1]");
  TORCH_CHECK(a.size(1) == K && a.size(0) == (gather ? T : P) &&
                  out.size(0) == P && out.size(1) == (glu ? N / 2 : N) &&
                  scale.size(0) == E && scale.size(1) == N &&
                  (!F::BLOCK_SCALED || scale.size(2) * 32 == K),
              name, ": shape mismatch");
  TORCH_CHECK(N >= 16 && N % 16 == 0 && N < (1 << 27) && (!glu || N % 32 == 0),
              name, ": needs N % 16 == 0 (N % 32 for the SwiGLU form), got ",
              N);
  const int64_t kstep = wk * F::KSTEP * u;
  TORCH_CHECK(K >= kstep && K < (1 << 30) && K % kstep == 0, name,
              ": needs K % ", kstep, " == 0, got ", K);
  TORCH_CHECK((uintptr_t)a.data_ptr() % 16 == 0 &&
                  (uintptr_t)wq.data_ptr() % 16 == 0 &&
                  (!F::BLOCK_SCALED || (uintptr_t)scale.data_ptr() % 8 == 0),
              name, ": a and the codes must be 16 B aligned, block scales "
              "8 B");
  const float* tw = nullptr;
  if (weighted) {
    TORCH_CHECK(topw.has_value() && topw->is_cuda() &&
                    topw->dtype() == torch::kFloat32 &&
                    topw->is_contiguous() && topw->numel() == P,
                name, ": the weighted form needs topw fp32 with T topk "
                "elements");
    tw = (const float*)topw->data_ptr();
  }
  const TiledArgs r{(const short*)a.data_ptr(), wq.data_ptr(),
                    scale.data_ptr(), (const int*)seg_start.data_ptr(),
                    (const int*)pair_of.data_ptr(), tw,
                    (const int*)tile_expert.data_ptr(),
                    (const int*)tile_row0.data_ptr(),
                    (const int*)ntiles.data_ptr(), out.data_ptr(), (int)N,
                    (int)K, (int)topk, gather ? 1 : 0, (int)max_tiles};
  dispatch<F>(name, r, epilogue, bm, wn, wk, nt, u);
  HIP_CHECK_KERNEL();
}

}  // namespace

// topi [T, K] int32 -> seg_start [E + 1], pair_of [T K], and the tile map of
// `bm`-row tiles: tile_expert / tile_row0 with at least T K / bm + min(E, T K)
// entries, ntiles [1]. hist is scratch, ceil(T K / 512) * E int32. All on the
// current stream, no allocation and no host read.
void moe_route_tiled(torch::Tensor topi, torch::Tensor seg_start,
                     torch::Tensor pair_of, torch::Tensor tile_expert,
                     torch::Tensor tile_row0, torch::Tensor ntiles,
                     torch::Tensor hist, int64_t bm) {
  const char* name = "moe_route_tiled";
  TORCH_CHECK(topi.is_cuda() && topi.dtype() == torch::kInt32 &&
                  topi.is_contiguous() && topi.dim() == 2 &&
                  i32_vec(seg_start) && i32_vec(pair_of) &&
                  i32_vec(tile_expert) && i32_vec(tile_row0) &&
                  i32_vec(ntiles) && i32_vec(hist),
              name, ": topi [T, K] and the outputs must be contiguous int32 "
              "on the GPU");
  const int64_t T = topi.size(0), K = topi.size(1), E = seg_start.size(0) - 1;
  TORCH_CHECK(T >= 1 && T <= moe_tile::MAX_T && K >= 1 &&
                  K <= moe_tile::MAX_TOPK && E >= 1 && E <= moe_tile::MAX_E,
              name, ": needs 1 <= T <= ", moe_tile::MAX_T, ", 1 <= K <= 8, "
              "1 <= E <= 64, got T = ", T, ", K = ", K, ", E = ", E);
  TORCH_CHECK(bm == 32 || bm == 64 || bm == 128, name,
              ": BM must be 32, 64 or 128");
  const int64_t P = T * K;
  const int64_t blocks = (P + moe_tile::ROUTE_THREADS - 1) /
                         moe_tile::ROUTE_THREADS;
  const int64_t max_tiles = P / bm + std::min(E, P);
  TORCH_CHECK(pair_of.size(0) == P && tile_expert.size(0) >= max_tiles &&
                  tile_row0.size(0) >= max_tiles && ntiles.size(0) == 1 &&
                  hist.size(0) >= blocks * E,
              name, ": needs pair_of [T K], a tile map of ", max_tiles,
              " entries, ntiles [1] and hist [", blocks * E, "]");
  auto stream = at::cuda::getCurrentHIPStream();
  moe_tile::moe_tile_hist_kernel<<<(unsigned)blocks, moe_tile::ROUTE_THREADS,
                                   0, stream>>>(
      (const int*)topi.data_ptr(), (int*)hist.data_ptr(), (int)P, (int)E);
  moe_tile::moe_tile_place_kernel<<<(unsigned)blocks, moe_tile::ROUTE_THREADS,
                                    0, stream>>>(
      (const int*)topi.data_ptr(), (const int*)hist.data_ptr(),
      (int*)seg_start.data_ptr(), (int*)pair_of.data_ptr(),
      (int*)tile_expert.data_ptr(), (int*)tile_row0.data_ptr(),
      (int*)ntiles.data_ptr(), (int)P, (int)E, (int)bm);
  HIP_CHECK_KERNEL();
}

// The expert-grouped tiled GEMM for W8A16 experts: wq float8_e4m3fn
// [E, N, K], scale fp32 [E, N]; the route's outputs at the same bm; epilogue
// and the shapes of a / out as moe_routed_gemm_fp8; (bm, wn, wk, nt, u) a
// point of MOE_TILE_FP8_CONFIGS, K % (wk 128 u) == 0.
void moe_tiled_gemm_fp8(torch::Tensor out, torch::Tensor a, torch::Tensor wq,
                        torch::Tensor scale, torch::Tensor seg_start,
                        torch::Tensor pair_of, torch::Tensor tile_expert,
                        torch::Tensor tile_row0, torch::Tensor ntiles,
                        c10::optional<torch::Tensor> topw, int64_t topk,
                        bool gather, int64_t epilogue, int64_t bm, int64_t wn,
                        int64_t wk, int64_t nt, int64_t u) {
  const char* name = "moe_tiled_gemm_fp8";
  TORCH_CHECK(wq.dtype() == at::kFloat8_e4m3fn &&
                  scale.dtype() == torch::kFloat32,
              name, ": wq must be float8_e4m3fn, scale fp32");
  tiled_quant<skinny::Fp8Coal>(name, out, a, wq, scale, seg_start, pair_of,
                               tile_expert, tile_row0, ntiles, topw, topk,
                               gather, epilogue, bm, wn, wk, nt, u);
}

// The same for W4A16 experts: q uint8 [E, N, K / 2], scale uint8 (e8m0)
// [E, N, K / 32]; a point of MOE_TILE_MXFP4_CONFIGS, K % (wk 256 u) == 0.
void moe_tiled_gemm_mxfp4(torch::Tensor out, torch::Tensor a, torch::Tensor q,
                          torch::Tensor scale, torch::Tensor seg_start,
                          torch::Tensor pair_of, torch::Tensor tile_expert,
                          torch::Tensor tile_row0, torch::Tensor ntiles,
                          c10::optional<torch::Tensor> topw, int64_t topk,
                          bool gather, int64_t epilogue, int64_t bm,
                          int64_t wn, int64_t wk, int64_t nt, int64_t u) {
  const char* name = "moe_tiled_gemm_mxfp4";
  TORCH_CHECK(q.dtype() == torch::kUInt8 && scale.dtype() == torch::kUInt8,
              name, ": q and scale must be uint8");
  tiled_quant<skinny::Mxfp4Coal>(name, out, a, q, scale, seg_start, pair_of,
                                 tile_expert, tile_row0, ntiles, topw, topk,
                                 gather, epilogue, bm, wn, wk, nt, u);
}

// {"fp8" | "mxfp4": [(BM, WN, WK, NT, U), ...]}, for the Python side to
// check its copy against.
std::map<std::string, std::vector<std::tuple<int, int, int, int, int>>>
moe_tile_configs() {
#define MOE_TILE_ENTRY(BM, WN, WK, NT, U) {BM, WN, WK, NT, U},
  return {{"fp8", {MOE_TILE_FP8_CONFIGS(MOE_TILE_ENTRY)}},
          {"mxfp4", {MOE_TILE_MXFP4_CONFIGS(MOE_TILE_ENTRY)}}};
#undef MOE_TILE_ENTRY
}
