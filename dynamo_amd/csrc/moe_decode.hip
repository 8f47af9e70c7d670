// Routed MoE decode for MI355X/gfx950: T <= 64 tokens, top-K of E experts,
// bf16, fp8 (W8A16) or mxfp4 (W4A16) expert weights. Three kernels replace
// the sort / pad / bmm / gather / index_add chain of MoEMLP.forward's decode
// branch:
//
//   moe_route_kernel        topi [T, K] -> seg_start [E + 1], pair_of [T K]
//   moe_skinny_gemm_kernel  one expert-grouped skinny GEMM per projection
//   moe_combine_kernel      out[t] = bf16(sum_j part[t K + j]), fp32, j ascending
//
// A pair is p = t K + j, token t's j-th pick. pair_of lists the pairs grouped
// by expert, ascending p within an expert (a stable counting sort, equal to
// argsort(topi.flatten(), stable)); expert e owns sorted positions
// seg_start[e] .. seg_start[e + 1] - 1, its segment.
//
// The GEMM is the W-streaming design of skinny_gemm_impl.h, whose Bf16Coal
// format (8 rows x 128 B per load, ds_bpermute to the MFMA B fragment,
// non-temporal W loads, U steps in flight, fixed-order cross-wave K reduction)
// it takes by inclusion. What is new is the work split and both ends of the
// data path. The grid is (column-tile groups, E): block (., e) reads its
// expert's segment length cnt and returns at once if it is 0, so an idle
// expert's weights are never read; otherwise it streams w[e]'s rows of its
// NT column tiles exactly once against all cnt <= 16 MT rows of the segment.
// m-tiles with 16 m >= cnt (wave-uniform) skip their A loads and MFMAs.
// A goes from global memory straight to VGPRs. Lane lr of m-tile m owns
// segment row r = 16 m + lr:
//   gather: row x[pair_of[s + r] / K], so the per-expert copy of x is never
//           materialised;
//   direct: row a[s + r], the sorted order a previous pass wrote.
// Rows r >= cnt read the segment's first row (their pair_of lookup too), so
// nothing is read past pair_of or a; they are never stored.
// Epilogues:
//   PLAIN     y[s + r, col] = bf16(acc)
//   GLU       w[e] is [2I, D], gate rows first; a block pairs gate tiles with
//             their up tiles at + I as the dense GLU = 1 does and stores
//             silu_mul_bf16(bf16(g), bf16(u)): the bits of silu_mul on PLAIN
//   WEIGHTED  part[pair_of[s + r], col] = acc * topw[pair], fp32. Every pair
//             is in exactly one segment, so part is fully written.
// Static grids on the current stream, no host sync and no allocation: the
// route captures into the decode hipGraph.
//
// Quantised experts (ops.Fp8ExpertWeight, ops.Mxfp4ExpertWeight) run
// moe_skinny_gemm_q_kernel in the GEMM's place: the Fp8Coal / Mxfp4Coal W
// streams of the same header, per-expert scales, and the segment's rows split
// into chunks of at most 32 on grid.z (described at the kernel). moe_route
// and moe_combine serve every format.
#include "skinny_gemm_impl.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <map>
#include <string>

namespace moe_decode {

constexpr int MAX_T = 64, MAX_TOPK = 8, MAX_E = 64;
constexpr int ROUTE_THREADS = MAX_T * MAX_TOPK;   // one thread per pair
constexpr int ROUTE_WAVES = ROUTE_THREADS / 64;
enum Epilogue { PLAIN = 0, GLU = 1, WEIGHTED = 2 };

// The device code of this namespace is built without the packed fp32 VALU
// forms (v_pk_add/mul/fma_f32): the attribute does per function, the kernels'
// lambdas included, what -target-feature -packed-fp32-ops does per file.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// One block. Counts per (wave, expert) with LDS integer atomics (a count does
// not depend on arrival order), an exclusive scan over the experts in wave 0,
// and a placement that uses no atomics: pair p of expert e goes to
//   seg_start[e] + (pairs of e in earlier waves) + (pairs of e in earlier
//   lanes of p's wave),
// which is the number of pairs q < p of e. An index outside [0, E) is clamped
// into it, so every pair is placed and pair_of is a permutation whatever the
// gating wrote.
__global__ __launch_bounds__(ROUTE_THREADS) void moe_route_kernel(
    const int* __restrict__ topi, int* __restrict__ seg_start,
    int* __restrict__ pair_of, int P, int E) {
  __shared__ int whist[ROUTE_WAVES][MAX_E];
  __shared__ int base[MAX_E];
  const int p = threadIdx.x;
  const int lane = p & 63, wid = p >> 6;
  for (int i = p; i < ROUTE_WAVES * MAX_E; i += ROUTE_THREADS)
    (&whist[0][0])[i] = 0;
  __syncthreads();
  int e = -1;
  if (p < P) {
    e = topi[p];
    e = e < 0 ? 0 : (e >= E ? E - 1 : e);
    atomicAdd(&whist[wid][e], 1);
  }
  __syncthreads();
  if (wid == 0) {
    int c = 0;
    if (lane < E)
      for (int v = 0; v < ROUTE_WAVES; v++) c += whist[v][lane];
    int incl = c;
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane < E) {
      base[lane] = incl - c;
      seg_start[lane] = incl - c;
    }
    if (lane == E - 1) seg_start[E] = incl;
  }
  __syncthreads();
  int rank = 0;
  for (int j = 0; j < 64; j++) {
    const int ej = __shfl(e, j, 64);
    rank += (j < lane && ej == e) ? 1 : 0;
  }
  if (p < P) {
    int pos = base[e] + rank;
    for (int v = 0; v < wid; v++) pos += whist[v][e];
    pair_of[pos] = p;
  }
}

// Requires K % (WPB * 64 * U) == 0, N % 16 == 0 (N % 32 for GLU, NT even),
// 1 <= topk, seg_start / pair_of as moe_route_kernel writes them with every
// segment at most 16 MT rows. w is [E, N, K]. Tile columns past N read column
// N - 1 (clamped addresses) and are not stored.
template <int WPB, int U, int NT, int MT, int EPI>
__global__ __launch_bounds__(WPB * 64) void moe_skinny_gemm_kernel(
    const short* __restrict__ a,          // gather: x [T, K]; direct: [P, K]
    const short* __restrict__ w,          // [E, N, K] bf16
    const int* __restrict__ seg_start,    // [E + 1]
    const int* __restrict__ pair_of,      // [P]
    const float* __restrict__ topw,       // [P] fp32, WEIGHTED only
    void* __restrict__ out,               // see the epilogues above
    int N, int K, int topk, int gather) {
  using F = skinny::Bf16Coal;
  using skinny::int4v;
  constexpr bool kGlu = EPI == GLU;
  static_assert(!kGlu || NT % 2 == 0, "GLU pairs gate and up tiles");
  const int e = blockIdx.y;
  const int s = seg_start[e];
  const int cnt = seg_start[e + 1] - s;   // block-uniform
  if (cnt <= 0) return;                   // idle expert: no W byte is read

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;       // 0..WPB-1 = k-slice
  const int lr = lane & 15;
  const int lg = lane >> 4;
  constexpr int NTO = kGlu ? NT / 2 : NT; // column tiles of the output
  const int NO = kGlu ? N / 2 : N;        // columns of the output
  const int n0 = (blockIdx.x * NTO) * 16;
  if (n0 >= NO) return;
  // m-tile m holds rows of the segment; tile 0 always does
  auto live = [&](int m) { return m == 0 || 16 * m < cnt; };

  const int kw = K / WPB;
  const int k0 = wid * kw;
  const int steps = kw / F::KSTEP;

  const short* xp[MT];
#pragma unroll
  for (int m = 0; m < MT; m++) {
    const int r = m * 16 + lr;
    const int pos = s + (r < cnt ? r : 0);
    const int row = gather ? pair_of[pos] / topk : pos;
    xp[m] = a + (size_t)row * K + k0 + F::x_k(lane);
  }
  const short* we = w + (size_t)e * N * K;
  const short* wp[NT][F::LOADS];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int h = 0; h < F::LOADS; h++) {
      int col = n0 + (t % NTO) * 16 + F::w_row(lane, h);
      col = col < NO ? col : NO - 1;
      if (kGlu && t >= NTO) col += NO;    // the up row of that column
      wp[t][h] = we + (size_t)col * K + k0 + F::w_k(lane);
    }
  const F::Sel sel = F::sel(lane);

  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int m = 0; m < MT; m++) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16x8 abuf[U][MT][F::FRAGS];
  int4v rbuf[NT][U][F::LOADS];
  auto load_x = [&](bf16x8 (&x)[MT][F::FRAGS], int d) {
#pragma unroll
    for (int m = 0; m < MT; m++)
      if (live(m)) {
#pragma unroll
        for (int f = 0; f < F::FRAGS; f++)
          x[m][f] = *reinterpret_cast<const bf16x8*>(xp[m] + d * F::KSTEP +
                                                     F::x_step(f));
      }
  };
  auto load_w = [&](int4v (&r)[F::LOADS], int t, int d) {
#pragma unroll
    for (int h = 0; h < F::LOADS; h++)
      r[h] = skinny::ldw<1>(wp[t][h] + d * F::KSTEP);
  };
  auto consume = [&](const bf16x8 (&x)[MT][F::FRAGS],
                     const int4v (&r)[F::LOADS], f32x4 (&c)[MT]) {
#pragma unroll
    for (int f = 0; f < F::FRAGS; f++) {
      const bf16x8 b = F::b_frag(f, r, sel, skinny::NoAux{});
#pragma unroll
      for (int m = 0; m < MT; m++)
        if (live(m))
          c[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[m][f], b, c[m],
                                                         0, 0, 0);
    }
  };

  // U steps in flight, as in skinny_gemm_kernel: each main-loop step takes
  // its registers, issues the loads of step d + u into them and then runs
  // the MFMAs of the taken ones.
#pragma unroll
  for (int u = 0; u < U; u++) {
    load_x(abuf[u], u);
#pragma unroll
    for (int t = 0; t < NT; t++) load_w(rbuf[t][u], t, u);
  }
  for (int d = U; d < steps; d += U) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      bf16x8 x[MT][F::FRAGS];
#pragma unroll
      for (int m = 0; m < MT; m++)
        if (live(m)) {
#pragma unroll
          for (int f = 0; f < F::FRAGS; f++) x[m][f] = abuf[u][m][f];
        }
      load_x(abuf[u], d + u);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        int4v r[F::LOADS];
#pragma unroll
        for (int h = 0; h < F::LOADS; h++) r[h] = rbuf[t][u][h];
        load_w(rbuf[t][u], t, d + u);
        consume(x, r, acc[t]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int t = 0; t < NT; t++) consume(abuf[u], rbuf[t][u], acc[t]);

  // Cross-wave reduction in wave order, one live m-tile at a time (cnt is
  // block-uniform, so every wave takes the same barriers).
  __shared__ f32x4 red[WPB > 1 ? (WPB - 1) * NT * 64 : 1];
  if (WPB > 1) {
#pragma unroll
    for (int m = 0; m < MT; m++) {
      if (!live(m)) break;
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

  // C layout: lane holds segment row 16 m + lg*4 + i, column tilecol + lr.
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = m * 16 + lg * 4 + i;
      if (r >= cnt) continue;
      if constexpr (EPI == WEIGHTED) {
        const int p = pair_of[s + r];
        const float wt = topw[p];
        float* part = reinterpret_cast<float*>(out) + (size_t)p * N;
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const int col = n0 + t * 16 + lr;
          if (col < N) part[col] = acc[t][m][i] * wt;
        }
      } else {
        short* y = reinterpret_cast<short*>(out) + (size_t)(s + r) * NO;
#pragma unroll
        for (int t = 0; t < NTO; t++) {
          const int col = n0 + t * 16 + lr;
          if (col >= NO) continue;
          if constexpr (kGlu)
            y[col] = silu_mul_bf16(f32_to_bf16(acc[t][m][i]),
                                   f32_to_bf16(acc[t + NTO][m][i]));
          else
            y[col] = f32_to_bf16(acc[t][m][i]);
        }
      }
    }
}

// out[t, c .. c + 8) = bf16(sum_j part[t K + j, c .. c + 8)), fp32, ascending
// j; one thread per 8 columns (two 16 B loads per j, one 16 B store). No
// atomics: the bits do not depend on how the tokens were grouped.
__global__ __launch_bounds__(256) void moe_combine_kernel(
    short* __restrict__ out, const float* __restrict__ part, int T, int D,
    int topk) {
  const int chunks = D / 8;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * chunks) return;
  const int t = i / chunks, c = (i % chunks) * 8;
  float4v lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < topk; j++) {
    const float4v* src = reinterpret_cast<const float4v*>(
        part + (size_t)(t * topk + j) * D + c);
    lo += src[0];
    hi += src[1];
  }
  short8 o;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    o[k] = f32_to_bf16(lo[k]);
    o[4 + k] = f32_to_bf16(hi[k]);
  }
  *reinterpret_cast<short8*>(out + (size_t)t * D + c) = o;
}

// The routed GEMM for quantised expert weights: F is Fp8Coal (W8A16, codes
// [E, N, K] e4m3, scale fp32 [E, N]) or Mxfp4Coal (W4A16, codes [E, N, K / 2]
// bytes, scale e8m0 [E, N, K / 32]). Same contract as moe_skinny_gemm_kernel;
// what differs:
//   rows    the accumulator tiles are bounded by registers (FRAGS = 4 / 8 A
//           fragments per m-tile and step), so MT <= 2 and grid.z carries the
//           row chunk: block (x, e, z) owns rows [CH z, CH z + CH) of expert
//           e's segment, CH = 16 MT, and returns before any load of codes or
//           scales if CH z >= the segment's length, which an idle expert's 0
//           always is. The launcher runs MT = 1, grid.z = 1 for T <= 16 and
//           MT = 2, grid.z = ceil(T / 32) above, so an expert with at most
//           32 rows streams its weights once and only a longer segment reads
//           them again, once per further chunk. s and cnt below are the
//           chunk's first sorted position and length; both depend on
//           blockIdx and seg_start only, so they are block-uniform and every
//           wave takes the same barriers.
//   A       one step covers F::KSTEP k as F::FRAGS bf16x8 fragments per
//           m-tile at F::x_k / F::x_step, the k order the format's b_frag
//           produces.
//   scales  fp8: scale[e, col] multiplies the fp32 accumulator in the
//           epilogue, before the gate weight and the one rounding (GLU: gate
//           and up by their own rows' scales, then rounded, then
//           silu_mul_bf16). mxfp4: per step and column tile the destination
//           lane loads the 8 scale bytes of its row (n = lane & 15) for the
//           step's 256 k into F::Aux, on the default cache policy, and
//           b_frag's v_cvt_scalef32_pk_bf16_fp4 applies them. Scale rows are
//           clamped like W rows: tile columns past N read column N - 1.
// Requires K % (WPB * F::KSTEP * U) == 0, N % 16 == 0 (N % 32 for GLU).
template <class F, int WPB, int U, int NT, int MT, int EPI>
__global__ __launch_bounds__(WPB * 64) void moe_skinny_gemm_q_kernel(
    const short* __restrict__ a,          // gather: x [T, K]; direct: [P, K]
    const typename F::welem* __restrict__ w,
    const typename F::scale_t* __restrict__ scale,
    const int* __restrict__ seg_start,    // [E + 1]
    const int* __restrict__ pair_of,      // [P]
    const float* __restrict__ topw,       // [P] fp32, WEIGHTED only
    void* __restrict__ out,
    int N, int K, int topk, int gather) {
  using skinny::int4v;
  typedef typename F::Aux Aux;
  static_assert(MT <= 2, "longer segments go to further row chunks");
  constexpr bool kGlu = EPI == GLU;
  static_assert(!kGlu || NT % 2 == 0, "GLU pairs gate and up tiles");
  constexpr int CH = 16 * MT;             // segment rows per block
  const int e = blockIdx.y;
  const int seg0 = seg_start[e];
  const int z0 = blockIdx.z * CH;
  const int left = seg_start[e + 1] - seg0 - z0;
  if (left <= 0) return;                  // idle expert or chunk: nothing read
  const int s = seg0 + z0;
  const int cnt = left < CH ? left : CH;  // block-uniform

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;       // 0..WPB-1 = k-slice
  const int lr = lane & 15;
  const int lg = lane >> 4;
  constexpr int NTO = kGlu ? NT / 2 : NT; // column tiles of the output
  const int NO = kGlu ? N / 2 : N;        // columns of the output
  const int n0 = (blockIdx.x * NTO) * 16;
  if (n0 >= NO) return;
  auto live = [&](int m) { return m == 0 || 16 * m < cnt; };

  const int kw = K / WPB;
  const int k0 = wid * kw;
  const int steps = kw / F::KSTEP;

  const short* xp[MT];
#pragma unroll
  for (int m = 0; m < MT; m++) {
    const int r = m * 16 + lr;
    const int pos = s + (r < cnt ? r : 0);
    const int row = gather ? pair_of[pos] / topk : pos;
    xp[m] = a + (size_t)row * K + k0 + F::x_k(lane);
  }
  const size_t erow = (size_t)e * N;      // the expert's first weight row
  const typename F::welem* wp[NT][F::LOADS];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int h = 0; h < F::LOADS; h++) {
      int col = n0 + (t % NTO) * 16 + F::w_row(lane, h);
      col = col < NO ? col : NO - 1;
      if (kGlu && t >= NTO) col += NO;    // the up row of that column
      wp[t][h] = w + (erow + col) * (K / F::WPACK) + k0 / F::WPACK +
                 F::w_k(lane);
    }
  const typename F::scale_t* sp[NT];
  if constexpr (F::BLOCK_SCALED) {
#pragma unroll
    for (int t = 0; t < NT; t++) {
      int col = n0 + (t % NTO) * 16 + lr;
      col = col < NO ? col : NO - 1;
      if (kGlu && t >= NTO) col += NO;
      sp[t] = scale + ((erow + col) * K + k0) / 32;
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
  Aux auxbuf[NT][U];
  auto load_x = [&](bf16x8 (&x)[MT][F::FRAGS], int d) {
#pragma unroll
    for (int m = 0; m < MT; m++)
      if (live(m)) {
#pragma unroll
        for (int f = 0; f < F::FRAGS; f++)
          x[m][f] = *reinterpret_cast<const bf16x8*>(xp[m] + d * F::KSTEP +
                                                     F::x_step(f));
      }
  };
  auto load_w = [&](int4v (&r)[F::LOADS], Aux& ax, int t, int d) {
#pragma unroll
    for (int h = 0; h < F::LOADS; h++)
      r[h] = skinny::ldw<1>(wp[t][h] + d * (F::KSTEP / F::WPACK));
    if constexpr (F::BLOCK_SCALED)
      ax = *reinterpret_cast<const Aux*>(sp[t] + d * (F::KSTEP / 32));
  };
  auto consume = [&](const bf16x8 (&x)[MT][F::FRAGS],
                     const int4v (&r)[F::LOADS], Aux ax, f32x4 (&c)[MT]) {
#pragma unroll
    for (int f = 0; f < F::FRAGS; f++) {
      const bf16x8 b = F::b_frag(f, r, sel, ax);
#pragma unroll
      for (int m = 0; m < MT; m++)
        if (live(m))
          c[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[m][f], b, c[m],
                                                         0, 0, 0);
    }
  };

  // U steps in flight, as in moe_skinny_gemm_kernel.
#pragma unroll
  for (int u = 0; u < U; u++) {
    load_x(abuf[u], u);
#pragma unroll
    for (int t = 0; t < NT; t++) load_w(rbuf[t][u], auxbuf[t][u], t, u);
  }
  for (int d = U; d < steps; d += U) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      bf16x8 x[MT][F::FRAGS];
#pragma unroll
      for (int m = 0; m < MT; m++)
        if (live(m)) {
#pragma unroll
          for (int f = 0; f < F::FRAGS; f++) x[m][f] = abuf[u][m][f];
        }
      load_x(abuf[u], d + u);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        int4v r[F::LOADS];
#pragma unroll
        for (int h = 0; h < F::LOADS; h++) r[h] = rbuf[t][u][h];
        const Aux ax = auxbuf[t][u];
        load_w(rbuf[t][u], auxbuf[t][u], t, d + u);
        consume(x, r, ax, acc[t]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int t = 0; t < NT; t++)
      consume(abuf[u], rbuf[t][u], auxbuf[t][u], acc[t]);

  // Cross-wave reduction in wave order, one live m-tile at a time.
  __shared__ f32x4 red[WPB > 1 ? (WPB - 1) * NT * 64 : 1];
  if (WPB > 1) {
#pragma unroll
    for (int m = 0; m < MT; m++) {
      if (!live(m)) break;
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

  // The row scales of this lane's columns (fp8), gate tiles then up tiles.
  float sc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    sc[t] = 1.f;
    if constexpr (F::SCALED) {
      int col = n0 + (t % NTO) * 16 + lr;
      col = col < NO ? col : NO - 1;
      if (kGlu && t >= NTO) col += NO;
      sc[t] = scale[erow + col];
    }
  }
  // C layout: lane holds chunk row 16 m + lg*4 + i, column tilecol + lr.
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = m * 16 + lg * 4 + i;
      if (r >= cnt) continue;
      if constexpr (EPI == WEIGHTED) {
        const int p = pair_of[s + r];
        const float wt = topw[p];
        float* part = reinterpret_cast<float*>(out) + (size_t)p * N;
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const int col = n0 + t * 16 + lr;
          if (col < N) part[col] = acc[t][m][i] * sc[t] * wt;
        }
      } else {
        short* y = reinterpret_cast<short*>(out) + (size_t)(s + r) * NO;
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

// The (WPB, U, NT) points of the quantised routed GEMM, each at MT = 1, 2 and
// the three epilogues; U counts steps of F::KSTEP k (128 fp8, 256 mxfp4), NT
// is even, and (1, 1, 2) accepts every K % F::KSTEP == 0. None uses scratch
// memory (profiles/README.md, "Routed MoE decode"); mxfp4 (8, 1, 4) would,
// 224 B per lane at MT = 2, and is not built.
#define MOE_DECODE_FP8_CONFIGS(X)                                           \
  X(1, 1, 2) X(1, 2, 2) X(2, 1, 4) X(2, 2, 2) X(4, 1, 2) X(4, 2, 2)          \
  X(4, 1, 4) X(8, 1, 2)
#define MOE_DECODE_MXFP4_CONFIGS(X)                                         \
  X(1, 1, 2) X(1, 2, 2) X(2, 1, 2) X(2, 1, 4) X(4, 1, 2) X(4, 1, 4)          \
  X(8, 1, 2)

// The (WPB, U, NT) points the binding can launch, each at MT = 1..4 and the
// three epilogues; U counts 64-k steps, NT is even so that every point has a
// GLU form, and (1, 1, 2) accepts every K % 64 == 0. None uses scratch
// memory (profiles/README.md, "Routed MoE decode", lists registers and
// occupancy).
#define MOE_DECODE_CONFIGS(X)                                               \
  X(1, 1, 2) X(1, 2, 2) X(1, 2, 4) X(2, 2, 2) X(4, 1, 2) X(4, 2, 2)          \
  X(4, 1, 4) X(8, 1, 2)

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace moe_decode

namespace {

struct RoutedArgs {
  const short* a;
  const short* w;
  const int* seg_start;
  const int* pair_of;
  const float* topw;
  void* out;
  int T, E, N, K, topk, gather;
};

// Launches <WPB, U, NT, EPI> at ceil(T / 16) accumulator tiles: distinct
// experts per token bound every segment by T rows.
template <int WPB, int U, int NT, int MT, int EPI>
void launch(const RoutedArgs& r) {
  if constexpr (MT > 1) {
    if (r.T <= (MT - 1) * 16) return launch<WPB, U, NT, MT - 1, EPI>(r);
  }
  const int NO = EPI == moe_decode::GLU ? r.N / 2 : r.N;
  constexpr int cols = (EPI == moe_decode::GLU ? NT / 2 : NT) * 16;
  const dim3 grid((NO + cols - 1) / cols, r.E);
  moe_decode::moe_skinny_gemm_kernel<WPB, U, NT, MT, EPI>
      <<<grid, WPB * 64, 0, at::cuda::getCurrentHIPStream()>>>(
          r.a, r.w, r.seg_start, r.pair_of, r.topw, r.out, r.N, r.K, r.topk,
          r.gather);
}

template <int EPI>
void dispatch(const RoutedArgs& r, int64_t wpb, int64_t u, int64_t nt) {
#define MOE_CASE(WPB, U, NT)                                                 \
  if (wpb == WPB && u == U && nt == NT) return launch<WPB, U, NT, 4, EPI>(r);
  MOE_DECODE_CONFIGS(MOE_CASE)
#undef MOE_CASE
  TORCH_CHECK(false, "moe_routed_gemm: no kernel for (WPB, U, NT) = (", wpb,
              ", ", u, ", ", nt, ")");
}

bool i32_vec(const torch::Tensor& t) {
  return t.is_cuda() && t.dtype() == torch::kInt32 && t.is_contiguous();
}

struct QuantArgs {
  RoutedArgs r;         // r.w unused
  const void* wq;
  const void* scale;
};

// Launches <F, WPB, U, NT, EPI>: one 16-row tile and one chunk for T <= 16,
// else 32-row chunks on grid.z (distinct experts per token bound every
// segment by T rows).
template <class F, int WPB, int U, int NT, int EPI>
void launch_q(const QuantArgs& q) {
  const RoutedArgs& r = q.r;
  const int NO = EPI == moe_decode::GLU ? r.N / 2 : r.N;
  constexpr int cols = (EPI == moe_decode::GLU ? NT / 2 : NT) * 16;
  const unsigned gx = (NO + cols - 1) / cols;
  const auto* wq = static_cast<const typename F::welem*>(q.wq);
  const auto* sc = static_cast<const typename F::scale_t*>(q.scale);
  auto stream = at::cuda::getCurrentHIPStream();
  if (r.T <= 16)
    moe_decode::moe_skinny_gemm_q_kernel<F, WPB, U, NT, 1, EPI>
        <<<dim3(gx, r.E, 1), WPB * 64, 0, stream>>>(
            r.a, wq, sc, r.seg_start, r.pair_of, r.topw, r.out, r.N, r.K,
            r.topk, r.gather);
  else
    moe_decode::moe_skinny_gemm_q_kernel<F, WPB, U, NT, 2, EPI>
        <<<dim3(gx, r.E, (r.T + 31) / 32), WPB * 64, 0, stream>>>(
            r.a, wq, sc, r.seg_start, r.pair_of, r.topw, r.out, r.N, r.K,
            r.topk, r.gather);
}

template <class F, int EPI>
void dispatch_q(const char* name, const QuantArgs& q, int64_t wpb, int64_t u,
                int64_t nt) {
#define MOE_CASE(WPB, U, NT)                                                 \
  if (wpb == WPB && u == U && nt == NT) return launch_q<F, WPB, U, NT, EPI>(q);
  if constexpr (std::is_same<F, skinny::Fp8Coal>::value) {
    MOE_DECODE_FP8_CONFIGS(MOE_CASE)
  } else {
    MOE_DECODE_MXFP4_CONFIGS(MOE_CASE)
  }
#undef MOE_CASE
  TORCH_CHECK(false, name, ": no kernel for (WPB, U, NT) = (", wpb, ", ", u,
              ", ", nt, ")");
}

// The checks and the launch of moe_routed_gemm_fp8 / _mxfp4; the callers have
// checked the dtypes of wq and scale.
template <class F>
void routed_quant(const char* name, torch::Tensor out, torch::Tensor a,
                  torch::Tensor wq, torch::Tensor scale,
                  torch::Tensor seg_start, torch::Tensor pair_of,
                  c10::optional<torch::Tensor> topw, int64_t topk, bool gather,
                  int64_t epilogue, int64_t wpb, int64_t u, int64_t nt) {
  TORCH_CHECK(epilogue >= 0 && epilogue <= 2, name, ": bad epilogue");
  const bool glu = epilogue == moe_decode::GLU;
  const bool weighted = epilogue == moe_decode::WEIGHTED;
  TORCH_CHECK(a.is_cuda() && wq.is_cuda() && scale.is_cuda() && out.is_cuda() &&
                  i32_vec(seg_start) && i32_vec(pair_of),
              name, ": tensors must be on the GPU, seg_start and pair_of "
              "contiguous int32");
  TORCH_CHECK(a.dtype() == torch::kBFloat16 &&
                  out.dtype() == (weighted ? torch::kFloat32
                                           : torch::kBFloat16),
              name, ": a bf16, out bf16 (fp32 if weighted)");
  TORCH_CHECK(a.dim() == 2 && wq.dim() == 3 && out.dim() == 2 &&
                  scale.dim() == (F::BLOCK_SCALED ? 3 : 2) &&
                  seg_start.dim() == 1 && pair_of.dim() == 1,
              name, ": a [rows, K], codes [E, N, K / ", F::WPACK,
              "], scale [E, N", F::BLOCK_SCALED ? ", K / 32]" : "]",
              ", out [P, cols]");
  TORCH_CHECK(a.is_contiguous() && wq.is_contiguous() &&
                  scale.is_contiguous() && out.is_contiguous(),
              name, ": tensors must be contiguous");
  const int64_t P = pair_of.size(0), E = wq.size(0), N = wq.size(1),
                K = wq.size(2) * F::WPACK;
  TORCH_CHECK(topk >= 1 && topk <= moe_decode::MAX_TOPK && P >= 1 &&
                  P % topk == 0 && P / topk <= moe_decode::MAX_T && E >= 1 &&
                  E <= moe_decode::MAX_E && seg_start.size(0) == E + 1,
              name, ": needs T <= 64, topk <= 8, E <= 64 and seg_start "
              "[E + 1]");
  const int64_t T = P / topk;
  TORCH_CHECK(a.size(1) == K && a.size(0) == (gather ? T : P) &&
                  out.size(0) == P && out.size(1) == (glu ? N / 2 : N) &&
                  scale.size(0) == E && scale.size(1) == N &&
                  (!F::BLOCK_SCALED || scale.size(2) * 32 == K),
              name, ": shape mismatch");
  TORCH_CHECK(N >= 16 && N % 16 == 0 && N < (1 << 27) && (!glu || N % 32 == 0),
              name, ": needs N % 16 == 0 (N % 32 for the SwiGLU form), got ",
              N);
  TORCH_CHECK(wpb > 0 && u > 0 && nt > 0, name, ": bad configuration");
  const int64_t kstep = wpb * F::KSTEP * u;
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
  const QuantArgs q{{(const short*)a.data_ptr(), nullptr,
                     (const int*)seg_start.data_ptr(),
                     (const int*)pair_of.data_ptr(), tw, out.data_ptr(),
                     (int)T, (int)E, (int)N, (int)K, (int)topk,
                     gather ? 1 : 0},
                    wq.data_ptr(), scale.data_ptr()};
  if (glu) dispatch_q<F, moe_decode::GLU>(name, q, wpb, u, nt);
  else if (weighted) dispatch_q<F, moe_decode::WEIGHTED>(name, q, wpb, u, nt);
  else dispatch_q<F, moe_decode::PLAIN>(name, q, wpb, u, nt);
  HIP_CHECK_KERNEL();
}

}  // namespace

// topi [T, K] int32 -> seg_start [E + 1], pair_of [T K], both int32.
void moe_route(torch::Tensor topi, torch::Tensor seg_start,
               torch::Tensor pair_of) {
  TORCH_CHECK(i32_vec(topi) && i32_vec(seg_start) && i32_vec(pair_of) &&
                  topi.dim() == 2 && seg_start.dim() == 1 &&
                  pair_of.dim() == 1,
              "moe_route: topi [T, K], seg_start [E + 1], pair_of [T K], "
              "contiguous int32 on the GPU");
  const int64_t T = topi.size(0), K = topi.size(1), E = seg_start.size(0) - 1;
  TORCH_CHECK(T >= 1 && T <= moe_decode::MAX_T && K >= 1 &&
                  K <= moe_decode::MAX_TOPK && E >= 1 &&
                  E <= moe_decode::MAX_E,
              "moe_route: needs 1 <= T <= 64, 1 <= K <= 8, 1 <= E <= 64, got "
              "T = ", T, ", K = ", K, ", E = ", E);
  TORCH_CHECK(pair_of.size(0) == T * K, "moe_route: pair_of must hold T K");
  moe_decode::moe_route_kernel<<<1, moe_decode::ROUTE_THREADS, 0,
                                 at::cuda::getCurrentHIPStream()>>>(
      (const int*)topi.data_ptr(), (int*)seg_start.data_ptr(),
      (int*)pair_of.data_ptr(), (int)(T * K), (int)E);
  HIP_CHECK_KERNEL();
}

// epilogue 0: out bf16 [P, N]; 1 (GLU): out bf16 [P, N / 2]; 2 (WEIGHTED):
// out fp32 [P, N], topw fp32 with P elements. a is x [T, K] if gather, else
// [P, K] in sorted order. P = pair_of's length = T topk.
void moe_routed_gemm(torch::Tensor out, torch::Tensor a, torch::Tensor w,
                     torch::Tensor seg_start, torch::Tensor pair_of,
                     c10::optional<torch::Tensor> topw, int64_t topk,
                     bool gather, int64_t epilogue, int64_t wpb, int64_t u,
                     int64_t nt) {
  const char* name = "moe_routed_gemm";
  TORCH_CHECK(epilogue >= 0 && epilogue <= 2, name, ": bad epilogue");
  const bool glu = epilogue == moe_decode::GLU;
  const bool weighted = epilogue == moe_decode::WEIGHTED;
  TORCH_CHECK(a.is_cuda() && w.is_cuda() && out.is_cuda() &&
                  i32_vec(seg_start) && i32_vec(pair_of),
              name, ": tensors must be on the GPU, seg_start and pair_of "
              "contiguous int32");
  TORCH_CHECK(a.dtype() == torch::kBFloat16 && w.dtype() == torch::kBFloat16 &&
                  out.dtype() == (weighted ? torch::kFloat32
                                           : torch::kBFloat16),
              name, ": a and w bf16, out bf16 (fp32 if weighted)");
  TORCH_CHECK(a.dim() == 2 && w.dim() == 3 && out.dim() == 2 &&
                  seg_start.dim() == 1 && pair_of.dim() == 1,
              name, ": a [rows, K], w [E, N, K], out [P, cols]");
  TORCH_CHECK(a.is_contiguous() && w.is_contiguous() && out.is_contiguous(),
              name, ": tensors must be contiguous");
  const int64_t P = pair_of.size(0), E = w.size(0), N = w.size(1),
                K = w.size(2);
  TORCH_CHECK(topk >= 1 && topk <= moe_decode::MAX_TOPK && P >= 1 &&
                  P % topk == 0 && P / topk <= moe_decode::MAX_T && E >= 1 &&
                  E <= moe_decode::MAX_E && seg_start.size(0) == E + 1,
              name, ": needs T <= 64, topk <= 8, E <= 64 and seg_start "
              "[E + 1]");
  const int64_t T = P / topk;
  TORCH_CHECK(a.size(1) == K && a.size(0) == (gather ? T : P) &&
                  out.size(0) == P && out.size(1) == (glu ? N / 2 : N),
              name, ": shape mismatch");
  TORCH_CHECK(N >= 16 && N % 16 == 0 && N < (1 << 27) && (!glu || N % 32 == 0),
              name, ": needs N % 16 == 0 (N % 32 for the SwiGLU form), got ",
              N);
  TORCH_CHECK(wpb > 0 && u > 0 && nt > 0, name, ": bad configuration");
  const int64_t kstep = wpb * 64 * u;
  TORCH_CHECK(K >= kstep && K < (1 << 30) && K % kstep == 0, name,
              ": needs K % ", kstep, " == 0, got ", K);
  TORCH_CHECK((uintptr_t)a.data_ptr() % 16 == 0 &&
                  (uintptr_t)w.data_ptr() % 16 == 0,
              name, ": a and w must be 16 B aligned");
  const float* tw = nullptr;
  if (weighted) {
    TORCH_CHECK(topw.has_value() && topw->is_cuda() &&
                    topw->dtype() == torch::kFloat32 &&
                    topw->is_contiguous() && topw->numel() == P,
                name, ": the weighted form needs topw fp32 with T topk "
                "elements");
    tw = (const float*)topw->data_ptr();
  }
  const RoutedArgs r{(const short*)a.data_ptr(), (const short*)w.data_ptr(),
                     (const int*)seg_start.data_ptr(),
                     (const int*)pair_of.data_ptr(), tw, out.data_ptr(),
                     (int)T, (int)E, (int)N, (int)K, (int)topk,
                     gather ? 1 : 0};
  if (glu) dispatch<moe_decode::GLU>(r, wpb, u, nt);
  else if (weighted) dispatch<moe_decode::WEIGHTED>(r, wpb, u, nt);
  else dispatch<moe_decode::PLAIN>(r, wpb, u, nt);
  HIP_CHECK_KERNEL();
}

// moe_routed_gemm for W8A16 experts: wq float8_e4m3fn [E, N, K], scale fp32
// [E, N]; (wpb, u, nt) a point of MOE_DECODE_FP8_CONFIGS, K % (wpb 128 u) == 0.
void moe_routed_gemm_fp8(torch::Tensor out, torch::Tensor a, torch::Tensor wq,
                         torch::Tensor scale, torch::Tensor seg_start,
                         torch::Tensor pair_of,
                         c10::optional<torch::Tensor> topw, int64_t topk,
                         bool gather, int64_t epilogue, int64_t wpb, int64_t u,
                         int64_t nt) {
  const char* name = "moe_routed_gemm_fp8";
  TORCH_CHECK(wq.dtype() == at::kFloat8_e4m3fn &&
                  scale.dtype() == torch::kFloat32,
              name, ": wq must be float8_e4m3fn, scale fp32");
  routed_quant<skinny::Fp8Coal>(name, out, a, wq, scale, seg_start, pair_of,
                                topw, topk, gather, epilogue, wpb, u, nt);
}

// moe_routed_gemm for W4A16 experts: q uint8 [E, N, K / 2], scale uint8 (e8m0)
// [E, N, K / 32]; a point of MOE_DECODE_MXFP4_CONFIGS, K % (wpb 256 u) == 0.
void moe_routed_gemm_mxfp4(torch::Tensor out, torch::Tensor a, torch::Tensor q,
                           torch::Tensor scale, torch::Tensor seg_start,
                           torch::Tensor pair_of,
                           c10::optional<torch::Tensor> topw, int64_t topk,
                           bool gather, int64_t epilogue, int64_t wpb,
                           int64_t u, int64_t nt) {
  const char* name = "moe_routed_gemm_mxfp4";
  TORCH_CHECK(q.dtype() == torch::kUInt8 && scale.dtype() == torch::kUInt8,
              name, ": q and scale must be uint8");
  routed_quant<skinny::Mxfp4Coal>(name, out, a, q, scale, seg_start, pair_of,
                                  topw, topk, gather, epilogue, wpb, u, nt);
}

// out [T, D] bf16 = sum over the topk rows of part [T topk, D] fp32.
void moe_combine(torch::Tensor out, torch::Tensor part, int64_t topk) {
  TORCH_CHECK(out.is_cuda() && part.is_cuda() &&
                  out.dtype() == torch::kBFloat16 &&
                  part.dtype() == torch::kFloat32 && out.dim() == 2 &&
                  part.dim() == 2 && out.is_contiguous() &&
                  part.is_contiguous(),
              "moe_combine: out [T, D] bf16, part [T topk, D] fp32, "
              "contiguous on the GPU");
  const int64_t T = out.size(0), D = out.size(1);
  TORCH_CHECK(topk >= 1 && part.size(0) == T * topk && part.size(1) == D &&
                  T >= 1 && D >= 8 && D % 8 == 0 && T * D < (1ll << 31),
              "moe_combine: needs part [T topk, D] and D % 8 == 0");
  TORCH_CHECK((uintptr_t)out.data_ptr() % 16 == 0 &&
                  (uintptr_t)part.data_ptr() % 16 == 0,
              "moe_combine: out and part must be 16 B aligned");
  const int64_t threads = T * (D / 8);
  moe_decode::moe_combine_kernel<<<(unsigned)((threads + 255) / 256), 256, 0,
                                   at::cuda::getCurrentHIPStream()>>>(
      (short*)out.data_ptr(), (const float*)part.data_ptr(), (int)T, (int)D,
      (int)topk);
  HIP_CHECK_KERNEL();
}

// The (WPB, U, NT) table, for the Python side to check its copy against.
std::vector<std::tuple<int, int, int>> moe_decode_configs() {
#define MOE_ENTRY(WPB, U, NT) {WPB, U, NT},
  return {MOE_DECODE_CONFIGS(MOE_ENTRY)};
}

// The same per quantised format: {"fp8": [...], "mxfp4": [...]}.
std::map<std::string, std::vector<std::tuple<int, int, int>>>
moe_decode_quant_configs() {
  return {{"fp8", {MOE_DECODE_FP8_CONFIGS(MOE_ENTRY)}},
          {"mxfp4", {MOE_DECODE_MXFP4_CONFIGS(MOE_ENTRY)}}};
#undef MOE_ENTRY
}
