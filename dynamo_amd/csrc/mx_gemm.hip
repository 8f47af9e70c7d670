// W8A8 / W4A8 prefill GEMM for MI355X/gfx950 on the block-scaled fp8/fp4 MFMA
// (v_mfma_scale_f32_16x16x128_f8f6f4), and the activation quantiser in front
// of it.
//   mxfp8_quantize_rows: x bf16 [M,K] -> xq e4m3 [M,K], xs e8m0 [M,K/32]
//   fp8_mx_gemm:   y[M,N] = bf16((dq(xq,xs) @ wq[N,K]^T) * scale[n])
//   mxfp4_mx_gemm: y[M,N] = dq(xq,xs) @ W_eff[N,K]^T
// y bf16, fp32 accumulate, any M >= 1, N % 16 == 0, K % 128 == 0; `glu` as in
// skinny_gemm.hip. ops/mxfp8.py defines the activation format and the
// quantiser's bytes.
//
// The instruction. One MFMA multiplies a 16 x 128 fp8 A tile by a 128 x 16
// fp8 (blgp 0) or fp4 (blgp 4) B tile. Lane l = (lg, lr) supplies row /
// column lr = l & 15. Of an fp8 operand its VGPRs 0-3 hold the 16 k from
// 16 lg and VGPRs 4-7 the 16 k from 64 + 16 lg; of an fp4 operand VGPRs 0-3
// hold the 32 k from 32 lg. The lane's scale operand is the e8m0 byte of MX
// block lg (k from 32 lg) of its row, whichever k its data registers hold.
// (Measured, not read: with the 32 k of an fp8 lane taken as consecutive,
// the layout probe of tests/test_gpu_mx_gemm.py got the scale of block
// lg / 2 + 2 h applied to half h of lane lg.) Every fragment is still two
// (or one) 16 B chunks of the stored rows, and the scale byte is replicated
// over the scale register, so the result does not depend on op_sel. An
// Fp8Weight has no block scales: B's scale operand is 127 (1.0) and the fp32
// scale[n] multiplies the accumulator in the epilogue, before the single
// rounding to bf16. There is no conversion instruction in the loop.
//
// Work split. A block of WM x WN waves owns a BM x BN tile of y; wave
// (wm, wn) owns BM / WM rows x BN / WN columns as TM x TN 16 x 16 accumulator
// tiles. Per k-step of 128 a wave reads its TN B fragments once and each of
// its TM A fragments once: an A fragment feeds TN MFMAs, a B fragment TM.
//
// Data movement. Per k-step the block copies the [BM, 128 B] slab of xq and
// the [BN, 128 B] (fp8) or [BN, 64 B] (fp4) slab of W into LDS, 16 B per
// thread and pass, a wave's loads running along full rows. Two stages: the
// global loads of step i + 1 are issued before the MFMAs of step i, stored to
// the other stage after them, and one barrier ends the step. Rows >= M and
// columns >= N are zero-filled and never dereferenced. The scale bytes are
// not staged: per k-step a lane loads one dword (the step's four blocks) per
// row tile and per column tile and shifts its own block's byte out; the 16
// lanes of a block share the address.
//
// Swizzle. A slab row is CH = 8 (or 4) chunks of 16 B, so 16 / CH rows fill
// one 256 B line of the 64 banks. Chunk c of row r lives at chunk
// c ^ ((r / (16 / CH)) & (CH - 1)). On paper: a fragment read has 16 lanes
// (rows r0 + 0..15, r0 % 16 == 0) on one chunk index c; r % (16 / CH) picks
// the row's place in the line and the XOR term runs over all CH values, so
// the 16 lanes hit the line's 16 slots once each. Unswizzled they would share
// 16 / CH slots. A copy store has 16 consecutive lanes on the CH chunks of
// 16 / CH consecutive rows: a permutation of one line.
//
// Launch order. Blocks are numbered in groups of 8 M tiles: inside a group
// consecutive blocks walk the group's M tiles of one column tile, then the
// next column tile, so concurrent blocks share one W slab and 8 x slabs in L2.
//
// Order of sums. One accumulator per (row, column) takes the k-steps
// ascending: row m of y does not depend on M, the point's BM or the launch
// order, and runs are bit-reproducible. No atomics.
#include "common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace mxg {

typedef __attribute__((ext_vector_type(2))) int int2v;
typedef __attribute__((ext_vector_type(4))) int int4v;
typedef __attribute__((ext_vector_type(8))) int int8v;

constexpr int KSTEP = 128;   // k per MFMA and per pipeline step
constexpr int GROUP_M = 8;   // M tiles per raster group

// ---- the activation quantiser -------------------------------------------
// A thread takes 8 consecutive bf16 (16 B), four threads one MX block; the
// block's amax goes through two quad_perm DPP steps. amax is taken on the
// bf16 bit patterns (monotone for finite values), floor(log2(amax)) is its
// exponent field, and x * 2^-e is exact in fp32, so the bytes are those of
// ops.mxfp8.quantize_mxfp8_rows. Requires K % 32 == 0: a quad never spans two
// rows and `chunks` = M K / 8 is a multiple of 4.
__global__ __launch_bounds__(256) void mxfp8_quantize_rows_kernel(
    const short* __restrict__ x, uint8_t* __restrict__ xq,
    uint8_t* __restrict__ xs, size_t chunks) {
#if defined(__HIP_DEVICE_COMPILE__)
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = c < chunks;
  short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) v = *reinterpret_cast<const short8*>(x + c * 8);
  int amax = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) amax = max(amax, (int)v[j] & 0x7fff);
  amax = max(amax, __builtin_amdgcn_update_dpp(0, amax, 0xB1, 0xf, 0xf, false));
  amax = max(amax, __builtin_amdgcn_update_dpp(0, amax, 0x4E, 0xf, 0xf, false));
  // e = floor(log2(amax)) - 7 clamped below at -126 (a bf16 subnormal amax
  // has exponent field 0 and clamps too); 0 for an all-zero block
  const int e = amax ? max((amax >> 7) - 134, -126) : 0;
  const float inv = __builtin_bit_cast(float, (127 - e) << 23);   // 2^-e
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; j++) f[j] = bf16_to_f32(v[j]) * inv;
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  if (live) {
    *reinterpret_cast<int2v*>(xq + c * 8) = int2v{lo, hi};
    if ((threadIdx.x & 3) == 0) xs[c >> 2] = (uint8_t)(e + 127);
  }
#endif
}

// ---- the B formats --------------------------------------------------------
struct Fp8B {     // Fp8Weight: e4m3 [N, K], one fp32 scale per row
  static constexpr int ROWB = 128;   // bytes of 128 k of one row
  static constexpr int BLGP = 0;
  static constexpr bool BLOCK_SCALED = false;
};
struct Mxfp4B {   // Mxfp4Weight: e2m1 [N, K/2], e8m0 [N, K/32]
  static constexpr int ROWB = 64;
  static constexpr int BLGP = 4;
  static constexpr bool BLOCK_SCALED = true;
};

template <class F, int BM, int BN>
constexpr int kLdsBytes = 2 * (BM * KSTEP + BN * F::ROWB);   // two stages

// Built without the packed fp32 VALU forms, as quant_tile_gemm.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// Requires K % 128 == 0, M >= 1, N % 16 == 0 (N % 32 if GLU), M K / 32 and
// N K / 32 < 2^31, gridDim.x = mtiles * ntiles, kLdsBytes of dynamic LDS.
// GLU: the block's B slab is BN / 2 gate rows followed by their BN / 2 up
// rows, a wave's tiles t >= TN / 2 are the up tiles of t - TN / 2, and y is
// [M, N / 2].
template <class F, int BM, int BN, int WM, int WN, int GLU>
__global__ __launch_bounds__(WM * WN * 64) void mx_gemm_kernel(
    const uint8_t* __restrict__ xq,       // [M, K] e4m3
    const uint8_t* __restrict__ xs,       // [M, K / 32] e8m0
    const uint8_t* __restrict__ w,        // [N, K] e4m3 or [N, K / 2] e2m1
    const void* __restrict__ wscale,      // fp32 [N] or e8m0 [N, K / 32]
    short* __restrict__ y,                // [M, N] ([M, N / 2] if GLU)
    int M, int N, int K, int mtiles, int ntiles) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int T = WM * WN * 64;
  constexpr int WMR = BM / WM, WNC = BN / WN;    // a wave's rows and columns
  constexpr int TM = WMR / 16, TN = WNC / 16;
  constexpr int TNO = GLU ? TN / 2 : TN;         // column tiles of y per wave
  constexpr int BNO = GLU ? BN / 2 : BN;         // columns of y per block
  constexpr int ACH = KSTEP / 16, BCH = F::ROWB / 16;   // chunks per slab row
  constexpr int APR = T / ACH, AP = BM / APR;    // rows per pass, passes
  constexpr int BPR = T / BCH, BP = BN / BPR;
  constexpr int A_BYTES = BM * KSTEP, B_BYTES = BN * F::ROWB;
  constexpr int STAGE = A_BYTES + B_BYTES;
  static_assert(WMR % 16 == 0 && WNC % 16 == 0 && T <= 512, "wave tiles");
  static_assert(!GLU || TN % 2 == 0, "GLU pairs gate and up tiles");
  static_assert(BM % APR == 0 && BN % BPR == 0, "whole copy passes");
  static_assert(kLdsBytes<F, BM, BN> <= 160 * 1024, "gfx950 LDS");
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wm = (tid >> 6) / WN, wn = (tid >> 6) % WN;
  const int lr = lane & 15, lg = lane >> 4;

  // grouped raster (see the head of the file)
  const int per_group = GROUP_M * ntiles;
  const int first_m = (blockIdx.x / per_group) * GROUP_M;
  const int gsz = min(mtiles - first_m, GROUP_M);
  const int rem = blockIdx.x % per_group;
  const int m0 = (first_m + rem % gsz) * BM;
  const int nb = (rem / gsz) * BNO;              // first column of y
  const int NO = GLU ? N / 2 : N;                // columns of y
  const int SK = K / 32;                         // scale bytes per row

  // W row behind slab row r, or -1 past the last column
  auto w_row = [&](int r) {
    const int up = GLU && r >= BN / 2;
    const int col = nb + (up ? r - BN / 2 : r);
    return col < NO ? col + (up ? NO : 0) : -1;
  };
  // first slab row of the wave's column tile t
  auto b_slab = [&](int t) {
    if (!GLU) return wn * WNC + t * 16;
    return (t < TNO ? 0 : BN / 2) + wn * (WNC / 2) + (t % TNO) * 16;
  };

  // ---- the copies: chunk cc of slab rows cr + pass * rows-per-pass ----
  const int acr = tid / ACH, acc_ = tid % ACH;
  const int bcr = tid / BCH, bcc = tid % BCH;
  const uint8_t* ap[AP];   // null: zero-fill
  const uint8_t* bp[BP];
#pragma unroll
  for (int p = 0; p < AP; p++) {
    const int row = m0 + acr + p * APR;
    ap[p] = row < M ? xq + (size_t)row * K + acc_ * 16 : nullptr;
  }
#pragma unroll
  for (int p = 0; p < BP; p++) {
    const int row = w_row(bcr + p * BPR);
    bp[p] = row >= 0 ? w + (size_t)row * (K / KSTEP * F::ROWB) + bcc * 16
                     : nullptr;
  }
  // scale dwords: rows and columns past the end read the last one's
  int sao[TM], sbo[TN];
#pragma unroll
  for (int m = 0; m < TM; m++)
    sao[m] = min(m0 + wm * WMR + m * 16 + lr, M - 1) * SK;
#pragma unroll
  for (int t = 0; t < TN; t++) {
    const int row = w_row(b_slab(t) + lr);
    sbo[t] = (row >= 0 ? row : N - 1) * SK;
  }

  int4v ga[AP], gb[BP];
  unsigned nsa[TM], nsb[TN];
  auto fetch = [&](int step) {
#pragma unroll
    for (int p = 0; p < AP; p++) {
      ga[p] = int4v{0, 0, 0, 0};
      if (ap[p])
        ga[p] = *reinterpret_cast<const int4v*>(ap[p] + step * KSTEP);
    }
#pragma unroll
    for (int p = 0; p < BP; p++) {
      gb[p] = int4v{0, 0, 0, 0};
      if (bp[p])
        gb[p] = *reinterpret_cast<const int4v*>(bp[p] + step * F::ROWB);
    }
#pragma unroll
    for (int m = 0; m < TM; m++)
      nsa[m] = *reinterpret_cast<const unsigned*>(xs + sao[m] + step * 4);
    if constexpr (F::BLOCK_SCALED) {
#pragma unroll
      for (int t = 0; t < TN; t++)
        nsb[t] = *reinterpret_cast<const unsigned*>(
            (const uint8_t*)wscale + sbo[t] + step * 4);
    }
  };
  auto store = [&](int stage) {
    char* sa = lds + stage * STAGE;
#pragma unroll
    for (int p = 0; p < AP; p++) {
      const int row = acr + p * APR;
      *reinterpret_cast<int4v*>(
          sa + row * KSTEP +
          ((acc_ ^ ((row / (16 / ACH)) & (ACH - 1))) << 4)) = ga[p];
    }
#pragma unroll
    for (int p = 0; p < BP; p++) {
      const int row = bcr + p * BPR;
      *reinterpret_cast<int4v*>(
          sa + A_BYTES + row * F::ROWB +
          ((bcc ^ ((row / (16 / BCH)) & (BCH - 1))) << 4)) = gb[p];
    }
  };
  // the lane's block's byte of a step's scale dword, in all four bytes
  auto own_scale = [&](unsigned dword) {
    return ((dword >> (8 * lg)) & 0xffu) * 0x01010101u;
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int m = 0; m < TM; m++)
#pragma unroll
    for (int t = 0; t < TN; t++) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment addresses: every slab base is a multiple of 16 rows, so the
  // swizzle term of a lane's row depends on lr alone
  const int a_off = (wm * WMR + lr) * KSTEP;
  const int a_swz = (lr / (16 / ACH)) & (ACH - 1);
  const int b_swz = (lr / (16 / BCH)) & (BCH - 1);

  auto compute = [&](int stage, const unsigned (&sa)[TM],
                     const unsigned (&sb)[TN]) {
    const char* s = lds + stage * STAGE;
    int8v b[TN];
#pragma unroll
    for (int t = 0; t < TN; t++) {
      const char* rp = s + A_BYTES + (b_slab(t) + lr) * F::ROWB;
      int4v lo, hi = int4v{0, 0, 0, 0};
      if constexpr (F::ROWB == 128) {
        lo = *reinterpret_cast<const int4v*>(rp + ((lg ^ b_swz) << 4));
        hi = *reinterpret_cast<const int4v*>(rp + (((lg + 4) ^ b_swz) << 4));
      } else {
        lo = *reinterpret_cast<const int4v*>(rp + ((lg ^ b_swz) << 4));
      }
      b[t] = int8v{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    }
#pragma unroll
    for (int m = 0; m < TM; m++) {
      const char* rp = s + a_off + m * 16 * KSTEP;
      const int4v lo =
          *reinterpret_cast<const int4v*>(rp + ((lg ^ a_swz) << 4));
      const int4v hi =
          *reinterpret_cast<const int4v*>(rp + (((lg + 4) ^ a_swz) << 4));
      const int8v a = int8v{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int t = 0; t < TN; t++)
        acc[m][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a, b[t], acc[m][t], 0, F::BLGP, 0, (int)sa[m], 0, (int)sb[t]);
    }
  };

  const int steps = K / KSTEP;
  unsigned sa[TM], sb[TN];
  fetch(0);
  store(0);
  __syncthreads();
  for (int step = 0; step < steps; step++) {
    const int stage = step & 1;
    const bool more = step + 1 < steps;
#pragma unroll
    for (int m = 0; m < TM; m++) sa[m] = own_scale(nsa[m]);
#pragma unroll
    for (int t = 0; t < TN; t++)
      sb[t] = F::BLOCK_SCALED ? own_scale(nsb[t]) : 0x7f7f7f7fu;
    if (more) fetch(step + 1);
    compute(stage, sa, sb);
    if (more) store(stage ^ 1);
    // step's reads of `stage` are done before step + 1 overwrites it
    __syncthreads();
  }

  // C layout: lane holds rows 16 m + lg 4 + i, i = 0..3, of column lr.
  const int row0 = m0 + wm * WMR + lg * 4;
  const int col0 = nb + wn * (GLU ? WNC / 2 : WNC) + lr;
  const float* rs = (const float*)wscale;
  if constexpr (GLU) {
#pragma unroll
    for (int t = 0; t < TNO; t++) {
      const int col = col0 + t * 16;
      if (col >= NO) continue;
      float sg = 1.f, su = 1.f;
      if constexpr (!F::BLOCK_SCALED) { sg = rs[col]; su = rs[col + NO]; }
#pragma unroll
      for (int m = 0; m < TM; m++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int row = row0 + m * 16 + i;
          if (row < M) {
            float g = acc[m][t][i], u = acc[m][t + TNO][i];
            if constexpr (!F::BLOCK_SCALED) { g *= sg; u *= su; }
            y[(size_t)row * NO + col] =
                silu_mul_bf16(f32_to_bf16(g), f32_to_bf16(u));
          }
        }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < TN; t++) {
    const int col = col0 + t * 16;
    if (col >= N) continue;
    float sc = 1.f;
    if constexpr (!F::BLOCK_SCALED) sc = rs[col];
#pragma unroll
    for (int m = 0; m < TM; m++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int row = row0 + m * 16 + i;
        if (row < M) {
          float v = acc[m][t][i];
          if constexpr (!F::BLOCK_SCALED) v *= sc;
          y[(size_t)row * N + col] = f32_to_bf16(v);
        }
      }
  }
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// The (BM, BN, WM, WN) points the bindings can launch, for both formats;
// every one accepts every K % 128 == 0 and has a GLU form.
// ops/__init__.py keeps a copy.
#define MX_GEMM_CONFIGS(X)                                                  \
  X(128, 128, 2, 2) X(256, 128, 2, 2) X(256, 128, 4, 2) X(128, 256, 2, 2)

}  // namespace mxg

namespace {

struct MxArgs {
  const uint8_t* xq;
  const uint8_t* xs;
  const uint8_t* w;
  const void* scale;
  short* y;
  int M, N, K;
  int64_t bm, bn, wm, wn;
  bool glu;
};

MxArgs check_args(const char* name, const torch::Tensor& y,
                  const torch::Tensor& xq, const torch::Tensor& xs,
                  const torch::Tensor& w, const torch::Tensor& scale,
                  int64_t bm, int64_t bn, int64_t wm, int64_t wn, bool glu,
                  int64_t w_pack, bool block_scaled) {
  TORCH_CHECK(xq.is_cuda() && xs.is_cuda() && w.is_cuda() && y.is_cuda() &&
                  scale.is_cuda(),
              name, ": tensors must be on the GPU");
  TORCH_CHECK(xq.dtype() == at::kFloat8_e4m3fn && xs.dtype() == torch::kUInt8,
              name, ": xq must be float8_e4m3fn and xs uint8");
  TORCH_CHECK(y.dtype() == torch::kBFloat16, name, ": y must be bf16");
  TORCH_CHECK(xq.dim() == 2 && xs.dim() == 2 && w.dim() == 2 &&
                  y.dim() == 2 && scale.dim() == (block_scaled ? 2 : 1),
              name,
              ": xq [M,K], xs [M,K/32], w [N,K], scale [N] or [N,K/32], "
              "y [M,N]");
  TORCH_CHECK(xq.is_contiguous() && xs.is_contiguous() && w.is_contiguous() &&
                  y.is_contiguous() && scale.is_contiguous(),
              name, ": tensors must be contiguous");
  const int64_t M = xq.size(0), K = xq.size(1), N = w.size(0);
  TORCH_CHECK(K >= mxg::KSTEP && K < (1 << 30) && K % mxg::KSTEP == 0, name,
              ": needs K % ", mxg::KSTEP, " == 0, got ", K);
  TORCH_CHECK(w.size(1) * w_pack == K && xs.size(0) == M &&
                  xs.size(1) * 32 == K && y.size(0) == M &&
                  y.size(1) == (glu ? N / 2 : N) && scale.size(0) == N &&
                  (!block_scaled || scale.size(1) * 32 == K),
              name, ": shape mismatch");
  TORCH_CHECK(M >= 1 && M < (1 << 24) && M * (K / 32) < (1ll << 31), name,
              ": needs 1 <= M < 2^24 and M K / 32 < 2^31, got M = ", M);
  TORCH_CHECK(N >= 16 && N % 16 == 0 && N < (1 << 27) &&
                  N * (K / 32) < (1ll << 31),
              name, ": needs N % 16 == 0 and N K / 32 < 2^31, got ", N);
  TORCH_CHECK(!glu || N % 32 == 0, name,
              ": the fused SwiGLU form needs N % 32 == 0, got ", N);
  TORCH_CHECK((uintptr_t)xq.data_ptr() % 16 == 0 &&
                  (uintptr_t)w.data_ptr() % 16 == 0 &&
                  (uintptr_t)xs.data_ptr() % 4 == 0 &&
                  (uintptr_t)scale.data_ptr() % 4 == 0,
              name, ": xq and w must be 16 B aligned, the scales 4 B");
  return {(const uint8_t*)xq.data_ptr(), (const uint8_t*)xs.data_ptr(),
          (const uint8_t*)w.data_ptr(), scale.data_ptr(),
          (short*)y.data_ptr(), (int)M, (int)N, (int)K, bm, bn, wm, wn, glu};
}

template <class F, int BM, int BN, int WM, int WN, int GLU>
void launch(const char* name, const MxArgs& a) {
  constexpr int lds = mxg::kLdsBytes<F, BM, BN>;
  auto* kern = mxg::mx_gemm_kernel<F, BM, BN, WM, WN, GLU>;
  if constexpr (lds > 65536) {
    static const hipError_t once = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)once;
  }
  const int mtiles = (a.M + BM - 1) / BM;
  constexpr int bno = GLU ? BN / 2 : BN;
  const int no = GLU ? a.N / 2 : a.N;
  const int ntiles = (no + bno - 1) / bno;
  const int64_t blocks = (int64_t)mtiles * ntiles;
  TORCH_CHECK(blocks < (1ll << 31), name, ": problem too large");
  kern<<<(unsigned)blocks, WM * WN * 64, lds,
         at::cuda::getCurrentHIPStream()>>>(a.xq, a.xs, a.w, a.scale, a.y,
                                            a.M, a.N, a.K, mtiles, ntiles);
}

template <class F>
void launch_format(const char* name, const MxArgs& a) {
#define MX_CASE(BM, BN, WM, WN)                                             \
  if (a.bm == BM && a.bn == BN && a.wm == WM && a.wn == WN)                 \
    return a.glu ? launch<F, BM, BN, WM, WN, 1>(name, a)                    \
                 : launch<F, BM, BN, WM, WN, 0>(name, a);
  MX_GEMM_CONFIGS(MX_CASE)
#undef MX_CASE
  TORCH_CHECK(false, name, ": no kernel for (BM, BN, WM, WN) = (", a.bm, ", ",
              a.bn, ", ", a.wm, ", ", a.wn, ")");
}

}  // namespace

// The launchers use the current stream and neither allocate nor synchronise,
// so they can run inside a captured graph.
void mxfp8_quantize_rows(torch::Tensor xq, torch::Tensor xs, torch::Tensor x) {
  const char* name = "mxfp8_quantize_rows";
  TORCH_CHECK(x.is_cuda() && xq.is_cuda() && xs.is_cuda(), name,
              ": tensors must be on the GPU");
  TORCH_CHECK(x.dtype() == torch::kBFloat16 &&
                  xq.dtype() == at::kFloat8_e4m3fn &&
                  xs.dtype() == torch::kUInt8,
              name, ": x must be bf16, xq float8_e4m3fn, xs uint8");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && xq.is_contiguous() &&
                  xs.is_contiguous(),
              name, ": x [M, K], contiguous tensors");
  const int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(M >= 1 && K >= 32 && K % 32 == 0, name,
              ": needs M >= 1 and K % 32 == 0, got [", M, ", ", K, "]");
  TORCH_CHECK(xq.dim() == 2 && xq.size(0) == M && xq.size(1) == K &&
                  xs.dim() == 2 && xs.size(0) == M && xs.size(1) * 32 == K,
              name, ": xq [M, K], xs [M, K / 32]");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
                  (uintptr_t)xq.data_ptr() % 8 == 0,
              name, ": x must be 16 B aligned, xq 8 B");
  const int64_t chunks = M * K / 8, blocks = (chunks + 255) / 256;
  TORCH_CHECK(blocks < (1ll << 31), name, ": problem too large");
  mxg::mxfp8_quantize_rows_kernel<<<(unsigned)blocks, 256, 0,
                                    at::cuda::getCurrentHIPStream()>>>(
      (const short*)x.data_ptr(), (uint8_t*)xq.data_ptr(),
      (uint8_t*)xs.data_ptr(), (size_t)chunks);
  HIP_CHECK_KERNEL();
}

void fp8_mx_gemm(torch::Tensor y, torch::Tensor xq, torch::Tensor xs,
                 torch::Tensor wq, torch::Tensor scale, int64_t bm, int64_t bn,
                 int64_t wm, int64_t wn, bool glu) {
  const char* name = "fp8_mx_gemm";
  TORCH_CHECK(wq.dtype() == at::kFloat8_e4m3fn, name,
              ": wq must be float8_e4m3fn");
  TORCH_CHECK(scale.dtype() == torch::kFloat32, name, ": scale must be fp32");
  launch_format<mxg::Fp8B>(name, check_args(name, y, xq, xs, wq, scale, bm,
                                            bn, wm, wn, glu, 1, false));
  HIP_CHECK_KERNEL();
}

void mxfp4_mx_gemm(torch::Tensor y, torch::Tensor xq, torch::Tensor xs,
                   torch::Tensor q, torch::Tensor scale, int64_t bm,
                   int64_t bn, int64_t wm, int64_t wn, bool glu) {
  const char* name = "mxfp4_mx_gemm";
  TORCH_CHECK(q.dtype() == torch::kUInt8 && scale.dtype() == torch::kUInt8,
              name, ": q and scale must be uint8");
  launch_format<mxg::Mxfp4B>(name, check_args(name, y, xq, xs, q, scale, bm,
                                              bn, wm, wn, glu, 2, true));
  HIP_CHECK_KERNEL();
}

std::map<std::string, std::vector<std::tuple<int, int, int, int>>>
mx_gemm_configs() {
#define MX_ENTRY(BM, BN, WM, WN) {BM, BN, WM, WN},
  const std::vector<std::tuple<int, int, int, int>> points = {
      MX_GEMM_CONFIGS(MX_ENTRY)};
#undef MX_ENTRY
  return {{"fp8", points}, {"mxfp4", points}};
}
