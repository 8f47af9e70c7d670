// RMSNorm kernels (bf16 in/out, fp32 accumulation), MI355X-native.
//
// Memory-bound: target HBM ceiling. Loads are vectorized short8 (16 B/lane)
// per guide Guideline 13. One workgroup per token row, grid-stride over rows.
//
// Capability parity: the reference (ai-dynamo/dynamo) delegates RMSNorm to its
// external engines; this is the native CDNA4 implementation for our workers.
#include "common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

constexpr int kBlock = 256;

// out[row] = x[row] / rms(x[row]) * w ; optionally first x = x + res (and the
// summed value is written back to res for the next residual hop).
template <bool FUSED_ADD>
__global__ void rmsnorm_kernel(short* __restrict__ out,        // [rows, D]
                               short* __restrict__ x,          // [rows, D]
                               short* __restrict__ res,        // [rows, D] or null
                               const short* __restrict__ w,    // [D]
                               float eps, int rows, int D) {
  __shared__ float lds[kBlock / WAVE_SIZE];
  const int nvec = D / 8;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    short* xrow = x + (int64_t)row * D;
    short* rrow = FUSED_ADD ? res + (int64_t)row * D : nullptr;
    short* orow = out + (int64_t)row * D;

    float ss = 0.f;
    for (int v = threadIdx.x; v < nvec; v += kBlock) {
      short8 xv = *reinterpret_cast<const short8*>(xrow + v * 8);
      if constexpr (FUSED_ADD) {
        short8 rv = *reinterpret_cast<const short8*>(rrow + v * 8);
        short8 sv;
#pragma unroll
        for (int i = 0; i < 8; i++) {
          float s = bf16_to_f32(xv[i]) + bf16_to_f32(rv[i]);
          sv[i] = f32_to_bf16(s);
          ss += s * s;
        }
        // write the summed residual back (residual stream stays bf16)
        *reinterpret_cast<short8*>(rrow + v * 8) = sv;
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          float xf = bf16_to_f32(xv[i]);
          ss += xf * xf;
        }
      }
    }
    ss = block_reduce_sum(ss, lds);
    const float inv = rsqrtf(ss / (float)D + eps);

    for (int v = threadIdx.x; v < nvec; v += kBlock) {
      // re-read the (possibly summed) row; bf16 round-trip is intentional:
      // the residual stream is bf16, so normalizing the stored value keeps
      // norm(x) consistent with what the next layer's residual add sees.
      const short* src = FUSED_ADD ? rrow : xrow;
      short8 sv = *reinterpret_cast<const short8*>(src + v * 8);
      short8 wv = *reinterpret_cast<const short8*>(w + v * 8);
      short8 ov;
#pragma unroll
      for (int i = 0; i < 8; i++)
        ov[i] = f32_to_bf16(bf16_to_f32(sv[i]) * inv * bf16_to_f32(wv[i]));
      *reinterpret_cast<short8*>(orow + v * 8) = ov;
    }
    __syncthreads();  // lds reuse across grid-stride iterations
  }
}

// Register-resident single pass for D = 8 * kBlock * VPT (VPT <= 4): every
// x / res / w vector of the thread is loaded before the first use, and the
// summed bf16 row stays in registers for the scale pass, so the row costs
// one memory round trip instead of VPT dependent ones plus a global
// re-read. Element ownership (thread t owns vectors t, t+kBlock, ...), the
// accumulation order of ss and the block reduction are those of
// rmsnorm_kernel, so the output is bit-identical to it.
template <bool FUSED_ADD, int VPT>
__global__ __launch_bounds__(kBlock) void rmsnorm_reg_kernel(
    short* __restrict__ out,        // [rows, D]
    short* __restrict__ x,          // [rows, D]
    short* __restrict__ res,        // [rows, D] or null
    const short* __restrict__ w,    // [D]
    float eps, int rows) {
  __shared__ float lds[kBlock / WAVE_SIZE];
  constexpr int D = 8 * kBlock * VPT;
  short8 wv[VPT];
#pragma unroll
  for (int j = 0; j < VPT; j++)
    wv[j] = *reinterpret_cast<const short8*>(w + (threadIdx.x + j * kBlock) * 8);
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    short* xrow = x + (int64_t)row * D;
    short* rrow = FUSED_ADD ? res + (int64_t)row * D : nullptr;
    short* orow = out + (int64_t)row * D;

    short8 sv[VPT], rv[VPT];
#pragma unroll
    for (int j = 0; j < VPT; j++) {
      const int v = threadIdx.x + j * kBlock;
      sv[j] = *reinterpret_cast<const short8*>(xrow + v * 8);
      if constexpr (FUSED_ADD)
        rv[j] = *reinterpret_cast<const short8*>(rrow + v * 8);
    }
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; j++) {
      if constexpr (FUSED_ADD) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          float s = bf16_to_f32(sv[j][i]) + bf16_to_f32(rv[j][i]);
          sv[j][i] = f32_to_bf16(s);
          ss += s * s;
        }
        *reinterpret_cast<short8*>(rrow + (threadIdx.x + j * kBlock) * 8) = sv[j];
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          float xf = bf16_to_f32(sv[j][i]);
          ss += xf * xf;
        }
      }
    }
    ss = block_reduce_sum(ss, lds);
    const float inv = rsqrtf(ss / (float)D + eps);

#pragma unroll
    for (int j = 0; j < VPT; j++) {
      short8 ov;
#pragma unroll
      for (int i = 0; i < 8; i++)
        ov[i] = f32_to_bf16(bf16_to_f32(sv[j][i]) * inv * bf16_to_f32(wv[j][i]));
      *reinterpret_cast<short8*>(orow + (threadIdx.x + j * kBlock) * 8) = ov;
    }
    __syncthreads();  // lds reuse across grid-stride iterations
  }
}

template <bool FUSED_ADD>
void launch_rmsnorm(short* out, short* x, short* res, const short* w,
                    float eps, int rows, int D, bool allow_fast,
                    hipStream_t stream) {
  const int grid = std::min<int>(rows, 2048);
  const int nvec = D / 8;
  const int vpt = (allow_fast && nvec % kBlock == 0) ? nvec / kBlock : 0;
  switch (vpt) {
    case 1:
      rmsnorm_reg_kernel<FUSED_ADD, 1><<<grid, kBlock, 0, stream>>>(
          out, x, res, w, eps, rows);
      break;
    case 2:
      rmsnorm_reg_kernel<FUSED_ADD, 2><<<grid, kBlock, 0, stream>>>(
          out, x, res, w, eps, rows);
      break;
    case 4:
      rmsnorm_reg_kernel<FUSED_ADD, 4><<<grid, kBlock, 0, stream>>>(
          out, x, res, w, eps, rows);
      break;
    default:
      rmsnorm_kernel<FUSED_ADD><<<grid, kBlock, 0, stream>>>(
          out, x, res, w, eps, rows, D);
  }
}

}  // namespace

void rmsnorm(torch::Tensor out, torch::Tensor input, torch::Tensor weight,
             double eps, bool allow_fast) {
  TORCH_CHECK(input.is_cuda() && input.dtype() == torch::kBFloat16);
  TORCH_CHECK(input.is_contiguous() && out.is_contiguous());
  const int D = input.size(-1);
  const int rows = input.numel() / D;
  TORCH_CHECK(D % 8 == 0, "hidden size must be a multiple of 8");
  if (rows == 0) return;
  auto stream = at::cuda::getCurrentHIPStream();
  launch_rmsnorm<false>((short*)out.data_ptr(), (short*)input.data_ptr(),
                        nullptr, (const short*)weight.data_ptr(), (float)eps,
                        rows, D, allow_fast, stream);
  HIP_CHECK_KERNEL();
}

void fused_add_rmsnorm(torch::Tensor input, torch::Tensor residual,
                       torch::Tensor weight, double eps, bool allow_fast) {
  TORCH_CHECK(input.is_cuda() && input.dtype() == torch::kBFloat16);
  TORCH_CHECK(input.is_contiguous() && residual.is_contiguous());
  const int D = input.size(-1);
  const int rows = input.numel() / D;
  TORCH_CHECK(D % 8 == 0);
  if (rows == 0) return;
  auto stream = at::cuda::getCurrentHIPStream();
  launch_rmsnorm<true>((short*)input.data_ptr(), (short*)input.data_ptr(),
                       (short*)residual.data_ptr(),
                       (const short*)weight.data_ptr(), (float)eps, rows, D,
                       allow_fast, stream);
  HIP_CHECK_KERNEL();
}
