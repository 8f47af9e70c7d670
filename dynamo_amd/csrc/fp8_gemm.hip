// Torch bindings for the W8A16 decode weight GEMM and the fp8 weight
// dequantisation (fp8_gemm_impl.h).
//   fp8_skinny_gemm: y[M,N] = bf16((x[M,K] @ bf16(wq[N,K])^T) * scale[n]),
//                    x/y bf16, wq float8_e4m3fn, scale fp32, 1 <= M <= 64.
//   fp8_dequant:     out[N,K] = bf16(float(wq[N,K]) * scale[n]).
// Both launchers use the current stream and neither allocate nor
// synchronise, so they can run inside the captured decode graph.
#include "fp8_gemm_impl.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

void fp8_skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor wq,
                     torch::Tensor scale, int64_t wpb, int64_t u, int64_t nt,
                     bool nontemporal) {
  TORCH_CHECK(x.is_cuda() && wq.is_cuda() && y.is_cuda() && scale.is_cuda(),
              "fp8_skinny_gemm: tensors must be on the GPU");
  TORCH_CHECK(x.dtype() == torch::kBFloat16 && y.dtype() == torch::kBFloat16,
              "fp8_skinny_gemm: x and y must be bf16");
  TORCH_CHECK(wq.dtype() == at::kFloat8_e4m3fn,
              "fp8_skinny_gemm: wq must be float8_e4m3fn");
  TORCH_CHECK(scale.dtype() == torch::kFloat32,
              "fp8_skinny_gemm: scale must be fp32");
  TORCH_CHECK(x.dim() == 2 && wq.dim() == 2 && y.dim() == 2 && scale.dim() == 1,
              "fp8_skinny_gemm: x [M,K], wq [N,K], scale [N], y [M,N]");
  TORCH_CHECK(x.is_contiguous() && wq.is_contiguous() && y.is_contiguous() &&
                  scale.is_contiguous(),
              "fp8_skinny_gemm: tensors must be contiguous");
  const int64_t M = x.size(0), K = x.size(1), N = wq.size(0);
  TORCH_CHECK(wq.size(1) == K && y.size(0) == M && y.size(1) == N &&
                  scale.size(0) == N,
              "fp8_skinny_gemm: shape mismatch");
  TORCH_CHECK(M >= 1 && M <= 64, "fp8_skinny_gemm: needs 1 <= M <= 64, got ", M);
  TORCH_CHECK(N >= 16 && N % 16 == 0,
              "fp8_skinny_gemm: needs N % 16 == 0, got ", N);
  TORCH_CHECK(N < (1 << 27), "fp8_skinny_gemm: N too large");
  TORCH_CHECK(wpb > 0 && u > 0 && nt > 0, "fp8_skinny_gemm: bad configuration");
  const int64_t kstep = wpb * 128 * u;
  TORCH_CHECK(K >= 128 && K < (1 << 30) && K % kstep == 0,
              "fp8_skinny_gemm: needs K >= 128 and K % ", kstep, " == 0, got ",
              K);
  auto stream = at::cuda::getCurrentHIPStream();
  const short* xp = (const short*)x.data_ptr();
  const unsigned char* wp = (const unsigned char*)wq.data_ptr();
  const float* sp = (const float*)scale.data_ptr();
  short* yp = (short*)y.data_ptr();
  TORCH_CHECK((uintptr_t)xp % 16 == 0 && (uintptr_t)wp % 16 == 0,
              "fp8_skinny_gemm: x and wq must be 16 B aligned");
  const int grid = (int)((N + nt * 16 - 1) / (nt * 16));
  const int mt = (int)((M + 15) / 16);

  bool launched = false;
#define FP8_LAUNCH(WPB, U, NT, MT, NTL)                                      \
  fp8gemm::fp8_skinny_gemm_kernel<WPB, U, NT, MT, NTL>                       \
      <<<grid, WPB * 64, 0, stream>>>(xp, wp, sp, yp, (int)M, (int)N, (int)K)
#define FP8_MT(WPB, U, NT, MT)                                               \
  if (mt == MT) {                                                            \
    if (nontemporal) FP8_LAUNCH(WPB, U, NT, MT, 1);                          \
    else FP8_LAUNCH(WPB, U, NT, MT, 0);                                      \
  }
#define FP8_CASE(WPB, U, NT)                                                 \
  if (!launched && wpb == WPB && u == U && nt == NT) {                       \
    FP8_MT(WPB, U, NT, 1) FP8_MT(WPB, U, NT, 2)                              \
    FP8_MT(WPB, U, NT, 3) FP8_MT(WPB, U, NT, 4)                              \
    launched = true;                                                         \
  }
  FP8_GEMM_CONFIGS(FP8_CASE)
#undef FP8_CASE
#undef FP8_MT
#undef FP8_LAUNCH
  TORCH_CHECK(launched, "fp8_skinny_gemm: no kernel for (WPB, U, NT) = (", wpb,
              ", ", u, ", ", nt, ")");
  HIP_CHECK_KERNEL();
}

void fp8_dequant(torch::Tensor out, torch::Tensor wq, torch::Tensor scale) {
  TORCH_CHECK(out.is_cuda() && wq.is_cuda() && scale.is_cuda(),
              "fp8_dequant: tensors must be on the GPU");
  TORCH_CHECK(out.dtype() == torch::kBFloat16 &&
                  wq.dtype() == at::kFloat8_e4m3fn &&
                  scale.dtype() == torch::kFloat32,
              "fp8_dequant: out bf16, wq float8_e4m3fn, scale fp32");
  TORCH_CHECK(out.dim() == 2 && wq.dim() == 2 && scale.dim() == 1,
              "fp8_dequant: out [N,K], wq [N,K], scale [N]");
  TORCH_CHECK(out.is_contiguous() && wq.is_contiguous() &&
                  scale.is_contiguous(),
              "fp8_dequant: tensors must be contiguous");
  const int64_t N = wq.size(0), K = wq.size(1);
  TORCH_CHECK(out.size(0) == N && out.size(1) == K && scale.size(0) == N,
              "fp8_dequant: shape mismatch");
  TORCH_CHECK(N >= 1 && K >= 16 && K % 16 == 0,
              "fp8_dequant: needs K % 16 == 0, got ", K);
  TORCH_CHECK((uintptr_t)out.data_ptr() % 16 == 0 &&
                  (uintptr_t)wq.data_ptr() % 16 == 0,
              "fp8_dequant: out and wq must be 16 B aligned");
  const int64_t threads = N * (K / 16);
  const int64_t blocks = (threads + 255) / 256;
  TORCH_CHECK(blocks < (1ll << 31), "fp8_dequant: matrix too large");
  auto stream = at::cuda::getCurrentHIPStream();
  fp8gemm::fp8_dequant_kernel<<<(unsigned)blocks, 256, 0, stream>>>(
      (short*)out.data_ptr(), (const unsigned char*)wq.data_ptr(),
      (const float*)scale.data_ptr(), (long long)N, (long long)K);
  HIP_CHECK_KERNEL();
}
