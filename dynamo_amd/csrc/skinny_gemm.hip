// Torch binding for the skinny-M decode weight GEMM (skinny_gemm_impl.h):
// y[M,N] = x[M,K] @ W[N,K]^T, bf16, 1 <= M <= 16. `coalesced` selects the
// row-coalesced kernel (u then counts 64-k double steps), `nontemporal` the
// cache policy of the W loads.
// The launcher uses the current stream and neither allocates nor
// synchronises, so it can run inside the captured decode graph.
#include "skinny_gemm_impl.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

void skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor w,
                 int64_t wpb, int64_t u, int64_t nt, bool nontemporal,
                 bool coalesced) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && y.is_cuda(),
              "skinny_gemm: tensors must be on the GPU");
  TORCH_CHECK(x.dtype() == torch::kBFloat16 && w.dtype() == torch::kBFloat16 &&
                  y.dtype() == torch::kBFloat16,
              "skinny_gemm: bf16 only");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && y.dim() == 2,
              "skinny_gemm: x [M,K], w [N,K], y [M,N]");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && y.is_contiguous(),
              "skinny_gemm: x, w and y must be contiguous");
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && y.size(0) == M && y.size(1) == N,
              "skinny_gemm: shape mismatch");
  TORCH_CHECK(M >= 1 && M <= 16, "skinny_gemm: needs 1 <= M <= 16, got ", M);
  TORCH_CHECK(N >= 16 && N % 16 == 0, "skinny_gemm: needs N % 16 == 0, got ", N);
  TORCH_CHECK(N < (1 << 27), "skinny_gemm: N too large");
  TORCH_CHECK(wpb > 0 && u > 0 && nt > 0, "skinny_gemm: bad configuration");
  const int64_t kstep = wpb * (coalesced ? 64 : 32) * u;
  TORCH_CHECK(K >= 2048 && K < (1 << 30) && K % kstep == 0,
              "skinny_gemm: needs K >= 2048 and K % ", kstep, " == 0, got ", K);
  auto stream = at::cuda::getCurrentHIPStream();
  const short* xp = (const short*)x.data_ptr();
  const short* wp = (const short*)w.data_ptr();
  short* yp = (short*)y.data_ptr();
  const int grid = (int)((N + nt * 16 - 1) / (nt * 16));

  bool launched = false;
#define SKINNY_CASE(WPB, U, NT)                                              \
  if (!launched && wpb == WPB && u == U && nt == NT) {                       \
    if (nontemporal)                                                         \
      skinny::skinny_gemm_kernel<WPB, U, NT, 1>                              \
          <<<grid, WPB * 64, 0, stream>>>(xp, wp, yp, (int)M, (int)N, (int)K); \
    else                                                                     \
      skinny::skinny_gemm_kernel<WPB, U, NT, 0>                              \
          <<<grid, WPB * 64, 0, stream>>>(xp, wp, yp, (int)M, (int)N, (int)K); \
    launched = true;                                                         \
  }
#define SKINNY_COAL_CASE(WPB, U2, NT)                                        \
  if (!launched && wpb == WPB && u == U2 && nt == NT) {                      \
    if (nontemporal)                                                         \
      skinny::skinny_gemm_coal_kernel<WPB, U2, NT, 1>                        \
          <<<grid, WPB * 64, 0, stream>>>(xp, wp, yp, (int)M, (int)N, (int)K); \
    else                                                                     \
      skinny::skinny_gemm_coal_kernel<WPB, U2, NT, 0>                        \
          <<<grid, WPB * 64, 0, stream>>>(xp, wp, yp, (int)M, (int)N, (int)K); \
    launched = true;                                                         \
  }
  if (coalesced) {
    SKINNY_GEMM_COAL_CONFIGS(SKINNY_COAL_CASE)
  } else {
    SKINNY_GEMM_CONFIGS(SKINNY_CASE)
  }
#undef SKINNY_COAL_CASE
#undef SKINNY_CASE
  TORCH_CHECK(launched, "skinny_gemm: no kernel for (WPB, U, NT) = (", wpb,
              ", ", u, ", ", nt, ")");
  HIP_CHECK_KERNEL();
}
