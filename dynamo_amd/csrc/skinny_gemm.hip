// Torch bindings for the skinny-M decode weight GEMM and the fp8 weight
// dequantisation (skinny_gemm_impl.h).
//   skinny_gemm:     y[M,N] = x[M,K] @ w[N,K]^T, bf16, 1 <= M <= 16.
//                    `coalesced` selects the row-coalesced format (u then
//                    counts 64-k steps, else 32-k ones).
//   fp8_skinny_gemm: y[M,N] = bf16((x[M,K] @ bf16(wq[N,K])^T) * scale[n]),
//                    x/y bf16, wq float8_e4m3fn, scale fp32, 1 <= M <= 64;
//                    u counts 128-k steps.
//   fp8_dequant:     out[N,K] = bf16(float(wq[N,K]) * scale[n]).
//   mxfp4_skinny_gemm: y[M,N] = x[M,K] @ W_eff[N,K]^T, x/y bf16, q uint8
//                    [N,K/2] (two e2m1 codes per byte, even k low), scale
//                    uint8 [N,K/32] (e8m0), 1 <= M <= 16 MXFP4_GEMM_MAX_MT;
//                    u counts 256-k steps.
//   mxfp4_dequant:   out[N,K] = bf16(W_eff[N,K]).
// `glu` selects the fused SwiGLU form of the three GEMMs: w is a gate/up
// weight [2I, K] (gate rows first), y is [M, I] = silu(gate) * up with the
// bits of silu_mul on the plain form's result. N % 32 == 0 and a table
// entry skinny::glu_capable lists only.
// `nontemporal` is the cache policy of the W loads. The launchers use the
// current stream and neither allocate nor synchronise, so they can run inside
// the captured decode graph.
#include "skinny_gemm_impl.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

struct GemmArgs {
  const short* x;
  const void* w;
  const void* scale;    // null for the bf16 formats
  short* y;
  int M, N, K;
  int64_t wpb, u, nt;
  bool nontemporal;
  bool glu;
};

// Everything the GEMM entry points require of their arguments but the W and
// scale dtypes; max_m, min_k and k_per_step are the format's limits. w is
// [N, K / w_pack]; scale is [N], or [N, K / 32] if block_scaled. y is [M, N],
// or [M, N / 2] if glu.
GemmArgs check_args(const char* name, int64_t max_m, int64_t min_k,
                    int64_t k_per_step, const torch::Tensor& y,
                    const torch::Tensor& x, const torch::Tensor& w,
                    const torch::Tensor* scale, int64_t wpb, int64_t u,
                    int64_t nt, bool nontemporal, bool glu,
                    int64_t w_pack = 1, bool block_scaled = false) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && y.is_cuda() &&
                  (!scale || scale->is_cuda()),
              name, ": tensors must be on the GPU");
  TORCH_CHECK(x.dtype() == torch::kBFloat16 && y.dtype() == torch::kBFloat16,
              name, ": x and y must be bf16");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && y.dim() == 2 &&
                  (!scale || scale->dim() == (block_scaled ? 2 : 1)),
              name, ": x [M,K], w [N,K], scale [N], y [M,N]");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && y.is_contiguous() &&
                  (!scale || scale->is_contiguous()),
              name, ": tensors must be contiguous");
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) * w_pack == K && y.size(0) == M &&
                  y.size(1) == (glu ? N / 2 : N) &&
                  (!scale || scale->size(0) == N) &&
                  (!block_scaled || scale->size(1) * 32 == K),
              name, ": shape mismatch");
  TORCH_CHECK(M >= 1 && M <= max_m, name, ": needs 1 <= M <= ", max_m,
              ", got ", M);
  TORCH_CHECK(N >= 16 && N % 16 == 0, name, ": needs N % 16 == 0, got ", N);
  TORCH_CHECK(N < (1 << 27), name, ": N too large");
  TORCH_CHECK(!glu || (N % 32 == 0 && nt % 2 == 0), name,
              ": the fused SwiGLU form needs N % 32 == 0 and an even NT, got "
              "N = ", N, ", NT = ", nt);
  TORCH_CHECK(wpb > 0 && u > 0 && nt > 0, name, ": bad configuration");
  const int64_t kstep = wpb * k_per_step * u;
  TORCH_CHECK(K >= min_k && K < (1 << 30) && K % kstep == 0, name,
              ": needs K >= ", min_k, " and K % ", kstep, " == 0, got ", K);
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
                  (uintptr_t)w.data_ptr() % 16 == 0,
              name, ": x and w must be 16 B aligned");
  TORCH_CHECK(!block_scaled || (uintptr_t)scale->data_ptr() % 8 == 0, name,
              ": scale must be 8 B aligned");
  return {(const short*)x.data_ptr(), w.data_ptr(),
          scale ? scale->data_ptr() : nullptr,
          (short*)y.data_ptr(), (int)M, (int)N, (int)K, wpb, u, nt,
          nontemporal, glu};
}

// Launches <F, WPB, U, NT> at ceil(M / 16) accumulator tiles, MT at the most.
// A GLU block owns NT / 2 of the N / 2 output column tiles: the same grid.
template <class F, int WPB, int U, int NT, int MT, int GLU>
void launch(const GemmArgs& a) {
  if constexpr (MT > 1) {
    if (a.M <= (MT - 1) * 16) return launch<F, WPB, U, NT, MT - 1, GLU>(a);
  }
  const int grid = (a.N + NT * 16 - 1) / (NT * 16);
  auto stream = at::cuda::getCurrentHIPStream();
  auto w = (const typename F::welem*)a.w;
  auto scale = (const typename F::scale_t*)a.scale;
  if (a.nontemporal)
    skinny::skinny_gemm_kernel<F, WPB, U, NT, MT, 1, GLU>
        <<<grid, WPB * 64, 0, stream>>>(a.x, w, scale, a.y, a.M, a.N, a.K);
  else
    skinny::skinny_gemm_kernel<F, WPB, U, NT, MT, 0, GLU>
        <<<grid, WPB * 64, 0, stream>>>(a.x, w, scale, a.y, a.M, a.N, a.K);
}

// The plain form, or the GLU one where the table entry has one.
template <class F, int WPB, int U, int NT, int MT>
void launch_form(const char* name, const GemmArgs& a) {
  if (!a.glu) return launch<F, WPB, U, NT, MT, 0>(a);
  if constexpr (skinny::glu_capable<F>(WPB, U, NT))
    return launch<F, WPB, U, NT, MT, 1>(a);
  TORCH_CHECK(false, name, ": no fused SwiGLU kernel for (WPB, U, NT) = (",
              WPB, ", ", U, ", ", NT, ") of this format");
}

typedef std::vector<std::tuple<int, int, int>> ConfigList;

// NAME(a) launches a's (wpb, u, nt) if TABLE lists it, else raises;
// NAME_configs() is TABLE as a list.
#define GEMM_CASE(WPB, U, NT)                                                \
  if (a.wpb == WPB && a.u == U && a.nt == NT)                                \
    return launch_form<Format, WPB, U, NT, kMaxMt>(name, a);
#define GEMM_ENTRY(WPB, U, NT) {WPB, U, NT},
#define GEMM_GLU_ENTRY(WPB, U, NT)                                           \
  if (skinny::glu_capable<Format>(WPB, U, NT)) l.push_back({WPB, U, NT});
#define GEMM_DISPATCH(NAME, F, MAX_MT, TABLE)                                \
  void NAME(const char* name, const GemmArgs& a) {                           \
    using Format = F;                                                        \
    constexpr int kMaxMt = MAX_MT;                                           \
    TABLE(GEMM_CASE)                                                         \
    TORCH_CHECK(false, name, ": no kernel for (WPB, U, NT) = (", a.wpb,      \
                ", ", a.u, ", ", a.nt, ")");                                 \
  }                                                                          \
  ConfigList NAME##_configs() { return {TABLE(GEMM_ENTRY)}; }              \
  ConfigList NAME##_glu_configs() {                                          \
    using Format = F;                                                        \
    ConfigList l;                                                            \
    TABLE(GEMM_GLU_ENTRY)                                                    \
    return l;                                                                \
  }
GEMM_DISPATCH(launch_plain, skinny::Bf16Plain, 1, SKINNY_GEMM_CONFIGS)
GEMM_DISPATCH(launch_coal, skinny::Bf16Coal, 1, SKINNY_GEMM_COAL_CONFIGS)
GEMM_DISPATCH(launch_fp8, skinny::Fp8Coal, 4, FP8_GEMM_CONFIGS)
GEMM_DISPATCH(launch_mxfp4, skinny::Mxfp4Coal, MXFP4_GEMM_MAX_MT,
              MXFP4_GEMM_CONFIGS)
#undef GEMM_DISPATCH
#undef GEMM_GLU_ENTRY
#undef GEMM_ENTRY
#undef GEMM_CASE

}  // namespace

void skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor w,
                 int64_t wpb, int64_t u, int64_t nt, bool nontemporal,
                 bool coalesced, bool glu) {
  const char* name = "skinny_gemm";
  TORCH_CHECK(w.dtype() == torch::kBFloat16, name, ": w must be bf16");
  const GemmArgs a = check_args(
      name, 16, 2048,
      coalesced ? skinny::Bf16Coal::KSTEP : skinny::Bf16Plain::KSTEP, y, x, w,
      nullptr, wpb, u, nt, nontemporal, glu);
  if (coalesced) launch_coal(name, a);
  else launch_plain(name, a);
  HIP_CHECK_KERNEL();
}

void fp8_skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor wq,
                     torch::Tensor scale, int64_t wpb, int64_t u, int64_t nt,
                     bool nontemporal, bool glu) {
  const char* name = "fp8_skinny_gemm";
  TORCH_CHECK(wq.dtype() == at::kFloat8_e4m3fn, name,
              ": wq must be float8_e4m3fn");
  TORCH_CHECK(scale.dtype() == torch::kFloat32, name, ": scale must be fp32");
  launch_fp8(name, check_args(name, 64, 128, skinny::Fp8Coal::KSTEP, y, x, wq,
                              &scale, wpb, u, nt, nontemporal, glu));
  HIP_CHECK_KERNEL();
}

void mxfp4_skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor q,
                       torch::Tensor scale, int64_t wpb, int64_t u,
                       int64_t nt, bool nontemporal, bool glu) {
  const char* name = "mxfp4_skinny_gemm";
  TORCH_CHECK(q.dtype() == torch::kUInt8 && scale.dtype() == torch::kUInt8,
              name, ": q and scale must be uint8");
  launch_mxfp4(name, check_args(name, 16 * MXFP4_GEMM_MAX_MT, 256,
                                skinny::Mxfp4Coal::KSTEP, y, x, q, &scale,
                                wpb, u, nt, nontemporal, glu,
                                skinny::Mxfp4Coal::WPACK, true));
  HIP_CHECK_KERNEL();
}

// The (WPB, U, NT) tables of the formats, for the Python side to check its
// own copies against.
std::map<std::string, ConfigList> skinny_gemm_configs() {
  return {{"bf16_plain", launch_plain_configs()},
          {"bf16_coalesced", launch_coal_configs()},
          {"fp8", launch_fp8_configs()},
          {"mxfp4", launch_mxfp4_configs()}};
}

// The entries of those tables that have a fused SwiGLU form.
std::map<std::string, ConfigList> skinny_gemm_glu_configs() {
  return {{"bf16_plain", launch_plain_glu_configs()},
          {"bf16_coalesced", launch_coal_glu_configs()},
          {"fp8", launch_fp8_glu_configs()},
          {"mxfp4", launch_mxfp4_glu_configs()}};
}

int64_t mxfp4_gemm_max_m() { return 16 * MXFP4_GEMM_MAX_MT; }

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
  skinny::fp8_dequant_kernel<<<(unsigned)blocks, 256, 0, stream>>>(
      (short*)out.data_ptr(), (const unsigned char*)wq.data_ptr(),
      (const float*)scale.data_ptr(), (long long)N, (long long)K);
  HIP_CHECK_KERNEL();
}

void mxfp4_dequant(torch::Tensor out, torch::Tensor q, torch::Tensor scale) {
  TORCH_CHECK(out.is_cuda() && q.is_cuda() && scale.is_cuda(),
              "mxfp4_dequant: tensors must be on the GPU");
  TORCH_CHECK(out.dtype() == torch::kBFloat16 && q.dtype() == torch::kUInt8 &&
                  scale.dtype() == torch::kUInt8,
              "mxfp4_dequant: out bf16, q uint8, scale uint8");
  TORCH_CHECK(out.dim() == 2 && q.dim() == 2 && scale.dim() == 2,
              "mxfp4_dequant: out [N,K], q [N,K/2], scale [N,K/32]");
  TORCH_CHECK(out.is_contiguous() && q.is_contiguous() &&
                  scale.is_contiguous(),
              "mxfp4_dequant: tensors must be contiguous");
  const int64_t N = out.size(0), K = out.size(1);
  TORCH_CHECK(N >= 1 && K >= 32 && K % 32 == 0,
              "mxfp4_dequant: needs K % 32 == 0, got ", K);
  TORCH_CHECK(q.size(0) == N && q.size(1) * 2 == K && scale.size(0) == N &&
                  scale.size(1) * 32 == K,
              "mxfp4_dequant: shape mismatch");
  TORCH_CHECK((uintptr_t)out.data_ptr() % 16 == 0 &&
                  (uintptr_t)q.data_ptr() % 16 == 0,
              "mxfp4_dequant: out and q must be 16 B aligned");
  const int64_t threads = N * (K / 32);
  const int64_t blocks = (threads + 255) / 256;
  TORCH_CHECK(blocks < (1ll << 31), "mxfp4_dequant: matrix too large");
  auto stream = at::cuda::getCurrentHIPStream();
  skinny::mxfp4_dequant_kernel<<<(unsigned)blocks, 256, 0, stream>>>(
      (short*)out.data_ptr(), (const unsigned char*)q.data_ptr(),
      (const unsigned char*)scale.data_ptr(), (long long)threads);
  HIP_CHECK_KERNEL();
}
