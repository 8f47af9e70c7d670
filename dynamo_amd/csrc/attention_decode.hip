// Torch bindings + production template choices for paged-attention decode.
// Kernel implementation: attention_decode_impl.h (shared with the
// standalone sweep tool benchmarks/decode_sweep.hip, which picked these
// (DP, HS, DEPTH) combos on MI355X hardware).
#include "attention_decode_impl.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

using namespace decode_attn;

// DYNAMO_DECODE_NT default, decided by the in-situ phase-1 trace row:
// nt K/V loads measured 105 -> 123 us per layer (profiles/README.md)
static constexpr bool kDecodeNtDefault = false;

int64_t paged_decode_num_chunks(int64_t max_ctx) {
  const int chunk = decode_chunk_tokens((int)max_ctx);
  return std::max<int64_t>(1, (max_ctx + chunk - 1) / chunk);
}

int64_t decode_chunk_tokens_py(int64_t max_ctx) {
  return decode_chunk_tokens((int)max_ctx);
}

void paged_attention_decode(torch::Tensor out, torch::Tensor q,
                            torch::Tensor kcache, torch::Tensor vcache,
                            torch::Tensor page_table, torch::Tensor ctx_lens,
                            torch::Tensor partial, torch::Tensor ml,
                            double scale, int64_t chunk_tokens,
                            bool v_transposed, int64_t nt_policy) {
  TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kBFloat16);
  TORCH_CHECK(page_table.dtype() == torch::kInt32 && ctx_lens.dtype() == torch::kInt32);
  const bool fp8 = kcache.dtype() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || kcache.dtype() == torch::kBFloat16,
              "kv cache must be bf16 or float8_e4m3fn");
  const int B = q.size(0);
  const int Hq = q.size(1);
  const int hd = q.size(2);
  const int Hkv = kcache.size(1);
  const int ps = kcache.size(2);
  const int G = Hq / Hkv;
  const int max_pages = page_table.size(1);
  const int C = ml.size(2);  // chunk capacity allocated by caller
  TORCH_CHECK(hd == 128, "only head_dim=128 supported natively");
  TORCH_CHECK((ps & (ps - 1)) == 0, "page_size must be a power of 2");
  int log2_ps = 0; while ((1 << log2_ps) < ps) log2_ps++;
  if (B == 0) return;
  const int chunk = (int)chunk_tokens;
  TORCH_CHECK(chunk >= 128 && chunk % 128 == 0, "bad chunk_tokens ", chunk);
  auto stream = at::cuda::getCurrentHIPStream();
  dim3 grid(B, Hkv, C);

  // Phase 1. `group` is empty for the VALU kernel (G is a template
  // parameter there) and the runtime G for the MFMA kernels.
  auto launch = [&](auto* kern, int lds, auto... group) {
    if (lds > 65536)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds);
    kern<<<grid, kBlock, lds, stream>>>(
        partial.data_ptr<float>(), ml.data_ptr<float>(),
        (short*)out.data_ptr(), (const short*)q.data_ptr(),
        (const short*)kcache.data_ptr(), (const short*)vcache.data_ptr(),
        page_table.data_ptr<int32_t>(), ctx_lens.data_ptr<int32_t>(),
        (float)scale, chunk, group..., B, Hkv, C, max_pages, log2_ps, hd);
  };
  const int swapped_lds = mfma_swapped_lds_bytes(G, hd);

  if (v_transposed) {
    // d-major V pages: one consumer, every GQA group 2..16
    TORCH_CHECK(vcache.size(2) == hd && vcache.size(3) == ps,
                "v_transposed expects vcache [P, Hkv, hd, ps]");
    TORCH_CHECK(ps % 32 == 0 && hd == 128 && G >= 2 && G <= 16,
                "v_transposed decode needs page_size%32==0, head_dim==128, "
                "2<=G<=16 (got G=", G, ")");
    // non-temporal K/V loads: DYNAMO_DECODE_NT, overridable per call
    // (nt_policy 0/1) so a test can compare both variants in one process.
    // Outputs are bit-identical.
    static const bool nt_env = [] {
      const char* e = getenv("DYNAMO_DECODE_NT");
      return e == nullptr ? kDecodeNtDefault : e[0] != '0';
    }();
    const bool use_nt = nt_policy < 0 ? nt_env : nt_policy != 0;
    if (fp8 && use_nt)
      launch(&paged_decode_mfma_swapped_dmajor<1, 1>, swapped_lds, G);
    else if (fp8)
      launch(&paged_decode_mfma_swapped_dmajor<1, 0>, swapped_lds, G);
    else if (use_nt)
      launch(&paged_decode_mfma_swapped_dmajor<0, 1>, swapped_lds, G);
    else
      launch(&paged_decode_mfma_swapped_dmajor<0, 0>, swapped_lds, G);
  } else if (fp8) {
    // fp8 KV: the runtime-G swapped kernel is the ONLY fp8 consumer
    TORCH_CHECK(ps % 32 == 0 && hd == 128 && G <= 16,
                "fp8 KV cache needs page_size%32==0, head_dim==128, G<=16");
    launch(&paged_decode_mfma_swapped<1>, swapped_lds, G);
  } else {
    static const bool use_mfma = [] {
      const char* e = getenv("DYNAMO_DECODE_MFMA");
      return e == nullptr || e[0] != '0';  // default ON (sweep-verified)
    }();
    // swapped-operand variant (tokens on MFMA M, in-register P exchange via
    // permlane swaps): sweep-verified bit-match + faster at every measured
    // (G, chunk); DYNAMO_DECODE_SWAPPED=0 falls back to the A-variant
    static const bool use_swapped = [] {
      const char* e = getenv("DYNAMO_DECODE_SWAPPED");
      return e == nullptr || e[0] != '0';
    }();
    auto launch_mfma = [&] {
      if (use_swapped)
        launch(&paged_decode_mfma_swapped<0>, swapped_lds, G);
      else
        launch(&paged_decode_mfma, mfma_lds_bytes(G, hd), G);
    };
    const bool mfma_ok = use_mfma && ps % 32 == 0 && hd == 128;
    switch (G) {  // combos picked by benchmarks/decode_sweep on MI355X
      case 1:
        launch(&paged_decode_phase1<1, 8, 1, 2>, phase1_lds_bytes(1, 1, hd));
        break;
      case 2:
        launch(&paged_decode_phase1<2, 8, 2, 2>, phase1_lds_bytes(2, 2, hd));
        break;
      case 4:
        // sweep: VALU DP16/HS2/D4 streams 3951 GB/s vs 3348 for the MFMA
        // variant at G=4 (occupancy beats MFMA here) — VALU is production
        launch(&paged_decode_phase1<4, 16, 2, 4>, phase1_lds_bytes(4, 2, hd));
        break;
      case 8:
        if (mfma_ok)
          launch_mfma();
        else
          launch(&paged_decode_phase1<8, 8, 2, 2>,
                 phase1_lds_bytes(8, 2, hd));
        break;
      case 16:
        TORCH_CHECK(mfma_ok, "G=16 requires the MFMA decode path");
        launch_mfma();
        break;
      default:
        // odd groups (e.g. qwen2 G=7): the runtime-G MFMA kernel is the ONLY
        // handler, so the DYNAMO_DECODE_MFMA preference toggle is ignored
        TORCH_CHECK(ps % 32 == 0 && hd == 128 && G <= 16,
                    "GQA group ", G, " needs the MFMA decode path "
                    "(page_size%32==0, head_dim==128)");
        launch_mfma();
        break;
    }
  }
  HIP_CHECK_KERNEL();

  // Phase 2: merge the chunk partials
  if (C > 1) {
    dim3 grid2(B, Hq);
    paged_decode_phase2<<<grid2, 128, 0, stream>>>(
        (short*)out.data_ptr(), partial.data_ptr<float>(), ml.data_ptr<float>(),
        ctx_lens.data_ptr<int32_t>(), chunk, Hq, C, hd);
    HIP_CHECK_KERNEL();
  }
}
