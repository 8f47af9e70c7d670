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

// rope_append_qkv(v_transposed) + paged_attention_decode(v_transposed) of one
// decode step in one phase-1 kernel (see RopeAppendArgs): row b of qkv is the
// new token of sequence b, slot_mapping[b] the slot of token ctx_lens[b] - 1
// under page_table[b] or negative (a padded row: nothing is appended). bf16
// d-major V pages only; everything else takes the two kernels.
void paged_attention_decode_rope(
    torch::Tensor out, torch::Tensor qkv, c10::optional<torch::Tensor> bias,
    torch::Tensor positions, torch::Tensor slot_mapping,
    torch::Tensor cos_sin_cache, torch::Tensor kcache, torch::Tensor vcache,
    torch::Tensor page_table, torch::Tensor ctx_lens, torch::Tensor partial,
    torch::Tensor ml, double scale, int64_t chunk_tokens, int64_t nt_policy) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dtype() == torch::kBFloat16);
  TORCH_CHECK(qkv.dim() == 2 && qkv.stride(1) == 1);
  TORCH_CHECK(out.dim() == 3 && out.is_contiguous() &&
              out.dtype() == torch::kBFloat16);
  TORCH_CHECK(kcache.dtype() == torch::kBFloat16 &&
                  vcache.dtype() == torch::kBFloat16,
              "the fused rope-append decode needs a bf16 kv cache");
  TORCH_CHECK(page_table.dtype() == torch::kInt32 &&
              ctx_lens.dtype() == torch::kInt32 &&
              positions.dtype() == torch::kInt32 &&
              slot_mapping.dtype() == torch::kInt64 &&
              cos_sin_cache.dtype() == torch::kFloat32);
  const int B = out.size(0);
  const int Hq = out.size(1);
  const int hd = out.size(2);
  const int Hkv = kcache.size(1);
  const int ps = kcache.size(2);
  const int G = Hq / Hkv;
  const int max_pages = page_table.size(1);
  const int C = ml.size(2);
  TORCH_CHECK(hd == 128 && kcache.size(3) == hd, "only head_dim=128");
  TORCH_CHECK(partial.dim() == 4 && ml.dim() == 4 && partial.size(0) >= B &&
              ml.size(0) >= B && partial.size(1) == Hq && ml.size(1) == Hq &&
              partial.size(2) == C && partial.size(3) == hd &&
              partial.is_contiguous() && ml.is_contiguous());
  TORCH_CHECK((ps & (ps - 1)) == 0 && ps % 32 == 0,
              "page_size must be a power of 2 and a multiple of 32");
  TORCH_CHECK(Hq == G * Hkv && G >= 2 && G <= 16, "needs 2<=G<=16, got ", G);
  TORCH_CHECK(vcache.size(2) == hd && vcache.size(3) == ps,
              "expects d-major V pages: vcache [P, Hkv, hd, ps]");
  TORCH_CHECK(kcache.is_contiguous() && vcache.is_contiguous() &&
              page_table.is_contiguous() && cos_sin_cache.is_contiguous());
  TORCH_CHECK(cos_sin_cache.dim() == 2 && cos_sin_cache.size(1) == hd);
  // 16-byte vector loads of the qkv rows and the bias
  TORCH_CHECK(qkv.size(0) >= B && qkv.size(1) >= (Hq + 2 * Hkv) * hd &&
              qkv.stride(0) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0);
  TORCH_CHECK(positions.numel() >= B && slot_mapping.numel() >= B &&
              ctx_lens.numel() >= B && page_table.size(0) >= B &&
              positions.is_contiguous() && slot_mapping.is_contiguous());
  const short* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->numel() == (Hq + 2 * Hkv) * hd &&
                bias->dtype() == torch::kBFloat16 && bias->is_contiguous());
    bp = (const short*)bias->data_ptr();
    TORCH_CHECK(reinterpret_cast<uintptr_t>(bp) % 16 == 0);
  }
  int log2_ps = 0; while ((1 << log2_ps) < ps) log2_ps++;
  if (B == 0) return;
  const int chunk = (int)chunk_tokens;
  TORCH_CHECK(chunk >= 128 && chunk % 128 == 0, "bad chunk_tokens ", chunk);
  auto stream = at::cuda::getCurrentHIPStream();
  static const bool nt_env = [] {
    const char* e = getenv("DYNAMO_DECODE_NT");
    return e == nullptr ? kDecodeNtDefault : e[0] != '0';
  }();
  const bool use_nt = nt_policy < 0 ? nt_env : nt_policy != 0;
  const RopeAppendArgs ra{
      (const short*)qkv.data_ptr(), bp, positions.data_ptr<int32_t>(),
      slot_mapping.data_ptr<int64_t>(), cos_sin_cache.data_ptr<float>(),
      (short*)kcache.data_ptr(), (short*)vcache.data_ptr(),
      (int)qkv.stride(0)};
  const int lds = mfma_swapped_lds_bytes(G, hd);
  auto launch = [&](auto* kern) {
    if (lds > 65536)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds);
    kern<<<dim3(B, Hkv, C), kBlock, lds, stream>>>(
        partial.data_ptr<float>(), ml.data_ptr<float>(),
        (short*)out.data_ptr(), (const short*)kcache.data_ptr(),
        (const short*)vcache.data_ptr(), page_table.data_ptr<int32_t>(),
        ctx_lens.data_ptr<int32_t>(), (float)scale, chunk, G, B, Hkv, C,
        max_pages, log2_ps, hd, ra);
  };
  if (use_nt) launch(&paged_decode_mfma_swapped_dmajor_rope<1>);
  else launch(&paged_decode_mfma_swapped_dmajor_rope<0>);
  HIP_CHECK_KERNEL();
  if (C > 1) {
    paged_decode_phase2<<<dim3(B, Hq), 128, 0, stream>>>(
        (short*)out.data_ptr(), partial.data_ptr<float>(), ml.data_ptr<float>(),
        ctx_lens.data_ptr<int32_t>(), chunk, Hq, C, hd);
    HIP_CHECK_KERNEL();
  }
}
