// Python bindings for the dynamo_amd native CDNA4 kernels (dynamo_amd._hip).
#include <torch/extension.h>
#include <pybind11/pybind11.h>

namespace py = pybind11;

// norm.hip
void rmsnorm(torch::Tensor out, torch::Tensor input, torch::Tensor weight,
             double eps, bool allow_fast);
void fused_add_rmsnorm(torch::Tensor input, torch::Tensor residual,
                       torch::Tensor weight, double eps, bool allow_fast);
// rope.hip
void rope_append_qkv(torch::Tensor q_out, torch::Tensor kcache,
                     torch::Tensor vcache, torch::Tensor qkv,
                     c10::optional<torch::Tensor> bias,
                     torch::Tensor positions, torch::Tensor slot_mapping,
                     torch::Tensor cos_sin_cache, bool v_transposed,
                     bool allow_fast);
void rope_inplace(torch::Tensor q, torch::Tensor k, torch::Tensor positions,
                  torch::Tensor cos_sin_cache, int64_t num_q_heads,
                  int64_t num_k_heads, int64_t head_dim);
// activation.hip
void silu_mul(torch::Tensor out, torch::Tensor gate_up);
void gelu(torch::Tensor out, torch::Tensor input);
// cache.hip
void kv_cache_append(torch::Tensor kcache, torch::Tensor vcache, torch::Tensor k,
                     torch::Tensor v, torch::Tensor slot_mapping,
                     bool v_transposed);
void gather_pages(torch::Tensor staging, torch::Tensor cache, torch::Tensor page_ids);
void scatter_pages(torch::Tensor staging, torch::Tensor cache, torch::Tensor page_ids);
void copy_pages(torch::Tensor dst_cache, torch::Tensor src_cache, torch::Tensor pairs);
// attention_decode.hip
int64_t paged_decode_num_chunks(int64_t max_ctx);
int64_t decode_chunk_tokens_py(int64_t max_ctx);
void paged_attention_decode(torch::Tensor out, torch::Tensor q, torch::Tensor kcache,
                            torch::Tensor vcache, torch::Tensor page_table,
                            torch::Tensor ctx_lens, torch::Tensor partial,
                            torch::Tensor ml, double scale,
                            int64_t chunk_tokens, bool v_transposed,
                            int64_t nt_policy);
// attention_prefill.hip
void attention_prefill_paged(torch::Tensor out, torch::Tensor q,
                             torch::Tensor kcache, torch::Tensor vcache,
                             torch::Tensor page_table, torch::Tensor tile_seq,
                             torch::Tensor tile_q0, torch::Tensor seq_q_start,
                             torch::Tensor seq_q_len, torch::Tensor seq_ctx_len,
                             double scale, bool v_transposed);
// sampling.hip
void greedy_sample(torch::Tensor out, torch::Tensor logits, bool allow_fast);
void topkp_sample(torch::Tensor out, torch::Tensor logits,
                  torch::Tensor inv_temp, torch::Tensor top_k,
                  torch::Tensor top_p, int64_t seed,
                  c10::optional<torch::Tensor> row_seeds);
void gumbel_sample(torch::Tensor out, torch::Tensor logits, torch::Tensor inv_temp,
                   int64_t seed, c10::optional<torch::Tensor> row_seeds,
                   bool allow_fast);
// logits_process.hip
void penalty_fold(torch::Tensor counts, torch::Tensor slot,
                  torch::Tensor token, torch::Tensor is_prompt);
void logits_process(torch::Tensor logits, c10::optional<torch::Tensor> counts,
                    torch::Tensor slot, torch::Tensor params,
                    c10::optional<torch::Tensor> bias_off,
                    c10::optional<torch::Tensor> bias_ids,
                    c10::optional<torch::Tensor> bias_vals, bool allow_fast);
// skinny_gemm.hip
void skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor w,
                 int64_t wpb, int64_t u, int64_t nt, bool nontemporal,
                 bool coalesced, bool glu);
std::map<std::string, std::vector<std::tuple<int, int, int>>>
skinny_gemm_configs();
std::map<std::string, std::vector<std::tuple<int, int, int>>>
skinny_gemm_glu_configs();
void fp8_skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor wq,
                     torch::Tensor scale, int64_t wpb, int64_t u, int64_t nt,
                     bool nontemporal, bool glu);
void fp8_dequant(torch::Tensor out, torch::Tensor wq, torch::Tensor scale);
void mxfp4_skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor q,
                       torch::Tensor scale, int64_t wpb, int64_t u,
                       int64_t nt, bool nontemporal, bool glu);
int64_t mxfp4_gemm_max_m();
void mxfp4_dequant(torch::Tensor out, torch::Tensor q, torch::Tensor scale);
// lora.hip
void lora_shrink(torch::Tensor t, torch::Tensor x, torch::Tensor A_bank,
                 torch::Tensor slots, torch::Tensor ranks);
void lora_expand_add(torch::Tensor y, torch::Tensor t, torch::Tensor B_bank,
                     torch::Tensor slots, torch::Tensor ranks,
                     torch::Tensor scales);
// moe.hip
void moe_grouped_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor w,
                      torch::Tensor tiles);
void moe_grouped_gemm_seg(torch::Tensor y, torch::Tensor x, torch::Tensor w,
                          torch::Tensor seg_start, int64_t max_tokens);
void topk_gating(torch::Tensor topw, torch::Tensor topi, torch::Tensor logits);
// ipc.hip
torch::Tensor ipc_alloc(int64_t nbytes, int64_t device);
py::bytes ipc_export(torch::Tensor t);
torch::Tensor ipc_open(py::bytes handle_bytes, int64_t nbytes, int64_t device);
void enable_peer_access(int64_t device, int64_t peer);
// probe.hip
torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B);
torch::Tensor tr16_probe();
torch::Tensor vstage_probe();
torch::Tensor pv_probe(int64_t hot);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "dynamo_amd native MI355X (gfx950) kernels";
  // allow_fast = false keeps an op on its general kernel, so a test can
  // compare the two paths on the same inputs in one process
  m.def("rmsnorm", &rmsnorm, py::arg("out"), py::arg("input"),
        py::arg("weight"), py::arg("eps"), py::arg("allow_fast") = true);
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm, py::arg("input"),
        py::arg("residual"), py::arg("weight"), py::arg("eps"),
        py::arg("allow_fast") = true);
  m.def("rope_inplace", &rope_inplace);
  m.def("rope_append_qkv", &rope_append_qkv,
        py::arg("q_out"), py::arg("kcache"), py::arg("vcache"),
        py::arg("qkv"), py::arg("bias"), py::arg("positions"),
        py::arg("slot_mapping"), py::arg("cos_sin"),
        py::arg("v_transposed") = false, py::arg("allow_fast") = true);
  m.def("silu_mul", &silu_mul);
  m.def("gelu", &gelu);
  m.def("kv_cache_append", &kv_cache_append, py::arg("kcache"),
        py::arg("vcache"), py::arg("k"), py::arg("v"),
        py::arg("slot_mapping"), py::arg("v_transposed") = false);
  m.def("gather_pages", &gather_pages);
  m.def("scatter_pages", &scatter_pages);
  m.def("copy_pages", &copy_pages);
  m.def("paged_decode_num_chunks", &paged_decode_num_chunks);
  m.def("decode_chunk_tokens", &decode_chunk_tokens_py);
  m.def("paged_attention_decode", &paged_attention_decode,
        py::arg("out"), py::arg("q"), py::arg("kcache"), py::arg("vcache"),
        py::arg("page_table"), py::arg("ctx_lens"), py::arg("partial"),
        py::arg("ml"), py::arg("scale"), py::arg("chunk_tokens"),
        py::arg("v_transposed") = false, py::arg("nt_policy") = -1);
  m.def("attention_prefill_paged", &attention_prefill_paged,
        py::arg("out"), py::arg("q"), py::arg("kcache"), py::arg("vcache"),
        py::arg("page_table"), py::arg("tile_seq"), py::arg("tile_q0"),
        py::arg("seq_q_start"), py::arg("seq_q_len"), py::arg("seq_ctx_len"),
        py::arg("scale"), py::arg("v_transposed") = false);
  m.def("greedy_sample", &greedy_sample, py::arg("out"), py::arg("logits"),
        py::arg("allow_fast") = true);
  m.def("gumbel_sample", &gumbel_sample, py::arg("out"), py::arg("logits"),
        py::arg("inv_temp"), py::arg("seed"),
        py::arg("row_seeds") = py::none(), py::arg("allow_fast") = true);
  m.def("topkp_sample", &topkp_sample, py::arg("out"), py::arg("logits"),
        py::arg("inv_temp"), py::arg("top_k"), py::arg("top_p"),
        py::arg("seed"), py::arg("row_seeds") = py::none());
  // per-request logit processors, in place on fp32 logits [B, V]. counts
  // [S, V] int32: bit 0 = token is in the prompt, bits 1.. = its count in the
  // output; slot [B] (-1 = no bank row); params [B, 5] = repetition, presence,
  // frequency, min_p, temperature; bias as CSR over rows. penalty_fold adds
  // entry i (slot, token, is_prompt) to the bank and skips ids out of range
  m.def("penalty_fold", &penalty_fold, py::arg("counts"), py::arg("slot"),
        py::arg("token"), py::arg("is_prompt"));
  m.def("logits_process", &logits_process, py::arg("logits"),
        py::arg("counts"), py::arg("slot"), py::arg("params"),
        py::arg("bias_off") = py::none(), py::arg("bias_ids") = py::none(),
        py::arg("bias_vals") = py::none(), py::arg("allow_fast") = true);
  // y = x @ w^T for 1 <= M <= 16 (decode); raises on anything the kernel
  // does not handle - dispatch and fallback live in ops.linear. glu = true
  // on any of the three GEMMs: w is a gate/up weight [2I, K], y is [M, I] =
  // silu(gate) * up (row-coalesced formats, even NT; ops.linear_silu_mul)
  m.def("skinny_gemm", &skinny_gemm, py::arg("y"), py::arg("x"), py::arg("w"),
        py::arg("wpb") = 4, py::arg("u") = 4, py::arg("nt") = 2,
        py::arg("nontemporal") = false, py::arg("coalesced") = false,
        py::arg("glu") = false);
  // W8A16: y = (x @ bf16(wq)^T) * scale for 1 <= M <= 64, e4m3 weights with
  // one fp32 scale per row; raises on anything the kernel does not handle -
  // dispatch lives in ops.linear
  m.def("fp8_skinny_gemm", &fp8_skinny_gemm, py::arg("y"), py::arg("x"),
        py::arg("wq"), py::arg("scale"), py::arg("wpb") = 1, py::arg("u") = 1,
        py::arg("nt") = 2, py::arg("nontemporal") = true,
        py::arg("glu") = false);
  m.def("fp8_dequant", &fp8_dequant, py::arg("out"), py::arg("wq"),
        py::arg("scale"));
  // W4A16: y = x @ W_eff^T for 1 <= M <= mxfp4_gemm_max_m(), OCP MXFP4
  // weights (q: two e2m1 codes per byte, scale: one e8m0 byte per 32 k);
  // raises on anything the kernel does not handle - dispatch lives in
  // ops.linear
  m.def("mxfp4_skinny_gemm", &mxfp4_skinny_gemm, py::arg("y"), py::arg("x"),
        py::arg("q"), py::arg("scale"), py::arg("wpb") = 1, py::arg("u") = 1,
        py::arg("nt") = 2, py::arg("nontemporal") = true,
        py::arg("glu") = false);
  m.def("mxfp4_gemm_max_m", &mxfp4_gemm_max_m);
  m.def("mxfp4_dequant", &mxfp4_dequant, py::arg("out"), py::arg("q"),
        py::arg("scale"));
  // {"bf16_plain" | "bf16_coalesced" | "fp8" | "mxfp4": [(WPB, U, NT), ...]}:
  // what the GEMM bindings can launch
  m.def("skinny_gemm_configs", &skinny_gemm_configs);
  // the same, restricted to the entries that take glu = true
  m.def("skinny_gemm_glu_configs", &skinny_gemm_glu_configs);
  // batched LoRA: each row i takes the adapter in bank slot slots[i] (a
  // device tensor; < 0 = none), so one captured graph serves any adapter mix.
  // t[i, r] = x[i] . A_bank[s, r] and y[i] += scales[s] * t[i] @ B_bank[s]^T
  // over r < ranks[s]; raises on K, N or R % 8 != 0, misaligned or
  // non-contiguous tensors
  m.def("lora_shrink", &lora_shrink, py::arg("t"), py::arg("x"),
        py::arg("A_bank"), py::arg("slots"), py::arg("ranks"));
  m.def("lora_expand_add", &lora_expand_add, py::arg("y"), py::arg("t"),
        py::arg("B_bank"), py::arg("slots"), py::arg("ranks"),
        py::arg("scales"));
  m.def("moe_grouped_gemm", &moe_grouped_gemm);
  m.def("moe_grouped_gemm_seg", &moe_grouped_gemm_seg);
  m.def("topk_gating", &topk_gating);
  m.def("ipc_alloc", &ipc_alloc);
  m.def("ipc_export", &ipc_export);
  m.def("ipc_open", &ipc_open);
  m.def("enable_peer_access", &enable_peer_access);
  m.def("mfma_probe", &mfma_probe);
  m.def("tr16_probe", &tr16_probe);
  m.def("vstage_probe", &vstage_probe);
  m.def("pv_probe", &pv_probe);
}
