// Per-request logit processors, MI355X-native: repetition / presence /
// frequency penalties, logit_bias and min_p, applied in place to the fp32
// logits between the decode step and the sampling kernels (sampling.hip).
//
// State is one int32 per (slot, token) in a [slots, V] bank: bit 0 says the
// token occurs in the request's prompt, bits 1.. count its occurrences in the
// output so far (word == 0: never seen). penalty_fold keeps the bank current
// from the host's token lists with integer atomics; logits_process streams
// one bank row next to one logits row.
//
// Order on a row (the contract; reference in ops/torch_ref.py):
//   1. repetition (r != 1), prompt or output tokens: l = l > 0 ? l / r : l * r
//   2. output tokens: l -= freq * cnt + pres
//   3. l[id] += bias
//   4. min_p (min_p > 0, T > 0): l = -inf where (l - max l) / T < ln(min_p)
// A row whose parameters are all neutral is not touched at all.
#include "common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

constexpr int kBlock = 512;
constexpr int kUnroll = 8;   // 16-byte loads in flight per thread and stream
constexpr int kParams = 5;   // per row: repetition, presence, frequency,
                             // min_p, temperature

// A bank row starts wherever slot * V falls, and the sweep below is aligned
// to the logits row, so bank vectors are only known to be 4-byte aligned.
// gfx950 serves a dword-aligned 16-byte global load in one instruction.
typedef int int4u __attribute__((ext_vector_type(4), aligned(4)));

__global__ void penalty_fold_kernel(int32_t* __restrict__ counts,  // [S, V]
                                    const int32_t* __restrict__ slot,
                                    const int32_t* __restrict__ token,
                                    const int32_t* __restrict__ is_prompt,
                                    int n, int S, int V) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i], t = token[i];
  if (s < 0 || s >= S || t < 0 || t >= V) return;
  int32_t* w = counts + (int64_t)s * V + t;
  if (is_prompt[i]) atomicOr(w, 1); else atomicAdd(w, 2);
}

// One pass over a logits row (and its bank row if COUNTS): f(l, w, v) gives
// element v's new value, and a 16-byte vector (a scalar in the head, the tail
// and the !FAST form) is stored only if a bit of it changed. FAST reads as
// sample_kernel's FAST path does: 16-byte vectors from the first 16-byte
// boundary of the row, scalars before it and after the last whole vector.
template <bool FAST, bool COUNTS, typename F>
DEVINL void row_sweep(float* __restrict__ row, const int32_t* __restrict__ crow,
                      int V, F f) {
  auto scalar = [&](int v) {
    const float l = row[v];
    const float x = f(l, COUNTS ? crow[v] : 0, v);
    if (__float_as_uint(x) != __float_as_uint(l)) row[v] = x;
  };
  if constexpr (FAST) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
    const int head = min(V, (4 - mis) & 3);
    const int n4 = (V - head) / 4;
    float4v* row4 = reinterpret_cast<float4v*>(row + head);
    const int4u* crow4 = reinterpret_cast<const int4u*>(crow + head);
    for (int i0 = 0; i0 < n4; i0 += kUnroll * kBlock) {
      float4v r[kUnroll];
      int4u c[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; u++) {
        const int i = i0 + u * kBlock + threadIdx.x;
        if (i < n4) {
          r[u] = row4[i];
          if constexpr (COUNTS) c[u] = crow4[i];
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; u++) {
        const int i = i0 + u * kBlock + threadIdx.x;
        if (i < n4) {
          float4v x;
          bool changed = false;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            x[e] = f(r[u][e], COUNTS ? c[u][e] : 0, head + i * 4 + e);
            changed |= __float_as_uint(x[e]) != __float_as_uint(r[u][e]);
          }
          if (changed) row4[i] = x;
        }
      }
    }
    if ((int)threadIdx.x < head) scalar(threadIdx.x);
    const int v = head + n4 * 4 + threadIdx.x;
    if (v < V) scalar(v);
  } else {
    for (int v = threadIdx.x; v < V; v += kBlock) scalar(v);
  }
}

// One workgroup per row; rows are independent.
template <bool FAST>
__global__ __launch_bounds__(kBlock) void logits_process_kernel(
    float* __restrict__ logits,           // [B, V], in place
    const int32_t* __restrict__ counts,   // [S, V] or null
    const int32_t* __restrict__ slot,     // [B], -1: no bank row
    const float* __restrict__ params,     // [B, kParams]
    const int32_t* __restrict__ bias_off, // [B + 1] or null
    const int32_t* __restrict__ bias_ids,
    const float* __restrict__ bias_vals,
    int nnz, int S, int V) {
  const int b = blockIdx.x;
  const float* p = params + b * kParams;
  const float rep = p[0], pres = p[1], freq = p[2], min_p = p[3], temp = p[4];
  const int s = slot[b];
  const bool penalise = counts != nullptr && s >= 0 && s < S &&
                        (rep != 1.f || pres != 0.f || freq != 0.f);
  const int b0 = bias_off ? max(bias_off[b], 0) : 0;
  const int b1 = bias_off ? min(bias_off[b + 1], nnz) : 0;
  const bool filter = min_p > 0.f && temp > 0.f;
  if (!penalise && b1 <= b0 && !filter) return;

  float* row = logits + (int64_t)b * V;
  if (penalise) {
    row_sweep<FAST, true>(
        row, counts + (int64_t)s * V, V, [&](float l, int32_t w, int) {
          if (w == 0) return l;
          if (rep != 1.f) l = l > 0.f ? l / rep : l * rep;
          const int cnt = w >> 1;
          if (cnt > 0) l -= freq * (float)cnt + pres;
          return l;
        });
  }
  if (b1 > b0) {
    // ids are distinct within a row (they come from a dict)
    if (penalise) __syncthreads();
    for (int j = b0 + threadIdx.x; j < b1; j += kBlock) {
      const int v = bias_ids[j];
      if (v >= 0 && v < V) row[v] += bias_vals[j];
    }
  }
  if (!filter) return;

  // the row was just written by this workgroup: both passes below read it
  // from L2
  if (penalise || b1 > b0) __syncthreads();
  float m = -INFINITY;
  row_sweep<FAST, false>(row, nullptr, V, [&](float l, int32_t, int) {
    m = fmaxf(m, l);
    return l;
  });
  m = wave_reduce_max(m);
  __shared__ float red[kBlock / WAVE_SIZE];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x / WAVE_SIZE] = m;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kBlock / WAVE_SIZE; w++) m = fmaxf(m, red[w]);
  // (l - m) / T < ln(min_p), without a division per element
  const float thr = logf(min_p) * temp;
  row_sweep<FAST, false>(row, nullptr, V, [&](float l, int32_t, int) {
    return l - m < thr ? -INFINITY : l;
  });
}

const int32_t* i32_ptr(const torch::Tensor& t, int64_t n, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kInt32 &&
              t.is_contiguous() && t.numel() == n, what,
              ": expected a contiguous int32 device tensor of ", n,
              " elements");
  return t.data_ptr<int32_t>();
}

}  // namespace

void penalty_fold(torch::Tensor counts, torch::Tensor slot,
                  torch::Tensor token, torch::Tensor is_prompt) {
  TORCH_CHECK(counts.is_cuda() && counts.dtype() == torch::kInt32 &&
              counts.dim() == 2 && counts.is_contiguous());
  const int64_t n = slot.numel();
  if (n == 0) return;
  TORCH_CHECK(n < (1ll << 31));
  const int32_t* sp = i32_ptr(slot, n, "slot");
  const int32_t* tp = i32_ptr(token, n, "token");
  const int32_t* pp = i32_ptr(is_prompt, n, "is_prompt");
  auto stream = at::cuda::getCurrentHIPStream();
  penalty_fold_kernel<<<(int)((n + 255) / 256), 256, 0, stream>>>(
      counts.data_ptr<int32_t>(), sp, tp, pp, (int)n, (int)counts.size(0),
      (int)counts.size(1));
  HIP_CHECK_KERNEL();
}

void logits_process(torch::Tensor logits, c10::optional<torch::Tensor> counts,
                    torch::Tensor slot, torch::Tensor params,
                    c10::optional<torch::Tensor> bias_off,
                    c10::optional<torch::Tensor> bias_ids,
                    c10::optional<torch::Tensor> bias_vals, bool allow_fast) {
  TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kFloat32 &&
              logits.dim() == 2 && logits.is_contiguous());
  const int B = logits.size(0);
  const int V = logits.size(1);
  if (B == 0) return;
  const int32_t* cp = nullptr;
  int S = 0;
  if (counts.has_value()) {
    TORCH_CHECK(counts->is_cuda() && counts->dtype() == torch::kInt32 &&
                counts->dim() == 2 && counts->is_contiguous() &&
                counts->size(1) == V);
    cp = counts->data_ptr<int32_t>();
    S = counts->size(0);
  }
  const int32_t* sp = i32_ptr(slot, B, "slot");
  TORCH_CHECK(params.is_cuda() && params.dtype() == torch::kFloat32 &&
              params.is_contiguous() && params.numel() == (int64_t)B * kParams);
  const int32_t* op = nullptr;
  const int32_t* ip = nullptr;
  const float* vp = nullptr;
  int nnz = 0;
  if (bias_off.has_value()) {
    TORCH_CHECK(bias_ids.has_value() && bias_vals.has_value());
    op = i32_ptr(*bias_off, B + 1, "bias offsets");
    ip = i32_ptr(*bias_ids, bias_ids->numel(), "bias ids");
    TORCH_CHECK(bias_vals->is_cuda() && bias_vals->dtype() == torch::kFloat32 &&
                bias_vals->is_contiguous() &&
                bias_vals->numel() == bias_ids->numel());
    vp = bias_vals->data_ptr<float>();
    nnz = (int)bias_ids->numel();
  }
  auto stream = at::cuda::getCurrentHIPStream();
  auto kern = allow_fast ? logits_process_kernel<true>
                         : logits_process_kernel<false>;
  kern<<<B, kBlock, 0, stream>>>(logits.data_ptr<float>(), cp, sp,
                                 params.data_ptr<float>(), op, ip, vp, nnz, S, V);
  HIP_CHECK_KERNEL();
}
