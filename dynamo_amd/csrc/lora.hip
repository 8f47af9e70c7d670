// Batched (per-row gathered) LoRA delta for the decode step:
//   t[i, r] = sum_k x[i, k] * A_bank[slots[i], r, k]            (lora_shrink)
//   y[i, n] = bf16(y[i, n] + scales[s] * sum_r t[i, r] * B_bank[s, n, r])
//                                                           (lora_expand_add)
// for r < ranks[s], s = slots[i]; a row with slots[i] < 0 is left alone.
//
// Every row picks its adapter on the device, so the launch needs no host
// knowledge of `slots` and one captured graph serves any adapter mix. Both
// kernels are bandwidth-bound gathers over the adapter bank:
//  - shrink: one block per (row, r) dot product over a K-contiguous A row;
//    its 4 waves interleave 16-byte loads over k (one fp32 accumulator per
//    lane in ascending k, then the xor butterfly of wave_reduce_sum) and the
//    4 wave sums are added in wave order. 4 waves per dot product, not 1:
//    at rank 16 a 16-row batch has only 256 dot products for 256 CUs, and
//    the down projection's K = 28672 is 57 KB per A row;
//  - expand: a lane owns two consecutive n, walks the R-contiguous B rows in
//    16-byte pieces in ascending r, rounds once.
// The order of every sum depends on K, R and the slot's rank alone, never on
// T, the row's position or its batch-mates: results are bit-identical from
// run to run and from batch to batch. No atomics. The bank is read with the
// default cache policy (batch-mates on one adapter re-read it out of L2).
// Bank entries at r >= ranks[s] and slots no row names are never loaded.
#include "common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

constexpr int kShrinkWaves = 4;                  // waves per (row, r) pair
constexpr int kShrinkBlock = kShrinkWaves * WAVE_SIZE;
constexpr int kExpandBlock = 256;
constexpr int kExpandNPerLane = 2;

// the slot's rank, 0 for "no adapter" (slot < 0, or a slot outside the bank)
DEVINL int row_rank(const int* __restrict__ slots,
                    const int* __restrict__ ranks, int row, int S, int R,
                    int* slot_out) {
  const int s = slots[row];
  *slot_out = s;
  if (s < 0 || s >= S) return 0;
  const int rk = ranks[s];
  return rk < 0 ? 0 : (rk > R ? R : rk);
}

__global__ __launch_bounds__(kShrinkBlock)
void lora_shrink_kernel(float* __restrict__ t,            // [T, R]
                        const short* __restrict__ x,      // [T, K]
                        const short* __restrict__ A,      // [S, R, K]
                        const int* __restrict__ slots,    // [T]
                        const int* __restrict__ ranks,    // [S]
                        int S, int R, int K) {
  __shared__ float wave_sum[kShrinkWaves];
  const int row = blockIdx.y;
  const int r = blockIdx.x;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  int s;
  const int rank = row_rank(slots, ranks, row, S, R, &s);
  if (r >= rank) return;                         // block-uniform
  const short* xr = x + (size_t)row * K;
  const short* ar = A + ((size_t)s * R + r) * (size_t)K;
  float acc = 0.f;
#pragma unroll 4
  for (int k0 = threadIdx.x * 8; k0 < K; k0 += kShrinkBlock * 8) {
    const short8 xv = *reinterpret_cast<const short8*>(xr + k0);
    const short8 av = *reinterpret_cast<const short8*>(ar + k0);
#pragma unroll
    for (int j = 0; j < 8; j++)
      acc = fmaf(bf16_to_f32(xv[j]), bf16_to_f32(av[j]), acc);
  }
  acc = wave_reduce_sum(acc);
  if (lane == 0) wave_sum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = wave_sum[0];
#pragma unroll
    for (int w = 1; w < kShrinkWaves; w++) sum += wave_sum[w];
    t[(size_t)row * R + r] = sum;
  }
}

__global__ __launch_bounds__(kExpandBlock)
void lora_expand_add_kernel(short* __restrict__ y,           // [T, N]
                            const float* __restrict__ t,     // [T, R]
                            const short* __restrict__ B,     // [S, N, R]
                            const int* __restrict__ slots,   // [T]
                            const int* __restrict__ ranks,   // [S]
                            const float* __restrict__ scales,  // [S]
                            int S, int R, int N) {
  const int row = blockIdx.y;
  int s;
  const int rank = row_rank(slots, ranks, row, S, R, &s);
  if (rank == 0) return;                         // block-uniform
  const int n0 = (blockIdx.x * kExpandBlock + threadIdx.x) * kExpandNPerLane;
  if (n0 >= N) return;                           // N is even: n0 + 1 < N
  const float scale = scales[s];
  const float* tr = t + (size_t)row * R;         // uniform address
  const short* b0 = B + ((size_t)s * N + n0) * (size_t)R;
  const short* b1 = b0 + R;
  float acc0 = 0.f, acc1 = 0.f;
  const int full = rank & ~7;
  for (int r0 = 0; r0 < full; r0 += 8) {
    const short8 v0 = *reinterpret_cast<const short8*>(b0 + r0);
    const short8 v1 = *reinterpret_cast<const short8*>(b1 + r0);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float tv = tr[r0 + j];
      acc0 = fmaf(tv, bf16_to_f32(v0[j]), acc0);
      acc1 = fmaf(tv, bf16_to_f32(v1[j]), acc1);
    }
  }
  // a rank that is no multiple of 8: element loads, so that nothing at
  // r >= rank is touched
  for (int r = full; r < rank; r++) {
    const float tv = tr[r];
    acc0 = fmaf(tv, bf16_to_f32(b0[r]), acc0);
    acc1 = fmaf(tv, bf16_to_f32(b1[r]), acc1);
  }
  uint32_t* yp = reinterpret_cast<uint32_t*>(y + (size_t)row * N + n0);
  const uint32_t yv = *yp;
  const float y0 = bf16_to_f32((short)(yv & 0xffffu));
  const float y1 = bf16_to_f32((short)(yv >> 16));
  const uint32_t o0 = (uint16_t)f32_to_bf16(fmaf(scale, acc0, y0));
  const uint32_t o1 = (uint16_t)f32_to_bf16(fmaf(scale, acc1, y1));
  *yp = o0 | (o1 << 16);
}

void check_common(const torch::Tensor& slots, const torch::Tensor& ranks,
                  int64_t T, int64_t S) {
  TORCH_CHECK(slots.is_cuda() && slots.dtype() == torch::kInt32 &&
              slots.is_contiguous() && slots.dim() == 1 && slots.size(0) == T,
              "lora: slots must be a contiguous int32 [T] device tensor");
  TORCH_CHECK(ranks.is_cuda() && ranks.dtype() == torch::kInt32 &&
              ranks.is_contiguous() && ranks.dim() == 1 && ranks.size(0) == S,
              "lora: ranks must be a contiguous int32 [S] device tensor");
}

bool aligned16(const torch::Tensor& v) {
  return reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0;
}

}  // namespace

void lora_shrink(torch::Tensor t, torch::Tensor x, torch::Tensor A_bank,
                 torch::Tensor slots, torch::Tensor ranks) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.dim() == 2,
              "lora_shrink: x must be a bf16 [T, K] device tensor");
  TORCH_CHECK(A_bank.is_cuda() && A_bank.dtype() == torch::kBFloat16 &&
              A_bank.dim() == 3,
              "lora_shrink: A_bank must be a bf16 [S, R, K] device tensor");
  TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32 && t.dim() == 2,
              "lora_shrink: t must be an fp32 [T, R] device tensor");
  const int64_t T = x.size(0), K = x.size(1);
  const int64_t S = A_bank.size(0), R = A_bank.size(1);
  TORCH_CHECK(T >= 1 && T <= 65535, "lora_shrink: need 1 <= T <= 65535");
  TORCH_CHECK(A_bank.size(2) == K && t.size(0) == T && t.size(1) == R,
              "lora_shrink: shape mismatch");
  TORCH_CHECK(K >= 8 && K % 8 == 0 && R >= 8 && R % 8 == 0,
              "lora_shrink: K and R must be multiples of 8");
  TORCH_CHECK(S >= 1 && S * R * K < (int64_t(1) << 40));
  TORCH_CHECK(x.is_contiguous() && A_bank.is_contiguous() && t.is_contiguous(),
              "lora_shrink: tensors must be contiguous");
  TORCH_CHECK(aligned16(x) && aligned16(A_bank) && aligned16(t),
              "lora_shrink: base pointers must be 16-byte aligned");
  check_common(slots, ranks, T, S);
  dim3 grid((unsigned)R, (unsigned)T);
  auto stream = at::cuda::getCurrentHIPStream();
  lora_shrink_kernel<<<grid, kShrinkBlock, 0, stream>>>(
      (float*)t.data_ptr(), (const short*)x.data_ptr(),
      (const short*)A_bank.data_ptr(), (const int*)slots.data_ptr(),
      (const int*)ranks.data_ptr(), (int)S, (int)R, (int)K);
  HIP_CHECK_KERNEL();
}

void lora_expand_add(torch::Tensor y, torch::Tensor t, torch::Tensor B_bank,
                     torch::Tensor slots, torch::Tensor ranks,
                     torch::Tensor scales) {
  TORCH_CHECK(y.is_cuda() && y.dtype() == torch::kBFloat16 && y.dim() == 2,
              "lora_expand_add: y must be a bf16 [T, N] device tensor");
  TORCH_CHECK(B_bank.is_cuda() && B_bank.dtype() == torch::kBFloat16 &&
              B_bank.dim() == 3,
              "lora_expand_add: B_bank must be a bf16 [S, N, R] device tensor");
  TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32 && t.dim() == 2,
              "lora_expand_add: t must be an fp32 [T, R] device tensor");
  const int64_t T = y.size(0), N = y.size(1);
  const int64_t S = B_bank.size(0), R = B_bank.size(2);
  TORCH_CHECK(T >= 1 && T <= 65535, "lora_expand_add: need 1 <= T <= 65535");
  TORCH_CHECK(B_bank.size(1) == N && t.size(0) == T && t.size(1) == R,
              "lora_expand_add: shape mismatch");
  TORCH_CHECK(N >= 8 && N % 8 == 0 && R >= 8 && R % 8 == 0,
              "lora_expand_add: N and R must be multiples of 8");
  TORCH_CHECK(S >= 1 && S * N * R < (int64_t(1) << 40) &&
              N < (int64_t(1) << 30));
  TORCH_CHECK(y.is_contiguous() && B_bank.is_contiguous() && t.is_contiguous(),
              "lora_expand_add: tensors must be contiguous");
  TORCH_CHECK(aligned16(y) && aligned16(B_bank) && aligned16(t),
              "lora_expand_add: base pointers must be 16-byte aligned");
  check_common(slots, ranks, T, S);
  TORCH_CHECK(scales.is_cuda() && scales.dtype() == torch::kFloat32 &&
              scales.is_contiguous() && scales.dim() == 1 &&
              scales.size(0) == S,
              "lora_expand_add: scales must be a contiguous fp32 [S] device "
              "tensor");
  constexpr int per_block = kExpandBlock * kExpandNPerLane;
  dim3 grid((unsigned)((N + per_block - 1) / per_block), (unsigned)T);
  auto stream = at::cuda::getCurrentHIPStream();
  lora_expand_add_kernel<<<grid, kExpandBlock, 0, stream>>>(
      (short*)y.data_ptr(), (const float*)t.data_ptr(),
      (const short*)B_bank.data_ptr(), (const int*)slots.data_ptr(),
      (const int*)ranks.data_ptr(), (const float*)scales.data_ptr(), (int)S,
      (int)R, (int)N);
  HIP_CHECK_KERNEL();
}
