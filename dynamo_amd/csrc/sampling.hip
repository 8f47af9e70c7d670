// Token sampling kernels, MI355X-native.
//
// greedy: fused argmax over the vocab.
// gumbel: exact softmax(logits/T) sampling via the Gumbel-max trick —
//   argmax(logits/T + G_i), G_i = -log(-log(U_i)) with a counter-based
//   in-kernel hash RNG (deterministic given seed; no host noise tensor).
// Both are single-pass, vectorized, one workgroup per sequence.
// top-k / top-p: one fused kernel, exact per-row thresholds by a search on
//   the logit's bit pattern (top-k, then the nucleus of the survivors), then
//   the same Gumbel argmax over the surviving set (topkp_sample_kernel below).
//
// Capability parity: the reference delegates sampling to its engines; this
// is the native path. Penalties, logit_bias and min_p edit the logits before
// any of these kernels runs (logits_process.hip).
#include "common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

constexpr int kBlock = 512;
constexpr int kScanUnroll = 8;  // 16-byte loads in flight per thread

DEVINL uint64_t hash_u64(uint64_t x) {
  // splitmix64 finalizer
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// One candidate of the argmax scan. The winner rule (strictly greater, or
// equal with the lower index) is a total order on (score, index), so the
// result does not depend on the order in which candidates are scanned.
template <bool GUMBEL>
DEVINL void sample_consider(float logit, int v, float it, uint64_t rs,
                            float& best, int& besti) {
  float x = logit * it;
  if constexpr (GUMBEL) {
    const uint64_t h = hash_u64(rs ^ (uint64_t)v);
    // uniform in (0,1): use top 53 bits
    const float u = (float)((h >> 11) + 1) * 4.8828125e-4f * 2.2737367544323206e-13f;
    x += -__logf(-__logf(u));
  }
  if (x > best || (x == best && v < besti)) { best = x; besti = v; }
}

// FAST: the row is read as 16-byte vectors, kScanUnroll loads in flight per
// thread, with a scalar head up to the first 16-byte boundary (rows of a
// V % 4 != 0 matrix start unaligned) and a scalar tail. !FAST: one scalar
// load per iteration.
template <bool GUMBEL, bool FAST>
__global__ __launch_bounds__(kBlock) void sample_kernel(
    int32_t* __restrict__ out,          // [B]
    const float* __restrict__ logits,   // [B, V]
    const float* __restrict__ inv_temp, // [B] or null
    uint64_t seed,
    const uint64_t* __restrict__ row_seeds,  // [B] or null
    int V) {
  const int b = blockIdx.x;
  const float* row = logits + (int64_t)b * V;
  const float it = GUMBEL ? inv_temp[b] : 1.f;
  // per-row seed (client-supplied sampling seed, already host-mixed with
  // the output position) or the scalar engine-step stream
  const uint64_t rs = row_seeds ? row_seeds[b] : (seed ^ ((uint64_t)b << 32));

  float best = -1e38f;
  int besti = -1;
  if constexpr (FAST) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
    const int head = min(V, (4 - mis) & 3);
    const int n4 = (V - head) / 4;
    const float4v* row4 = reinterpret_cast<const float4v*>(row + head);
    for (int i0 = 0; i0 < n4; i0 += kScanUnroll * kBlock) {
      float4v r[kScanUnroll];
#pragma unroll
      for (int u = 0; u < kScanUnroll; u++) {
        const int i = i0 + u * kBlock + threadIdx.x;
        if (i < n4) r[u] = row4[i];
      }
#pragma unroll
      for (int u = 0; u < kScanUnroll; u++) {
        const int i = i0 + u * kBlock + threadIdx.x;
        if (i < n4) {
#pragma unroll
          for (int e = 0; e < 4; e++)
            sample_consider<GUMBEL>(r[u][e], head + i * 4 + e, it, rs, best,
                                    besti);
        }
      }
    }
    // scalar head and tail: at most 3 elements each
    if ((int)threadIdx.x < head)
      sample_consider<GUMBEL>(row[threadIdx.x], threadIdx.x, it, rs, best,
                              besti);
    const int v = head + n4 * 4 + threadIdx.x;
    if (v < V) sample_consider<GUMBEL>(row[v], v, it, rs, best, besti);
  } else {
    for (int v = threadIdx.x; v < V; v += kBlock)
      sample_consider<GUMBEL>(row[v], v, it, rs, best, besti);
  }
  // wave reduce (value, index)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off, WAVE_SIZE);
    const int oi = __shfl_xor(besti, off, WAVE_SIZE);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  __shared__ float sb[kBlock / WAVE_SIZE];
  __shared__ int si[kBlock / WAVE_SIZE];
  const int wid = threadIdx.x / WAVE_SIZE;
  if ((threadIdx.x & 63) == 0) { sb[wid] = best; si[wid] = besti; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / WAVE_SIZE; w++) {
      if (sb[w] > best || (sb[w] == best && si[w] < besti)) { best = sb[w]; besti = si[w]; }
    }
    out[b] = besti;
  }
}

// Order-preserving key of an fp32: a < b as floats iff key(a) < key(b) as
// unsigned integers (-0 is folded into +0; NaNs land beyond the infinities).
DEVINL uint32_t float_key(float x) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// f(row[v], v) once for every v in [0, V) over the threads of the block,
// each thread in the same order on every call: 16-byte loads, kScanUnroll in
// flight per thread, with the scalar head and tail of sample_kernel<, true>
// (valid for any V and any row alignment).
template <class F>
DEVINL void scan_row(const float* __restrict__ row, int V, F&& f) {
  const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
  const int head = min(V, (4 - mis) & 3);
  const int n4 = (V - head) / 4;
  const float4v* row4 = reinterpret_cast<const float4v*>(row + head);
  for (int i0 = 0; i0 < n4; i0 += kScanUnroll * kBlock) {
    float4v r[kScanUnroll];
#pragma unroll
    for (int u = 0; u < kScanUnroll; u++) {
      const int i = i0 + u * kBlock + threadIdx.x;
      if (i < n4) r[u] = row4[i];
    }
#pragma unroll
    for (int u = 0; u < kScanUnroll; u++) {
      const int i = i0 + u * kBlock + threadIdx.x;
      if (i < n4) {
#pragma unroll
        for (int e = 0; e < 4; e++) f(r[u][e], head + i * 4 + e);
      }
    }
  }
  if ((int)threadIdx.x < head) f(row[threadIdx.x], (int)threadIdx.x);
  const int v = head + n4 * 4 + threadIdx.x;
  if (v < V) f(row[v], v);
}

constexpr int kCand = 8;  // thresholds tried per pass: 3 bits of the key

// The smallest key t in [lo, hi] with stat(t) <= bound, where
//   stat(t) = sum over { v : key(row[v]) > t } of w_v,
// w_v = 1 (MASS false: a count) or __expf(row[v] - m) (MASS true: a mass,
// and bound = top_p * stat(lo), taken from the first pass). Within a pass
// stat does not grow with t, in fp32 too: the candidates add subsets of the
// same terms in the same order. Across passes `base` is an earlier pass's
// sum, so two passes can differ by fp32 rounding (~1e-7 of the mass). The
// row is taken to hold no NaN (fmaxf skips one, so its key lies above hi
// and neither search counts it; the final scan never draws it), and counts
// are summed in fp32, exact for V < 2^24. hi is taken to meet the bound
// without being tried, so the result never exceeds it. Each pass tries kCand keys that cut [lo, hi] into equal
// parts, so 11 passes settle all 32 bits; elements at or below lo no longer
// count and the ones above hi are carried in `base`, so once the range has
// narrowed to a few exponents most waves skip most of the row. A count that
// hits k exactly ends the search: that set is the top k.
// `red` is kCand * kWaves floats of LDS. Every thread returns the same key.
template <bool MASS>
DEVINL uint32_t search_threshold(const float* __restrict__ row, int V, float m,
                                 uint32_t lo, uint32_t hi, float bound,
                                 float top_p, float* red) {
  constexpr int kWaves = kBlock / WAVE_SIZE;
  float base = 0.f;  // stat(hi)
  bool first = true;
  while (lo < hi) {
    const uint32_t step = (hi - lo) / kCand + 1;
    uint32_t c[kCand];
#pragma unroll
    for (int j = 0; j < kCand; j++)
      c[j] = (uint32_t)min((uint64_t)lo + (uint64_t)j * step, (uint64_t)hi);
    float acc[kCand];
#pragma unroll
    for (int j = 0; j < kCand; j++) acc[j] = 0.f;
    scan_row(row, V, [&](float x, int) {
      const uint32_t key = float_key(x);
      if (key > lo && key <= hi) {
        const float w = MASS ? __expf(x - m) : 1.f;
#pragma unroll
        for (int j = 0; j < kCand; j++) acc[j] += key > c[j] ? w : 0.f;
      }
    });
#pragma unroll
    for (int j = 0; j < kCand; j++) acc[j] = wave_reduce_sum(acc[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int j = 0; j < kCand; j++)
        red[j * kWaves + threadIdx.x / WAVE_SIZE] = acc[j];
    }
    __syncthreads();
    float stat[kCand];
#pragma unroll
    for (int j = 0; j < kCand; j++) {
      float s = red[j * kWaves];
      for (int w = 1; w < kWaves; w++) s += red[j * kWaves + w];
      stat[j] = base + s;
    }
    __syncthreads();
    if (MASS && first) bound = top_p * stat[0];
    first = false;
    // the candidates below hi, in order, up to the first that meets the
    // bound: it becomes hi, the last one that misses it becomes lo - 1
    uint32_t new_lo = lo, new_hi = hi;
    bool done = false, exact = false;
#pragma unroll
    for (int j = 0; j < kCand; j++) {
      if (done || c[j] >= hi) {
        done = true;
      } else if (stat[j] <= bound) {
        new_hi = c[j];
        base = stat[j];
        done = true;
      } else {
        new_lo = c[j] + 1;
        exact = !MASS && stat[j] == bound + 1.f;
      }
    }
    lo = new_lo;
    hi = exact ? new_lo : new_hi;
  }
  return lo;
}

// Fused top-k / top-p (nucleus) sampling: one block per row, no sort.
//
// The keep set is torch_ref.topkp_keep_mask, exactly: top-k first, every
// entry >= the k-th largest logit (a tie at the boundary is kept whole);
// then the nucleus of the softmax over those survivors, a token being kept
// iff the mass of the tokens strictly above it is <= top_p times the
// survivors' mass. Both are thresholds on the logit, found by a search on
// its order-preserving bit pattern (search_threshold), so they are exact
// values of the row whatever its scale, and the top-k one needs no
// exponential. A row runs only the searches its parameters switch on. The
// threshold never exceeds the row maximum: the argmax survives any top_p
// and -1 is never written for a row with a finite entry. The final pass is
// gumbel_sample's scan (sample_consider) over the surviving set, which
// samples the renormalized filtered distribution exactly and equals
// gumbel_sample on the -inf masked row token for token. The keep set is
// defined on the T=1 softmax, as in engine/sampling.py::_filter_topk_topp;
// temperature only shapes sampling inside the set. Single launch, no host
// sync, hipGraph-capturable.
__global__ __launch_bounds__(kBlock) void topkp_sample_kernel(
    int32_t* __restrict__ out,          // [B]
    const float* __restrict__ logits,   // [B, V]
    const float* __restrict__ inv_temp, // [B]
    const int32_t* __restrict__ top_k,  // [B] (<=0 or >=V: off)
    const float* __restrict__ top_p,    // [B] (>=1: off)
    uint64_t seed,
    const uint64_t* __restrict__ row_seeds,  // [B] or null
    int V) {
  const int b = blockIdx.x;
  const uint64_t rs = row_seeds ? row_seeds[b] : (seed ^ ((uint64_t)b << 32));
  const float* row = logits + (int64_t)b * V;
  const int k = top_k[b];
  const float p = top_p[b];
  const bool use_k = (k > 0 && k < V);
  const bool use_p = (p < 1.0f);
  constexpr int kWaves = kBlock / WAVE_SIZE;
  __shared__ float red[kCand * kWaves];
  __shared__ float bcast;

  uint32_t thr = 0;  // keep { v : key(row[v]) >= thr }
  if (use_k || use_p) {
    // row max: the top of both searches, and the softmax shift
    float m = -1e38f;
    scan_row(row, V, [&](float x, int) { m = fmaxf(m, x); });
    m = wave_reduce_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x / WAVE_SIZE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < kWaves; w++) m = fmaxf(m, red[w]);
      bcast = m;
    }
    __syncthreads();
    m = bcast;
    __syncthreads();
    const uint32_t top = float_key(m);
    // the k-th largest key: the smallest t with count(key > t) <= k - 1
    if (use_k)
      thr = search_threshold<false>(row, V, m, 0, top, (float)(k - 1), 0.f,
                                    red);
    // the nucleus over { key >= thr }: starting one below thr makes the
    // first pass's stat(lo) the survivors' mass
    if (use_p) {
      const uint32_t lo = thr > 0 ? thr - 1 : 0;
      thr = max(thr, search_threshold<true>(row, V, m, lo, top, 0.f, p, red));
    }
  }

  // final pass: Gumbel-argmax of logits/T over the surviving set
  const float it_ = inv_temp[b];
  float best = -1e38f;
  int besti = -1;
  scan_row(row, V, [&](float x, int v) {
    if (float_key(x) >= thr) sample_consider<true>(x, v, it_, rs, best, besti);
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off, WAVE_SIZE);
    const int oi = __shfl_xor(besti, off, WAVE_SIZE);
    if (ob > best || (ob == best && oi != -1 && (besti == -1 || oi < besti))) {
      best = ob; besti = oi;
    }
  }
  __shared__ float sb2[kWaves];
  __shared__ int si2[kWaves];
  const int wid = threadIdx.x / WAVE_SIZE;
  if ((threadIdx.x & 63) == 0) { sb2[wid] = best; si2[wid] = besti; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; w++) {
      if (sb2[w] > best || (sb2[w] == best && si2[w] != -1 &&
                            (besti == -1 || si2[w] < besti))) {
        best = sb2[w]; besti = si2[w];
      }
    }
    out[b] = besti;
  }
}

}  // namespace

void greedy_sample(torch::Tensor out, torch::Tensor logits, bool allow_fast) {
  TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kFloat32);
  TORCH_CHECK(out.dtype() == torch::kInt32);
  const int B = logits.size(0);
  const int V = logits.size(1);
  if (B == 0) return;
  auto stream = at::cuda::getCurrentHIPStream();
  auto kern = allow_fast ? sample_kernel<false, true>
                         : sample_kernel<false, false>;
  kern<<<B, kBlock, 0, stream>>>(out.data_ptr<int32_t>(),
                                 logits.data_ptr<float>(), nullptr, 0, nullptr,
                                 V);
  HIP_CHECK_KERNEL();
}

static const uint64_t* opt_seeds(const c10::optional<torch::Tensor>& t,
                                 int B) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->dtype() == torch::kInt64 && t->numel() == B &&
              t->is_cuda() && t->is_contiguous());
  return reinterpret_cast<const uint64_t*>(t->data_ptr<int64_t>());
}

void gumbel_sample(torch::Tensor out, torch::Tensor logits, torch::Tensor inv_temp,
                   int64_t seed, c10::optional<torch::Tensor> row_seeds,
                   bool allow_fast) {
  TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kFloat32);
  TORCH_CHECK(inv_temp.dtype() == torch::kFloat32);
  const int B = logits.size(0);
  const int V = logits.size(1);
  if (B == 0) return;
  auto stream = at::cuda::getCurrentHIPStream();
  auto kern = allow_fast ? sample_kernel<true, true>
                         : sample_kernel<true, false>;
  kern<<<B, kBlock, 0, stream>>>(
      out.data_ptr<int32_t>(), logits.data_ptr<float>(),
      inv_temp.data_ptr<float>(), (uint64_t)seed, opt_seeds(row_seeds, B), V);
  HIP_CHECK_KERNEL();
}

void topkp_sample(torch::Tensor out, torch::Tensor logits,
                  torch::Tensor inv_temp, torch::Tensor top_k,
                  torch::Tensor top_p, int64_t seed,
                  c10::optional<torch::Tensor> row_seeds) {
  TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kFloat32);
  TORCH_CHECK(inv_temp.dtype() == torch::kFloat32);
  TORCH_CHECK(top_k.dtype() == torch::kInt32);
  TORCH_CHECK(top_p.dtype() == torch::kFloat32);
  const int B = logits.size(0);
  const int V = logits.size(1);
  TORCH_CHECK(top_k.numel() == B && top_p.numel() == B && inv_temp.numel() == B);
  if (B == 0) return;
  auto stream = at::cuda::getCurrentHIPStream();
  topkp_sample_kernel<<<B, kBlock, 0, stream>>>(
      out.data_ptr<int32_t>(), logits.data_ptr<float>(),
      inv_temp.data_ptr<float>(), top_k.data_ptr<int32_t>(),
      top_p.data_ptr<float>(), (uint64_t)seed, opt_seeds(row_seeds, B), V);
  HIP_CHECK_KERNEL();
}
