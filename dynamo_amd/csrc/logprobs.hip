// Fused top-N logprobs of the sampled tokens, MI355X-native.
//
// For row b with n = min(want[b], V) > 0 (want[b] == 0: the row is skipped):
//   lse         = log(sum_v exp(l[v]))
//   token_lp[b] = l[sampled[b]] - lse
//   top_*[b, 0..n-1]: the n largest entries under the sampler's total order,
//     larger logit first and the lower token id first among equal logits,
//     with logprob l[v] - lse (-inf entries have logprob -inf and come last).
// Slots >= n and skipped rows are not written. A row is taken to hold at
// least one finite entry and no NaN, as in sampling.hip.
//
// The order is the unsigned order of a 64-bit composite,
//   float_key(l) << 32 | (0xFFFFFFFF - v),
// unique per token, so every selection below is exact and tie-free.
//
// Two launches, no host sync, no [B, V] temporary, no cross-block traffic
// other than the scratch between the launches; hipGraph-capturable.
//
// Phase 1, grid (S, B): a block streams one contiguous slice of a row once
// (16-byte loads, kScanUnroll in flight per thread, scalar head and tail as in
// sampling.hip's scan_row). Every thread keeps online-softmax statistics
// (m, s) and rescales only when its max rises. The slice's top n goes through
// a threshold queue in LDS: an element whose composite exceeds the block's
// threshold (the n-th largest composite at the last flush, 0 before the
// first) is appended with one LDS add per wave (ballot + lane prefix). Between
// two flush checks the block pushes at most kStepElems elements, a flush
// leaves at most kMaxN, and a flush runs whenever count + kStepElems would
// pass kQueueCap: the queue cannot overflow whatever the input (an ascending
// row pushes everything; an all-equal row nothing after the first flush).
// A flush is an exact radix select on the composites (12-bit digits from the
// top, ending as soon as the boundary bin is taken whole), then a compaction.
//
// Phase 2, grid B: merges the S statistics (a slice with m = -inf adds 0),
// selects the top n of the S * nmax composites with the same select, ranks
// those n by counting, and writes the outputs from l[id] and l[sampled[b]].
#include "common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

constexpr int kBlock = 512;
constexpr int kWaves = kBlock / WAVE_SIZE;
constexpr int kScanUnroll = 8;   // 16-byte loads in flight per thread
constexpr int kStepVecs = 2;     // of them between two flush checks
constexpr int kStepElems = kStepVecs * 4 * kBlock;
constexpr int kMaxN = 20;
constexpr int kMaxSlices = 64;
constexpr int kQueueCap = kStepElems + 64;
constexpr int kBins = 4096;      // 12-bit digits
constexpr int kGroups = kBins / WAVE_SIZE;
constexpr int kKeep = 32;

static_assert(kQueueCap >= kStepElems + kMaxN, "queue capacity invariant");
static_assert(kQueueCap >= kMaxSlices * kMaxN, "phase 2 holds S * nmax");
static_assert(kGroups == WAVE_SIZE, "one bin group per lane of wave 0");
static_assert(kKeep >= kMaxN && kScanUnroll % kStepVecs == 0, "");

struct SelectLds {
  uint64_t q[kQueueCap];   // candidate composites
  uint64_t keep[kKeep];
  uint64_t thr;            // push only composites above this
  uint32_t hist[kBins];
  uint32_t gsum[kGroups];
  uint32_t sel[3];         // digit, entries above its bin, entries in it
  uint32_t qcnt, keepn;
};

// as sampling.hip's: a < b as floats iff key(a) < key(b) as unsigned
DEVINL uint32_t float_key(float x) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

DEVINL uint64_t composite(float x, int v) {
  return ((uint64_t)float_key(x) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)v);
}

// (m, s) += (om, os) for softmax statistics sum = s * exp(m); an empty side
// has m = -inf, s = 0 and adds nothing.
DEVINL void stat_merge(float& m, float& s, float om, float os) {
  if (om > m) {
    const float tm = m, ts = s;
    m = om; s = os; om = tm; os = ts;
  }
  if (om != -INFINITY) s += os * __expf(om - m);
}

DEVINL void stat_wave_reduce(float& m, float& s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off, WAVE_SIZE);
    const float os = __shfl_xor(s, off, WAVE_SIZE);
    stat_merge(m, s, om, os);
  }
}

// Called by a whole wave. With suffix(l) = x_l + x_(l+1) + ... + x_63, finds
// the one lane with suffix(lane + 1) < k <= suffix(lane) (1 <= k <= suffix(0))
// and returns suffix(lane + 1) in `above`.
DEVINL int suffix_pick(uint32_t x, uint32_t k, uint32_t& above) {
  const int lane = threadIdx.x & 63;
  uint32_t incl = x;
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const uint32_t t = __shfl_down(incl, off, WAVE_SIZE);
    if (lane + off < WAVE_SIZE) incl += t;
  }
  const uint32_t excl = incl - x;
  const uint64_t hit = __ballot(excl < k && k <= incl);
  const int pick = hit ? __builtin_ctzll(hit) : 0;
  above = __shfl(excl, pick, WAVE_SIZE);
  return pick;
}

// Called by the whole block after a barrier, cnt > n >= 1 uniform. Leaves the
// n largest of L.q[0, cnt) in L.q[0, n) (in no order), sets L.qcnt = n and
// L.thr to the n-th largest, and ends with a barrier. The n largest have to
// be distinct values (composites are; phase 2 pads with zeros below them).
DEVINL void block_select(SelectLds& L, int cnt, int n) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x / WAVE_SIZE;
  uint64_t prefix = 0, pmask = 0;
  uint32_t k = n;  // entries still to take among those that match prefix
  for (int pass = 0; pass < 6; pass++) {
    const int shift = pass < 5 ? 52 - 12 * pass : 0;
    const uint32_t dmask = pass < 5 ? 4095u : 15u;
    for (int i = threadIdx.x; i < kBins; i += kBlock) L.hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += kBlock) {
      const uint64_t c = L.q[i];
      if ((c & pmask) == prefix)
        atomicAdd(&L.hist[(uint32_t)(c >> shift) & dmask], 1u);
    }
    __syncthreads();
    for (int g = wid; g < kGroups; g += kWaves) {
      uint32_t s = L.hist[g * WAVE_SIZE + lane];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, WAVE_SIZE);
      if (lane == 0) L.gsum[g] = s;
    }
    __syncthreads();
    if (wid == 0) {
      // the highest digit d with count(digit >= d) >= k: group, then bin
      uint32_t above_g, above_b;
      const int g = suffix_pick(L.gsum[lane], k, above_g);
      const uint32_t h = L.hist[g * WAVE_SIZE + lane];
      const int d = suffix_pick(h, k - above_g, above_b);
      if (lane == d) {
        L.sel[0] = g * WAVE_SIZE + d;
        L.sel[1] = above_g + above_b;
        L.sel[2] = h;
      }
    }
    __syncthreads();
    k -= L.sel[1];
    prefix |= (uint64_t)L.sel[0] << shift;
    pmask |= (uint64_t)dmask << shift;
    if (L.sel[2] == k) break;  // the whole bin is taken
  }
  // exactly n entries are >= prefix
  for (int i = threadIdx.x; i < cnt; i += kBlock) {
    const uint64_t c = L.q[i];
    if (c >= prefix) {
      const uint32_t pos = atomicAdd(&L.keepn, 1u);
      if (pos < kKeep) L.keep[pos] = c;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < n) L.q[threadIdx.x] = L.keep[threadIdx.x];
  if (threadIdx.x == 0) {
    L.keepn = 0;
    L.qcnt = n;
    L.thr = prefix;
  }
  __syncthreads();
}

// Flush check, by the whole block: reduces the queue to its top n if the next
// step could overflow it (or if `force`). Barriers on both sides of the read
// of the count, so pushes may follow at once.
DEVINL void flush(SelectLds& L, int n, bool force) {
  __syncthreads();
  const int cnt = L.qcnt;
  if (cnt > n && (force || cnt + kStepElems > kQueueCap))
    block_select(L, cnt, n);
  else
    __syncthreads();
}

// Called by a whole wave: appends c of the lanes with p set.
DEVINL void push(SelectLds& L, bool p, uint64_t c) {
  const uint64_t mask = __ballot(p);
  if (mask == 0) return;
  const int lane = threadIdx.x & 63;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&L.qcnt, (uint32_t)__popcll(mask));
  base = __shfl(base, 0, WAVE_SIZE);
  if (p) {
    const uint32_t pos = base + __popcll(mask & ((1ull << lane) - 1ull));
    if (pos < kQueueCap) L.q[pos] = c;
  }
}

__global__ __launch_bounds__(kBlock) void logprobs_slice_kernel(
    float* __restrict__ stats,          // [B, S, 2]
    uint64_t* __restrict__ cand,        // [B, S, nmax]
    const float* __restrict__ logits,   // [B, V]
    const int32_t* __restrict__ want,   // [B]
    int V, int per, int nmax) {
  const int s = blockIdx.x, b = blockIdx.y, S = gridDim.x;
  const int w = want[b];
  if (w <= 0) return;
  const int n = min(w, nmax);
  __shared__ SelectLds L;
  __shared__ float red_m[kWaves], red_s[kWaves];
  if (threadIdx.x == 0) { L.qcnt = 0; L.keepn = 0; L.thr = 0; }

  const int v0 = (int)min((int64_t)V, (int64_t)s * per);
  const int len = (int)min((int64_t)V, (int64_t)s * per + per) - v0;
  const float* p = logits + (int64_t)b * V + v0;
  const int mis = (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
  const int head = min(len, (4 - mis) & 3);
  const int n4 = (len - head) / 4;
  const float4v* p4 = reinterpret_cast<const float4v*>(p + head);

  float m = -INFINITY, sum = 0.f;
  uint64_t thr = 0;
  // every lane of the wave calls this; only valid ones contribute
  auto take = [&](float x, int v, bool valid) {
    if (valid) {
      if (x > m) {
        sum = sum * __expf(m - x) + 1.f;
        m = x;
      } else if (x != -INFINITY) {
        sum += __expf(x - m);
      }
    }
    const uint64_t c = composite(x, v);
    push(L, valid && c > thr, c);
  };

  for (int i0 = 0; i0 < n4; i0 += kScanUnroll * kBlock) {
    float4v r[kScanUnroll];
#pragma unroll
    for (int u = 0; u < kScanUnroll; u++) {
      const int i = i0 + u * kBlock + threadIdx.x;
      r[u] = i < n4 ? p4[i] : float4v{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int h = 0; h < kScanUnroll / kStepVecs; h++) {
      if (i0 + h * kStepVecs * kBlock < n4) {  // uniform
        flush(L, n, false);
        thr = L.thr;
#pragma unroll
        for (int uu = 0; uu < kStepVecs; uu++) {
          const int u = h * kStepVecs + uu;
          const int i = i0 + u * kBlock + threadIdx.x;
#pragma unroll
          for (int e = 0; e < 4; e++)
            take(r[u][e], v0 + head + i * 4 + e, i < n4);
        }
      }
    }
  }
  // scalar head and tail: at most 3 elements each
  flush(L, n, false);
  thr = L.thr;
  {
    const bool valid = (int)threadIdx.x < head;
    take(valid ? p[threadIdx.x] : 0.f, v0 + threadIdx.x, valid);
    const int t = head + n4 * 4 + threadIdx.x;
    const bool tvalid = t < len;
    take(tvalid ? p[t] : 0.f, v0 + t, tvalid);
  }
  flush(L, n, true);

  const int cnt = L.qcnt;  // <= n
  if ((int)threadIdx.x < nmax)
    cand[((int64_t)b * S + s) * nmax + threadIdx.x] =
        (int)threadIdx.x < cnt ? L.q[threadIdx.x] : 0ull;

  stat_wave_reduce(m, sum);
  const int wid = threadIdx.x / WAVE_SIZE;
  if ((threadIdx.x & 63) == 0) { red_m[wid] = m; red_s[wid] = sum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kWaves; i++) stat_merge(m, sum, red_m[i], red_s[i]);
    stats[((int64_t)b * S + s) * 2] = m;
    stats[((int64_t)b * S + s) * 2 + 1] = sum;
  }
}

__global__ __launch_bounds__(kBlock) void logprobs_merge_kernel(
    float* __restrict__ token_lp,        // [B]
    float* __restrict__ top_lp,          // [B, nmax]
    int32_t* __restrict__ top_ids,       // [B, nmax]
    const float* __restrict__ logits,    // [B, V]
    const int32_t* __restrict__ sampled, // [B]
    const int32_t* __restrict__ want,    // [B]
    const float* __restrict__ stats,     // [B, S, 2]
    const uint64_t* __restrict__ cand,   // [B, S, nmax]
    int V, int S, int nmax) {
  const int b = blockIdx.x;
  const int w = want[b];
  if (w <= 0) return;
  const int n = min(min(w, nmax), V);
  __shared__ SelectLds L;
  __shared__ double lse_s;
  const float* row = logits + (int64_t)b * V;

  const int C = S * nmax;  // <= kQueueCap
  for (int i = threadIdx.x; i < C; i += kBlock)
    L.q[i] = cand[(int64_t)b * C + i];
  if (threadIdx.x == 0) { L.qcnt = C; L.keepn = 0; L.thr = 0; }
  if (threadIdx.x < WAVE_SIZE) {
    // S <= 64 slices, one per lane; in double, which is free at this size
    float m = -INFINITY, sum = 0.f;
    if ((int)threadIdx.x < S) {
      m = stats[((int64_t)b * S + threadIdx.x) * 2];
      sum = stats[((int64_t)b * S + threadIdx.x) * 2 + 1];
    }
    const float M = wave_reduce_max(m);
    double t = m == -INFINITY ? 0.0 : (double)sum * exp((double)m - (double)M);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, WAVE_SIZE);
    if (threadIdx.x == 0) lse_s = (double)M + log(t);
  }
  __syncthreads();
  if (C > n) block_select(L, C, n);
  const double lse = lse_s;  // l - lse is rounded to fp32 once
  if ((int)threadIdx.x < n) {
    const uint64_t c = L.q[threadIdx.x];
    int rank = 0;
    for (int j = 0; j < n; j++) rank += L.q[j] > c;
    const uint32_t id = 0xFFFFFFFFu - (uint32_t)c;
    top_ids[(int64_t)b * nmax + rank] = (int32_t)id;
    top_lp[(int64_t)b * nmax + rank] =
        id < (uint32_t)V ? (float)(row[id] - lse) : __int_as_float(0x7fc00000);
  }
  if (threadIdx.x == 0) {
    // an id outside the row reads nothing and gives NaN
    const int sv = sampled[b];
    token_lp[b] = sv >= 0 && sv < V ? (float)(row[sv] - lse)
                                    : __int_as_float(0x7fc00000);
  }
}

}  // namespace

void top_logprobs(torch::Tensor token_lp, torch::Tensor top_lp,
                  torch::Tensor top_ids, torch::Tensor logits,
                  torch::Tensor sampled, torch::Tensor want,
                  torch::Tensor stats, torch::Tensor cand, int64_t nmax,
                  int64_t slices) {
  TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kFloat32 &&
              logits.dim() == 2 && logits.is_contiguous(),
              "top_logprobs: logits must be contiguous fp32 [B, V] on the GPU");
  const int64_t B = logits.size(0);
  const int64_t V = logits.size(1);
  TORCH_CHECK(1 <= nmax && nmax <= kMaxN, "top_logprobs: nmax ", nmax,
              " outside [1, ", kMaxN, "]");
  TORCH_CHECK(1 <= slices && slices <= kMaxSlices, "top_logprobs: ", slices,
              " slices outside [1, ", kMaxSlices, "]");
  // token ids (and the few past V that idle lanes form) are ints
  TORCH_CHECK(V >= 1 && V < (1ll << 31) - 8 * kStepElems && B < 65536,
              "top_logprobs: V or B out of range");
  auto ok = [&](const torch::Tensor& t, at::ScalarType dt, int64_t numel) {
    return t.is_cuda() && t.dtype() == dt && t.is_contiguous() &&
           t.numel() == numel;
  };
  TORCH_CHECK(ok(token_lp, torch::kFloat32, B) &&
              ok(top_lp, torch::kFloat32, B * nmax) &&
              ok(top_ids, torch::kInt32, B * nmax),
              "top_logprobs: outputs are fp32 [B], fp32 [B, nmax], int32 "
              "[B, nmax], contiguous");
  TORCH_CHECK(ok(sampled, torch::kInt32, B) && ok(want, torch::kInt32, B),
              "top_logprobs: sampled and want are contiguous int32 [B]");
  TORCH_CHECK(ok(stats, torch::kFloat32, B * slices * 2) &&
              ok(cand, torch::kInt64, B * slices * nmax),
              "top_logprobs: scratch is fp32 [B, S, 2] and int64 [B, S, nmax]");
  if (B == 0) return;
  const int S = (int)slices;
  // slice length: a multiple of 4, so every slice of an aligned row is
  const int per = (int)(((V + S - 1) / S + 3) / 4 * 4);
  auto stream = at::cuda::getCurrentHIPStream();
  uint64_t* cp = reinterpret_cast<uint64_t*>(cand.data_ptr<int64_t>());
  logprobs_slice_kernel<<<dim3(S, (unsigned)B), kBlock, 0, stream>>>(
      stats.data_ptr<float>(), cp, logits.data_ptr<float>(),
      want.data_ptr<int32_t>(), (int)V, per, (int)nmax);
  HIP_CHECK_KERNEL();
  logprobs_merge_kernel<<<(unsigned)B, kBlock, 0, stream>>>(
      token_lp.data_ptr<float>(), top_lp.data_ptr<float>(),
      top_ids.data_ptr<int32_t>(), logits.data_ptr<float>(),
      sampled.data_ptr<int32_t>(), want.data_ptr<int32_t>(),
      stats.data_ptr<float>(), cp, (int)V, S, (int)nmax);
  HIP_CHECK_KERNEL();
}
