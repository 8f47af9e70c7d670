// Skinny-M (decode-regime) GEMM sweep for MI355X/gfx950.
//
// y[M<=16, N] = x[M, K] @ W[N, K]^T, bf16 in / bf16 out, fp32 accum.
// At decode M=conc (16): the GEMM is pure W-streaming. In the decode step
// every W byte is read once per step (137 GB of weights pass between two
// uses of a matrix), so the rate that matters is the COLD one: each timed
// launch rotates over R distinct copies of W with R * bytes(W) >= 1 GiB and
// never touches the buffer of the launch before it. The same-buffer ("hot")
// rate is printed next to it; for the o / qkv shapes (134 / 168 MB) it is an
// Infinity-Cache figure the step never sees. The hipBLASLt baseline in the
// same two cache states is benchmarks/gemm_probe.py.
//
// Design (the kernel is dynamo_amd/csrc/skinny_gemm_impl.h, shared with the
// production binding dynamo_amd/csrc/skinny_gemm.hip):
//   mfma_f32_16x16x32_bf16 with A = x, B = W^T. Per-lane operand layout
//   (lr = lane&15, lg = lane>>4):
//     A-frag: x[lr][k0 + lg*8 .. +8]        -> one b128 load, contiguous K
//     B-frag: W[n0 + lr][k0 + lg*8 .. +8]   -> one b128 load, contiguous K
//   i.e. BOTH operands come straight from global as 16B loads - no LDS
//   staging, no transpose, no swizzle. Each wave owns one (or NT) 16-col
//   N-tiles and a K/WPB slice; the WPB waves of a block LDS-reduce their
//   fp32 accumulators and wave 0 writes bf16.
//
// "COAL" rows are the kernel's Bf16Coal format, the row-coalesced one that
// production runs (8 rows x 128 B per load + ds_bpermute; its U counts 64-k
// steps), "FP8" rows its Fp8Coal format (W8A16, U counts 128-k steps), "MXFP4"
// rows its Mxfp4Coal format (W4A16, U counts 256-k steps, M <= 32). The
// LDS-staged, persistent and ceiling kernels below are the round-2
// experiments, same-buffer only.
//
// Each (WPB, U, NT) point runs with default-policy W loads ("d") and with
// non-temporal ones ("nt"); x is always on the default policy.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I dynamo_amd/csrc \
//          benchmarks/skinny_sweep.hip -o benchmarks/skinny_sweep
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>

#include "skinny_gemm_impl.h"

using skinny::skinny_gemm_kernel;
using skinny::Bf16Plain;  // the register-streaming format
using skinny::Bf16Coal;
using skinny::Fp8Coal;
using skinny::Mxfp4Coal;

// LDS-staged skinny GEMM: one 16-col n-tile per block, 4 waves. W tiles
// (16 rows x KC cols) are staged cooperatively with fully-linear 1KB
// bursts per wave-instruction (the 6.3 TB/s pattern), then each wave
// mfma-consumes a quarter of the k-chunk from XOR-swizzled LDS. Double-
// buffered: loads for chunk i+1 are in flight while chunk i computes.
template <int KC>  // k elems per staged chunk (KC % 512 == 0)
__global__ __launch_bounds__(256) void skinny_gemm_lds_kernel(
    const short* __restrict__ x, const short* __restrict__ w,
    short* __restrict__ y, int M, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int lr = lane & 15;
  const int lg = lane >> 4;
  const int n0 = blockIdx.x * 16;
  if (n0 >= N) return;

  // LDS: double buffer of 16 rows x KC*2 bytes, XOR-swizzled in 16B units
  constexpr int ROWB = KC * 2;             // bytes per row
  __shared__ char wbuf[2][16 * ROWB];
  __shared__ f32x4 red[3 * 64];

  const int ar = lr < M ? lr : 0;
  const int kw = KC / 4;                    // k elems per wave per chunk
  const int mf = kw / 32;                   // mfmas per wave per chunk
  const int nchunks = K / KC;

  // staging geometry: round r stages rows {4r..4r+3}; wave w stages row
  // 4r + w as ONE contiguous 1KB+ burst (64 lanes x 16B x (ROWB/1024)).
  constexpr int LPR = ROWB / 1024;          // 1KB bursts per row
  const int srow0 = wid;                    // wave stages rows wid, wid+4, ..
  f32x4 acc{0.f, 0.f, 0.f, 0.f};

  bf16x8 sreg[4 * LPR];                     // staged-load regs (4 rows/wave)
  bf16x8 areg[16];                          // A prefetch (mf <= 16)

  auto issue_stage = [&](int c) {
#pragma unroll
    for (int rr = 0; rr < 4; rr++)
#pragma unroll
      for (int l = 0; l < LPR; l++) {
        const int row = srow0 + rr * 4;
        const int col = n0 + row;
        const short* src = w + (size_t)(col < N ? col : N - 1) * K + c * KC +
                           (l * 64 + lane) * 8;
        sreg[rr * LPR + l] = *reinterpret_cast<const bf16x8*>(src);
      }
  };
  auto issue_a = [&](int c) {
#pragma unroll
    for (int u = 0; u < 16; u++)
      if (u < mf)
        areg[u] = *reinterpret_cast<const bf16x8*>(
            x + (size_t)ar * K + c * KC + wid * kw + u * 32 + lg * 8);
  };
  auto write_stage = [&](int buf) {
#pragma unroll
    for (int rr = 0; rr < 4; rr++)
#pragma unroll
      for (int l = 0; l < LPR; l++) {
        const int row = srow0 + rr * 4;
        const int boff = (l * 64 + lane) * 16;
        *reinterpret_cast<bf16x8*>(
            &wbuf[buf][row * ROWB + (boff ^ ((row & 7) << 4))]) =
            sreg[rr * LPR + l];
      }
  };
  auto compute = [&](int buf, bf16x8* a) {
#pragma unroll
    for (int u = 0; u < 16; u++) {
      if (u >= mf) break;
      const int fo = (wid * kw + u * 32 + lg * 8) * 2;  // byte col in row
      bf16x8 b = *reinterpret_cast<const bf16x8*>(
          &wbuf[buf][lr * ROWB + (fo ^ ((lr & 7) << 4))]);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b, acc, 0, 0, 0);
    }
  };

  issue_stage(0);
  issue_a(0);
  write_stage(0);
  bf16x8 acur[16];
#pragma unroll
  for (int u = 0; u < 16; u++) acur[u] = areg[u];
  for (int c = 1; c < nchunks; c++) {
    issue_stage(c);        // loads for next chunk in flight
    issue_a(c);
    __syncthreads();       // wbuf[(c-1)&1] fully written
    compute((c - 1) & 1, acur);
#pragma unroll
    for (int u = 0; u < 16; u++) acur[u] = areg[u];
    __syncthreads();       // all reads of wbuf[c&1] from chunk c-2 done
    write_stage(c & 1);
  }
  __syncthreads();
  compute((nchunks - 1) & 1, acur);

  // cross-wave reduce + write
  if (wid > 0) red[(wid - 1) * 64 + lane] = acc;
  __syncthreads();
  if (wid != 0) return;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    f32x4 o = red[r * 64 + lane];
    acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
  }
  const int col = n0 + lr;
  if (col >= N) return;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int row = lg * 4 + i;
    if (row < M) y[(size_t)row * N + col] = f32_to_bf16(acc[i]);
  }
}

// Contiguity ceilings: how fast can W stream with larger per-row bursts?
// MODE 0: 16 rows x 64B per instruction (the mfma B-frag native pattern)
// MODE 1: 8 rows x 128B per instruction
// MODE 2: fully linear 1KB per instruction (absolute HBM read peak)
template <int MODE>
__global__ __launch_bounds__(256) void stream_ceiling2_kernel(
    const short* __restrict__ w, short* __restrict__ y, long total_elems) {
  const int lane = threadIdx.x & 63;
  const long wavei = (long)(blockIdx.x * 4 + (threadIdx.x >> 6));
  const long nwaves = (long)gridDim.x * 4;
  f32x4 acc{0.f, 0.f, 0.f, 0.f};
  // W is viewed as R rows x 4096 elems (8 KB rows). Each wave step reads
  // 4096 elems (8 instrs x 64 lanes x 16B); MODE picks the shape of that
  // footprint: 16 rows x 512B, 8 rows x 1KB, or linear 8KB.
  const long chunk = 4096;
  const long nchunks = total_elems / chunk;
  for (long g = wavei; g < nchunks; g += nwaves) {
    bf16x8 b[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      long off;
      if (MODE == 2) {
        off = g * chunk + (u * 64 + lane) * 8;
      } else if (MODE == 1) {
        const long rowbase = (g / 8) * 8, cb = g % 8;
        off = (rowbase + (lane >> 3)) * 4096 + cb * 512 + u * 64 +
              (lane & 7) * 8;
      } else {
        const long rowbase = (g / 16) * 16, cb = g % 16;
        off = (rowbase + (lane >> 2)) * 4096 + cb * 256 + u * 32 +
              (lane & 3) * 8;
      }
      b[u] = *reinterpret_cast<const bf16x8*>(w + off);
    }
#pragma unroll
    for (int u = 0; u < 8; u++)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[u], b[u], acc, 0, 0, 0);
  }
  if (acc.x == 1e30f) y[lane] = f32_to_bf16(acc.x);
}

// Persistent variant: grid is pinned near 1 WG/CU (256); each block loops
// over n-tile groups. The o-shape ceiling run showed the 16-rows-x-64B
// pattern streams at 6.9 TB/s when exactly 256 blocks are resident but
// drops to ~5.2-5.5 with thousands of interleaved blocks (DRAM stream
// thrash) - so bound the resident streams, not the work per block.
template <int WPB, int U, int NT>
__global__ __launch_bounds__(WPB * 64) void skinny_gemm_ps_kernel(
    const short* __restrict__ x, const short* __restrict__ w,
    short* __restrict__ y, int M, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int lr = lane & 15;
  const int lg = lane >> 4;
  const int kw = K / WPB;
  const int k0 = wid * kw;
  const int steps = kw / 32;
  const int ar = lr < M ? lr : 0;
  const short* xp = x + (size_t)ar * K + k0 + lg * 8;
  const int ngroups = (N + NT * 16 - 1) / (NT * 16);
  __shared__ f32x4 red[WPB > 1 ? (WPB - 1) * NT * 64 : 1];

  for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int n0 = g * NT * 16;
    const short* wp[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const int col = n0 + t * 16 + lr;
      wp[t] = w + (size_t)(col < N ? col : N - 1) * K + k0 + lg * 8;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 abuf[U];
    bf16x8 bbuf[NT][U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      abuf[u] = *reinterpret_cast<const bf16x8*>(xp + u * 32);
#pragma unroll
      for (int t = 0; t < NT; t++)
        bbuf[t][u] = *reinterpret_cast<const bf16x8*>(wp[t] + u * 32);
    }
    for (int ss = U; ss < steps; ss += U) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        bf16x8 a = abuf[u];
        abuf[u] = *reinterpret_cast<const bf16x8*>(xp + (ss + u) * 32);
#pragma unroll
        for (int t = 0; t < NT; t++) {
          bf16x8 b = bbuf[t][u];
          bbuf[t][u] = *reinterpret_cast<const bf16x8*>(wp[t] + (ss + u) * 32);
          acc[t] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int t = 0; t < NT; t++)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(abuf[u], bbuf[t][u],
                                                         acc[t], 0, 0, 0);
    if (WPB > 1) {
      if (g != blockIdx.x) __syncthreads();  // red[] reuse across groups
      if (wid > 0) {
#pragma unroll
        for (int t = 0; t < NT; t++)
          red[((wid - 1) * NT + t) * 64 + lane] = acc[t];
      }
      __syncthreads();
      if (wid == 0) {
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
          for (int r = 0; r < WPB - 1; r++) {
            f32x4 o = red[(r * NT + t) * 64 + lane];
            acc[t].x += o.x; acc[t].y += o.y; acc[t].z += o.z;
            acc[t].w += o.w;
          }
      }
    }
    if (wid == 0) {
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int col = n0 + t * 16 + lr;
        if (col >= N) break;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int row = lg * 4 + i;
          if (row < M) y[(size_t)row * N + col] = f32_to_bf16(acc[t][i]);
        }
      }
    }
  }
}

// Streaming ceiling for the same access pattern: b128 loads of 16 W rows
// per instruction, results discarded (kept live via a dummy accumulate).
template <int U, int NT>
__global__ __launch_bounds__(256) void stream_ceiling_kernel(
    const short* __restrict__ x, const short* __restrict__ w,
    short* __restrict__ y, int M, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int lr = lane & 15;
  const int n0 = (blockIdx.x * NT) * 16;
  if (n0 >= N) return;
  const int kw = K / 4, k0 = wid * kw, steps = kw / 32;
  const short* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; t++)
    wp[t] = w + (size_t)(n0 + t * 16 + lr) * K + k0 + (lane >> 4) * 8;
  f32x4 acc{0.f, 0.f, 0.f, 0.f};
  bf16x8 bbuf[NT][U];
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int t = 0; t < NT; t++)
      bbuf[t][u] = *reinterpret_cast<const bf16x8*>(wp[t] + u * 32);
  for (int s = U; s < steps; s += U) {
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int t = 0; t < NT; t++) {
        bf16x8 b = bbuf[t][u];
        bbuf[t][u] = *reinterpret_cast<const bf16x8*>(wp[t] + (s + u) * 32);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, b, acc, 0, 0, 0);
      }
  }
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int t = 0; t < NT; t++)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bbuf[t][u], bbuf[t][u],
                                                    acc, 0, 0, 0);
  if (acc.x == 1e30f) y[lane] = f32_to_bf16(acc.x);
}

// ---------------------------------------------------------------------------
// Times kern(x, W copy, rest...): launch i reads W copy i % R, the copies
// being `stride` elements apart.
template <class Kern, class W, class... Rest>
static double bench(Kern kern, int grid, int block, int iters, int R,
                    size_t stride, const short* x, const W* w, Rest... rest) {
  for (int i = 0; i < 5; i++)
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, 0, x,
                       w + (i % R) * stride, rest...);
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  hipEventRecord(a);
  for (int i = 0; i < iters; i++)
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, 0, x,
                       w + ((i + 5) % R) * stride, rest...);
  hipEventRecord(b);
  hipEventSynchronize(b);
  float ms;
  hipEventElapsedTime(&ms, a, b);
  hipEventDestroy(a);
  hipEventDestroy(b);
  return ms * 1e3 / iters;  // us
}

static short f2b(float f) {
  unsigned u;
  __builtin_memcpy(&u, &f, 4);
  return (short)(u >> 16);
}
static float b2f(short s) {
  unsigned u = (unsigned)(unsigned short)s << 16;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

struct Shape { const char* name; int K, N; };

int main(int argc, char** argv) {
  // the bf16 kernels use the first 16 rows; the FP8 rows run M up to 64
  const int M = std::min(argc > 1 ? atoi(argv[1]) : 16, 64);
  Shape shapes[] = {
      {"qkv   ", 8192, 10240},  {"o     ", 8192, 8192},
      {"gateup", 8192, 57344},  {"down  ", 28672, 8192},
      {"lmhead", 8192, 128256},
  };
  const int maxK = 28672, maxN = 128256;
  std::vector<short> hx(64 * maxK), hw((size_t)1 << 25);
  srand(7);
  for (auto& v : hx) v = f2b((rand() % 2000 - 1000) / 1000.f);
  for (auto& v : hw) v = f2b((rand() % 2000 - 1000) / 1000.f);
  short *x, *w, *y;
  hipMalloc(&x, hx.size() * 2);
  // big W: replicate the host block (content irrelevant for timing; the
  // first 64 MB is real for numerics checks)
  // (also the pool for the cold rotation: the largest need is 2 lm_head
  // copies = 4.2 GB)
  size_t welems = (size_t)maxN * maxK;
  hipMalloc(&w, welems * 2);
  for (size_t off = 0; off < welems; off += hw.size()) {
    size_t n = std::min(hw.size(), welems - off);
    hipMemcpy(w + off, hw.data(), n * 2, hipMemcpyHostToDevice);
  }
  hipMemcpy(x, hx.data(), hx.size() * 2, hipMemcpyHostToDevice);
  hipMalloc(&y, (size_t)64 * maxN * 2);
  float* wscale;
  {
    std::vector<float> hs(maxN, 1.f / 448);
    hipMalloc(&wscale, hs.size() * 4);
    hipMemcpy(wscale, hs.data(), hs.size() * 4, hipMemcpyHostToDevice);
  }

  unsigned char* mxscale;   // e8m0 2^0 for every block of the largest shape
  hipMalloc(&mxscale, (size_t)maxN * 8192 / 32);
  hipMemset(mxscale, 127, (size_t)maxN * 8192 / 32);

  // numerics check on a small shape
  {
    const int cK = 512, cN = 64;
    std::vector<short> hy(M * cN);
    std::vector<short> cx(M * cK);
    for (int m = 0; m < M; m++)
      for (int k = 0; k < cK; k++) cx[m * cK + k] = hx[m * maxK + k];
    short* xd2;
    hipMalloc(&xd2, cx.size() * 2);
    hipMemcpy(xd2, cx.data(), cx.size() * 2, hipMemcpyHostToDevice);
    const float* noscale = nullptr;
    hipLaunchKernelGGL((skinny_gemm_kernel<Bf16Plain, 4, 4, 2, 1, 1>),
                       dim3(cN / 32), dim3(256), 0, 0, xd2, w, noscale, y, M,
                       cN, cK);
    hipMemcpy(hy.data(), y, hy.size() * 2, hipMemcpyDeviceToHost);
    double maxerr = 0;
    for (int m = 0; m < M; m++)
      for (int n = 0; n < cN; n++) {
        double ref = 0;
        for (int k = 0; k < cK; k++)
          ref += (double)b2f(cx[m * cK + k]) * b2f(hw[(size_t)n * cK + k]);
        double got = b2f(hy[m * cN + n]);
        double err = std::abs(got - ref) / std::max(1.0, std::abs(ref));
        maxerr = std::max(maxerr, err);
      }
    printf("numerics (K=%d N=%d WPB4 U4 NT2 nt): maxrelerr=%.4f %s\n", cK, cN,
           maxerr, maxerr < 0.02 ? "PASS" : "FAIL");
    hipLaunchKernelGGL((skinny_gemm_lds_kernel<512>), dim3(cN / 16),
                       dim3(256), 0, 0, xd2, w, y, M, cN, cK);
    hipMemcpy(hy.data(), y, hy.size() * 2, hipMemcpyDeviceToHost);
    maxerr = 0;
    for (int m = 0; m < M; m++)
      for (int n = 0; n < cN; n++) {
        double ref = 0;
        for (int k = 0; k < cK; k++)
          ref += (double)b2f(cx[m * cK + k]) * b2f(hw[(size_t)n * cK + k]);
        double got = b2f(hy[m * cN + n]);
        double err = std::abs(got - ref) / std::max(1.0, std::abs(ref));
        maxerr = std::max(maxerr, err);
      }
    {
      // the row-coalesced format must reproduce the register-streaming one
      // bit for bit at equal WPB
      std::vector<short> h0(M * cN), h1(M * cN);
      hipLaunchKernelGGL((skinny_gemm_kernel<Bf16Plain, 4, 4, 2, 1, 0>),
                         dim3(cN / 32), dim3(256), 0, 0, xd2, w, noscale, y,
                         M, cN, cK);
      hipMemcpy(h0.data(), y, h0.size() * 2, hipMemcpyDeviceToHost);
      hipLaunchKernelGGL((skinny_gemm_kernel<Bf16Coal, 4, 2, 2, 1, 0>),
                         dim3(cN / 32), dim3(256), 0, 0, xd2, w, noscale, y,
                         M, cN, cK);
      hipMemcpy(h1.data(), y, h1.size() * 2, hipMemcpyDeviceToHost);
      printf("coalesced vs register kernel (WPB4): %s\n",
             h0 == h1 ? "bit-identical PASS" : "DIFFERENT FAIL");
    }
    printf("numerics LDS kc512: maxrelerr=%.4f %s\n", maxerr,
           maxerr < 0.02 ? "PASS" : "FAIL");
    hipFree(xd2);
  }

  const int iters = 30;
  for (auto& s : shapes) {
    // compact x for this K
    std::vector<short> cx(16 * s.K);
    for (int m = 0; m < 16; m++)
      for (int k = 0; k < s.K; k++) cx[m * s.K + k] = hx[m * maxK + (k % maxK)];
    hipMemcpy(x, cx.data(), cx.size() * 2, hipMemcpyHostToDevice);
    double gb = (double)s.N * s.K * 2 / 1e9;
    printf("%s K=%6d N=%6d:", s.name, s.K, s.N);
    // rate of format F over RR copies of W (bytes GB each, at WP)
#define RATE(F, WPB, U, NT, MT, NTL, GB, WP, SCALE, RR)                     \
  (GB / bench(skinny_gemm_kernel<F, WPB, U, NT, MT, NTL>,                   \
              (s.N + NT * 16 - 1) / (NT * 16), WPB * 64, iters, RR,         \
              (size_t)s.N * s.K / F::WPACK, x, WP,                          \
              (const typename F::scale_t*)SCALE, y, M, s.N, s.K) * 1e3)
#define RUN1(WPB, U, NT, NTL, RR)                                           \
  RATE(Bf16Plain, WPB, U, NT, 1, NTL, gb, w, nullptr, RR)
#define RUN(WPB, U, NT)                                                     \
  {                                                                         \
    double hd = RUN1(WPB, U, NT, 0, 1), hn = RUN1(WPB, U, NT, 1, 1);        \
    double cd = RUN1(WPB, U, NT, 0, R), cn = RUN1(WPB, U, NT, 1, R);        \
    printf("\n    w%du%dn%d  hot d %5.2f nt %5.2f | cold d %5.2f nt %5.2f "  \
           "TB/s (%6.1f us)", WPB, U, NT, hd, hn, cd, cn, gb / cn * 1e3);   \
  }
    // R copies of W: at least 1 GiB in rotation, never the same buffer twice
    const size_t wbytes = (size_t)s.N * s.K * 2;
    const int R = (int)std::max<size_t>(2, (((size_t)1 << 30) + wbytes - 1) / wbytes);
    printf(" R=%d", R);
    SKINNY_GEMM_CONFIGS(RUN)
#undef RUN
#undef RUN1
    // row-coalesced loads + ds_bpermute (U2 counts 64-k steps)
#define RUNQ1(WPB, U2, NT, NTL, RR)                                         \
  RATE(Bf16Coal, WPB, U2, NT, 1, NTL, gb, w, nullptr, RR)
#define RUNQ(WPB, U2, NT)                                                   \
  {                                                                         \
    double hd = RUNQ1(WPB, U2, NT, 0, 1), hn = RUNQ1(WPB, U2, NT, 1, 1);    \
    double cd = RUNQ1(WPB, U2, NT, 0, R), cn = RUNQ1(WPB, U2, NT, 1, R);    \
    printf("\n    COAL w%du%dn%d  hot d %5.2f nt %5.2f | cold d %5.2f nt "   \
           "%5.2f TB/s (%6.1f us)", WPB, U2, NT, hd, hn, cd, cn,            \
           gb / cd * 1e3);                                                  \
  }
    RUNQ(4, 2, 2) RUNQ(8, 2, 2) RUNQ(8, 1, 4) RUNQ(8, 2, 4) RUNQ(4, 2, 4)
    RUNQ(8, 4, 2) RUNQ(2, 2, 4) RUNQ(2, 2, 8) RUNQ(4, 1, 8) RUNQ(8, 1, 2)
    // no K split: one wave sums all of K in order (bit-identical to the
    // library's gate/up kernel)
    RUNQ(1, 4, 2) RUNQ(1, 2, 4) RUNQ(1, 4, 4) RUNQ(1, 8, 2) RUNQ(1, 2, 2)
    RUNQ(1, 1, 8) RUNQ(1, 2, 8)
#undef RUNQ
#undef RUNQ1
    // W8A16 (Fp8Coal): the same pool read as e4m3 bytes, nt W loads,
    // cold over R8 copies (R8 * bytes >= 1 GiB); TB/s are of the e4m3 W.
    // Timing only: arbitrary bytes include the NaN codes.
    {
      const size_t w8bytes = (size_t)s.N * s.K;
      const int R8 = (int)std::max<size_t>(
          2, (((size_t)1 << 30) + w8bytes - 1) / w8bytes);
      const double gb8 = (double)w8bytes / 1e9;
      printf("\n    FP8 R=%d", R8);
#define RUNF1(WPB, U, NT, MT, RR)                                           \
  RATE(Fp8Coal, WPB, U, NT, MT, 1, gb8, (const unsigned char*)w, wscale, RR)
#define RUNF(WPB, U, NT)                                                    \
  if (s.K % (WPB * 128 * U) == 0) {                                         \
    double h = M <= 16 ? RUNF1(WPB, U, NT, 1, 1) : RUNF1(WPB, U, NT, 4, 1); \
    double c = M <= 16 ? RUNF1(WPB, U, NT, 1, R8)                           \
                       : RUNF1(WPB, U, NT, 4, R8);                          \
    printf("\n    FP8 w%du%dn%d  hot %5.2f | cold %5.2f TB/s (%6.1f us)",    \
           WPB, U, NT, h, c, gb8 / c * 1e3);                                \
  }
      FP8_GEMM_CONFIGS(RUNF)
#undef RUNF
#undef RUNF1
    }
    // W4A16 (Mxfp4Coal): the same pool read as packed e2m1 bytes, nt W
    // loads, cold over R4 copies (R4 * bytes >= 1 GiB); TB/s are of the
    // packed W plus its scales. The scales (all 2^0) are one buffer, not
    // rotated: 1/17 of the bytes. Timing only.
    if (M <= 16 * MXFP4_GEMM_MAX_MT) {
      const size_t w4bytes = (size_t)s.N * s.K / 2;
      const int R4 = (int)std::max<size_t>(
          2, (((size_t)1 << 30) + w4bytes - 1) / w4bytes);
      const double gb4 = (double)(w4bytes + w4bytes / 16) / 1e9;
      printf("\n    MXFP4 R=%d", R4);
#define RUNM1(WPB, U, NT, MT, RR)                                           \
  RATE(Mxfp4Coal, WPB, U, NT, MT, 1, gb4, (const unsigned char*)w, mxscale, \
       RR)
#define RUNM(WPB, U, NT)                                                    \
  if (s.K % (WPB * 256 * U) == 0) {                                         \
    double h = M <= 16 ? RUNM1(WPB, U, NT, 1, 1) : RUNM1(WPB, U, NT, 2, 1); \
    double c = M <= 16 ? RUNM1(WPB, U, NT, 1, R4)                           \
                       : RUNM1(WPB, U, NT, 2, R4);                          \
    printf("\n    MXFP4 w%du%dn%d  hot %5.2f | cold %5.2f TB/s (%6.1f us)",  \
           WPB, U, NT, h, c, gb4 / c * 1e3);                                \
  }
      MXFP4_GEMM_CONFIGS(RUNM)
#undef RUNM
#undef RUNM1
    }
#undef RATE
    printf("\n        ");
    #define RUNC(U, NT)                                                         \
  {                                                                         \
    double us = bench(stream_ceiling_kernel<U, NT>,                         \
                      (s.N + NT * 16 - 1) / (NT * 16), 256, iters, 1, 0, x, \
                      w, y, M, s.N, s.K);                                   \
    printf("  CEIL u%dn%d %6.1fus %5.2fTB/s", U, NT, us, gb / us * 1e3);    \
  }
    RUNC(4, 2) RUNC(4, 4) RUNC(8, 4)
#undef RUNC
    printf("\n        ");
#define RUNP(WPB, U, NT, GRID)                                              \
  {                                                                         \
    int ng = (s.N + NT * 16 - 1) / (NT * 16);                               \
    double us = bench(skinny_gemm_ps_kernel<WPB, U, NT>,                    \
                      std::min(GRID, ng), WPB * 64, iters, 1, 0, x, w, y,   \
                      M, s.N, s.K);                                         \
    printf("  PS w%du%dn%d g%d %6.1fus %5.2fTB/s", WPB, U, NT, GRID, us,    \
           gb / us * 1e3);                                                  \
  }
    RUNP(4, 4, 2, 256) RUNP(4, 4, 2, 512)
#undef RUNP
#define RUNL(KC)                                                            \
  {                                                                         \
    double us = bench(skinny_gemm_lds_kernel<KC>, s.N / 16, 256, iters, 1,  \
                      0, x, w, y, M, s.N, s.K);                             \
    printf("  LDS kc%d %6.1fus %5.2fTB/s", KC, us, gb / us * 1e3);          \
  }
    RUNL(512) RUNL(1024) RUNL(2048)
#undef RUNL
    printf("\n");
  }
  {
    long total = (long)maxN * maxK;  // 3.7G elems = 7.35 GB
    double gb = total * 2 / 1e9;
#define RUNC2(MODE, GRID)                                                   \
  {                                                                         \
    for (int i = 0; i < 2; i++)                                             \
      hipLaunchKernelGGL(stream_ceiling2_kernel<MODE>, dim3(GRID),          \
                         dim3(256), 0, 0, w, y, total);                     \
    hipEvent_t a, b;                                                        \
    hipEventCreate(&a); hipEventCreate(&b);                                 \
    hipEventRecord(a);                                                      \
    for (int i = 0; i < 8; i++)                                             \
      hipLaunchKernelGGL(stream_ceiling2_kernel<MODE>, dim3(GRID),          \
                         dim3(256), 0, 0, w, y, total);                     \
    hipEventRecord(b); hipEventSynchronize(b);                              \
    float ms; hipEventElapsedTime(&ms, a, b);                               \
    printf("CEIL2 mode%d g%d: %8.1f us  %5.2f TB/s\n", MODE, GRID,         \
           ms * 1e3 / 8, gb / (ms / 8));                                    \
    hipEventDestroy(a); hipEventDestroy(b);                                 \
  }
    RUNC2(0, 256) RUNC2(1, 256) RUNC2(2, 256)
    RUNC2(0, 512) RUNC2(1, 512) RUNC2(2, 512)
#undef RUNC2
  }
  hipFree(x); hipFree(w); hipFree(y); hipFree(wscale); hipFree(mxscale);
  return 0;
}
