// Shared-prefix paged decode attention: decode rows whose page tables begin
// with the same physical pages (a common system prompt under the prefix
// cache) stream those pages once.
//
// The d-major decode kernel (paged_decode_mfma_swapped_dmajor) runs one
// workgroup per (sequence, kv head, chunk): sixteen rows that share 6k
// tokens read those 6k tokens of K and V sixteen times, and at G = 8 half of
// the 16 MFMA columns are padding. Here the grid is (W, Hkv, C) over WORK
// ITEMS. An item is a list of batch rows and a token range:
//   item_rows  [W, R] int32   rows whose queries ride the item's columns,
//                             R = 64 / G, padded with -1; item_rows[w, 0] ==
//                             -1 is an unused item (every block exits)
//   item_range [W, 2] int32   (t_begin, t_end), walked through the page
//                             table row of item_rows[w, 0]; t_end == -1 is
//                             ctx_lens[item_rows[w, 0]], read here, so a
//                             row's own tail grows without a new plan
// The members' query heads are folded onto the MFMA columns beside the GQA
// group, as attention_multiquery.hip folds a query run:
//   column = m * G + g      member m, group head g < G
// zero-padded to 16 * CT columns, CT in {1, 2, 4}. The token side is the
// decode kernel's: 4 waves each walking a chunk/4 slab in 64-token tiles, K
// in contiguous 1 KB bursts through the wave's XOR-swizzled LDS region, V^T
// fragments as direct b128 loads from the d-major pages, wave-local barriers
// only. Each K and V fragment is loaded once per tile and feeds CT MFMAs;
// each column tile keeps its own (m_run, l_run, acc[8]).
//
// There is no causal limit: every column of an item sees the same tokens,
// t < min(t_end, slab_end). Tiles wholly below that take the unmasked path.
//
// The block of chunk c covers [c * chunk, (c + 1) * chunk) of the item's
// range and exits without writing when t_begin > c * chunk or t_end <=
// c * chunk (t_begin is a multiple of chunk). Otherwise every member row
// gets partial[row, head, c, :] and ml[row, head, c, :]; the chunk merge
// paged_decode_phase2 over ctx_lens always follows, also with one chunk, so
// a pad row (ctx 0) comes out as zeros from there.
//
// What the plan (ops.shared_prefix_plan) guarantees and this kernel relies
// on: every slot (row, c) with c * chunk < ctx_row is written by exactly one
// item. A group's shared length is a multiple of chunk; its prefix item
// (members = the group, range [0, prefix_len)) writes the chunks below
// prefix_len / chunk, each member's own item ([prefix_len, -1)) the rest; an
// ungrouped row is one item [0, -1).
//
// Registers (gfx950 resource-usage report, VGPRs + AGPRs of the 512 a
// 256-thread block may use; scratch is 0 bytes in every instantiation, one
// wave per SIMD like the multi-query kernel):
//   <bf16, 1> 214 + 48    <bf16, 2> 256 + 112    <bf16, 4> 256 + 236
//   <fp8,  1> 230 + 48    <fp8,  2> 256 + 114    <fp8,  4> 256 + 232
// CT = 1 and 2 keep the Q fragments in VGPRs; CT = 4 reads them from LDS at
// each use and runs QK / softmax / PV in two passes of two column tiles over
// the 64-token K tile, which stays whole in the wave's LDS region (16 KB).
//
// LDS: Q [16*CT][hd] bf16 and the four per-wave K regions while the slabs
// are walked (68 / 72 / 80 KB); afterwards the same bytes hold the
// cross-wave merge region 4 * 16*CT * (hd + 2) fp32 (33 / 65 / 130 KB). The
// two are never live together (a block barrier separates them); the launch
// takes the larger: 68 / 72 / 130 KB.
#include "attention_decode_impl.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

using namespace decode_attn;

namespace {

constexpr int kSpMaxCols = 64;   // four 16-column MFMA tiles
constexpr int kKRegion = 16384;  // bytes of K staging per wave (64 rows x 256)

template <int CT>
constexpr int sp_lds_bytes() {
  constexpr int walk = 16 * CT * 128 * 2 + 4 * kKRegion;
  constexpr int merge = 4 * 16 * CT * (128 + 2) * 4;
  return walk > merge ? walk : merge;
}

template <int FP8, int CT>
__global__ __launch_bounds__(kBlock) void paged_sp_phase1(
    float* __restrict__ partial,        // [>= B, Hq, C, hd] fp32
    float* __restrict__ ml,             // [>= B, Hq, C, 2] fp32 (m, l)
    const short* __restrict__ q,        // [B, Hq, hd]
    const short* __restrict__ kcache,   // [P, Hkv, ps, hd]
    const short* __restrict__ vcache,   // [P, Hkv, hd, ps]
    const int32_t* __restrict__ page_table,  // [B, max_pages]
    const int32_t* __restrict__ ctx_lens,    // [B]
    const int32_t* __restrict__ item_rows,   // [W, R]
    const int32_t* __restrict__ item_range,  // [W, 2]
    float scale, int chunk, int G, int B, int Hkv, int C, int max_pages,
    int log2_ps, int R) {
  constexpr int hd = 128;
  constexpr int NC = 16 * CT;         // padded columns
  constexpr bool kQRegs = CT <= 2;    // Q fragments live in registers
  constexpr int CG = CT < 2 ? CT : 2; // column tiles per QK/softmax/PV pass
  const int kSlab = chunk / 4;
  const int w = blockIdx.x;
  const int h = blockIdx.y;
  const int c = blockIdx.z;
  const int Hq = Hkv * G;
  // members: the leading entries that name a batch row. More of them than
  // the launch's column tiles hold is a caller error; the clamp keeps every
  // index below in bounds all the same
  const int32_t* irow = item_rows + (int64_t)w * R;
  const int cap = min(R, NC / G);
  int nm = 0;
  while (nm < cap && (unsigned)irow[nm] < (unsigned)B) nm++;
  if (nm == 0) return;
  const int row0 = irow[0];
  const int chunk_start = c * chunk;
  const int t_begin = item_range[2 * w];
  int t_end = item_range[2 * w + 1];
  if (t_end < 0) t_end = ctx_lens[row0];
  t_end = min(t_end, max_pages << log2_ps);
  if (chunk_start < t_begin || chunk_start >= t_end) return;
  const int ncols = nm * G;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int lr = lane & 15;
  const int lg = lane >> 4;
  const int ps = 1 << log2_ps;

  extern __shared__ float lds[];
  short* q_lds_s = reinterpret_cast<short*>(lds);               // [NC][hd]
  short* k_lds = q_lds_s + NC * hd + wid * (kKRegion / 2);      // per-wave
  float* merge = lds;                 // [4][NC][hd+2], after the walk

  // ---- Q of all columns -> LDS (16 B chunks XOR-swizzled by column, like
  // the K rows), zero past ncols. CT <= 2 keeps the fragments in registers;
  // CT = 4 re-reads them per tile (64 more VGPRs would spill).
  for (int i = threadIdx.x; i < NC * 16; i += kBlock) {
    const int col = i >> 4;
    short8 v{};
    if (col < ncols)
      v = *reinterpret_cast<const short8*>(
          q + ((int64_t)irow[col / G] * Hq + h * G + col % G) * hd +
          (i & 15) * 8);
    *reinterpret_cast<short8*>(
        (char*)q_lds_s + col * 256 + (((i & 15) * 16) ^ ((col & 7) << 4))) = v;
  }
  __syncthreads();
  auto q_from_lds = [&](int ct, int kc) {
    const int col = ct * 16 + lr;
    short8 v = *reinterpret_cast<const short8*>(
        (const char*)q_lds_s + col * 256 +
        ((kc * 64 + lg * 16) ^ ((col & 7) << 4)));
    return *reinterpret_cast<bf16x8_t*>(&v);
  };
  bf16x8_t q_frag[kQRegs ? CT : 1][4];
  if constexpr (kQRegs) {
#pragma unroll
    for (int ct = 0; ct < CT; ct++)
#pragma unroll
      for (int kc = 0; kc < 4; kc++) q_frag[ct][kc] = q_from_lds(ct, kc);
  }

  float m_run[CT], l_run[CT];
  f32x4 acc[CT][8];
#pragma unroll
  for (int ct = 0; ct < CT; ct++) {
    m_run[ct] = kNegInf; l_run[ct] = 0.f;
#pragma unroll
    for (int d = 0; d < 8; d++) acc[ct][d] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // a wave whose slab starts at or past t_end walks nothing and brings the
  // empty (m, l) = (kNegInf, 0) to the merge
  const int slab_start = chunk_start + wid * kSlab;
  const int slab_end = min(slab_start + kSlab, t_end);
  const int32_t* pt = page_table + (int64_t)row0 * max_pages;

  // 32 tokens of K -> rows half*32.. of the wave's LDS region [64 rows]
  // [256 B], 16 B chunks XOR-swizzled by row (the decode kernel's staging:
  // contiguous 1 KB bursts, 4 rows each). Rows past slab_end clamp to the
  // last valid token and are zeroed when read.
  auto stage_k32 = [&](int t0, int half, short8 (&sreg)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int tok = t0 + half * 32 + i * 4 + (lane >> 4);
      const int tsafe = tok < slab_end ? tok : slab_end - 1;
      const int64_t pb =
          (((int64_t)pt[tsafe >> log2_ps] * Hkv + h) * ps) * hd;
      sreg[i] = ld8<FP8, 0>(
          kcache, pb + (int64_t)(tsafe & (ps - 1)) * hd + (lane & 15) * 8);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int row = half * 32 + i * 4 + (lane >> 4);
      *reinterpret_cast<short8*>(
          (char*)k_lds + row * 256 +
          (((lane & 15) * 16) ^ ((row & 7) << 4))) = sreg[i];
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  // The four 16-token S^T tiles of the 64-token tile for the CG column tiles
  // from ct0. kc and the 32-token half are the outer loops: the two K
  // fragments of a slice are read from LDS once and feed 2 * CG MFMAs on
  // independent accumulators.
  auto qk_tile = [&](int t0, int ct0, f32x4 (&sT)[CG][4]) {
#pragma unroll
    for (int cg = 0; cg < CG; cg++)
#pragma unroll
      for (int tg = 0; tg < 4; tg++) sT[cg][tg] = f32x4{0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kc = 0; kc < 4; kc++)
#pragma unroll
      for (int half = 0; half < 2; half++) {
        short8 ka[2];
#pragma unroll
        for (int tg2 = 0; tg2 < 2; tg2++) {
          const int row = half * 32 + tg2 * 16 + lr;
          ka[tg2] = *reinterpret_cast<const short8*>(
              (const char*)k_lds + row * 256 +
              ((kc * 64 + lg * 16) ^ ((row & 7) << 4)));
          if (t0 + row >= slab_end) ka[tg2] = short8{};
        }
#pragma unroll
        for (int cg = 0; cg < CG; cg++) {
          bf16x8_t qf;
          if constexpr (kQRegs) qf = q_frag[ct0 + cg][kc];
          else qf = q_from_lds(ct0 + cg, kc);
#pragma unroll
          for (int tg2 = 0; tg2 < 2; tg2++)
            sT[cg][half * 2 + tg2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                *reinterpret_cast<bf16x8_t*>(&ka[tg2]), qf,
                sT[cg][half * 2 + tg2], 0, 0, 0);
        }
      }
    __builtin_amdgcn_s_setprio(0);
  };
  // V^T fragments straight from the d-major pages, as in the decode kernel:
  // vf[da*2+tc] = dims da*16+lr, tokens t0 + tc*32 + lg*8 + 0..7. Tokens
  // past slab_end are zeroed (stale page tails can hold NaN, and P = 0 does
  // not mask NaN * 0).
  auto load_v64 = [&](int t0_, short8 (&vf)[16]) {
#pragma unroll
    for (int tc = 0; tc < 2; tc++) {
      const int tb = t0_ + tc * 32;
      const int tlast = ((slab_end - 1) >> 5) << 5;  // last valid 32-block
      const int tsafe = tb < slab_end ? tb : tlast;
      const int64_t pb =
          (((int64_t)pt[tsafe >> log2_ps] * Hkv + h) * ps) * hd;
      const int tin = tsafe & (ps - 1);
      const int rem = slab_end - tb;
#pragma unroll
      for (int da = 0; da < 8; da++) {
        const int vrow = da * 16 + lr;
        short8 v8 = ld8<FP8, 0>(vcache,
                                pb + (int64_t)vrow * ps + tin + lg * 8);
        if (rem < 32) {
#pragma unroll
          for (int j = 0; j < 8; j++)
            if (lg * 8 + j >= rem) v8[j] = 0;
        }
        vf[da * 2 + tc] = v8;
      }
    }
  };
  // Softmax of one column tile over the four 16-token S^T tiles and its two
  // P fragments. Interior tiles skip the mask; the slab's last tile masks
  // every column at slab_end.
  auto softmax_ct = [&](int t0, bool interior, const f32x4 (&sT)[4],
                        float& m, float& l, f32x4 (&a)[8],
                        bf16x8_t (&p_frag)[2]) {
    float pv[4][4];
    float mt = kNegInf;
    if (interior) {
#pragma unroll
      for (int tg = 0; tg < 4; tg++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          pv[tg][r] = sT[tg][r] * scale;
          mt = fmaxf(mt, pv[tg][r]);
        }
    } else {
#pragma unroll
      for (int tg = 0; tg < 4; tg++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int tok = t0 + tg * 16 + lg * 4 + r;
          pv[tg][r] = (tok < slab_end) ? sT[tg][r] * scale : kNegInf;
          mt = fmaxf(mt, pv[tg][r]);
        }
    }
    swapped_update_max(mt, m, l, a);
    float psum = 0.f;
#pragma unroll
    for (int tg = 0; tg < 4; tg++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        pv[tg][r] = (pv[tg][r] > kNegInf * 0.5f) ? __expf(pv[tg][r] - m)
                                                 : 0.f;
        psum += pv[tg][r];
      }
    psum += __shfl_xor(psum, 16, WAVE_SIZE);
    psum += __shfl_xor(psum, 32, WAVE_SIZE);
    l += psum;
#pragma unroll
    for (int tc = 0; tc < 2; tc++)
      p_frag[tc] = pack_p_frag(pv[tc * 2], pv[tc * 2 + 1]);
  };
  // QK, softmax and PV of the CG column tiles from ct0, one column tile's
  // P fragments live at a time; the V fragments stay in registers and feed
  // every column tile.
  auto columns_pass = [&](int t0, int ct0, const short8 (&v64)[16]) {
    const bool interior = t0 + 64 <= slab_end;
    f32x4 sT[CG][4];
    qk_tile(t0, ct0, sT);
#pragma unroll
    for (int cg = 0; cg < CG; cg++) {
      const int ct = ct0 + cg;
      bf16x8_t p_frag[2];
      softmax_ct(t0, interior, sT[cg], m_run[ct], l_run[ct], acc[ct],
                 p_frag);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int da = 0; da < 8; da++)
#pragma unroll
        for (int tc = 0; tc < 2; tc++) {
          short8 va_s = v64[da * 2 + tc];
          acc[ct][da] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              *reinterpret_cast<bf16x8_t*>(&va_s), p_frag[tc], acc[ct][da],
              0, 0, 0);
        }
      __builtin_amdgcn_s_setprio(0);
    }
  };

  short8 v64[16], sreg[8];
  for (int t0 = slab_start; t0 < slab_end; t0 += 64) {
    stage_k32(t0, 0, sreg);       // K tokens t0..t0+31
    load_v64(t0, v64);            // V loads stay in flight under the QK
    stage_k32(t0, 1, sreg);       // K tokens t0+32..t0+63
    // a pass whose column tiles hold no member (a row's own one-member item
    // in a launch sized for the groups) is skipped: its state stays empty
#pragma unroll
    for (int ct0 = 0; ct0 < CT; ct0 += CG)
      if (ct0 * 16 < ncols) columns_pass(t0, ct0, v64);
    // back-edge fence: the next tile's staging writes must not be scheduled
    // above this tile's outstanding LDS fragment reads
    __builtin_amdgcn_wave_barrier();
  }

  // ---- cross-wave merge: acc[ct][da][r] is O^T[dim da*16+lg*4+r][column
  // ct*16+lr]; the merge region takes over the walk's LDS ----
  __syncthreads();
  float* my = merge + wid * NC * (hd + 2);
#pragma unroll
  for (int ct = 0; ct < CT; ct++) {
    const int col = ct * 16 + lr;
    if (col < ncols) {
#pragma unroll
      for (int da = 0; da < 8; da++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          my[col * (hd + 2) + da * 16 + lg * 4 + r] = acc[ct][da][r];
      if (lg == 0) {
        my[col * (hd + 2) + hd] = m_run[ct];
        my[col * (hd + 2) + hd + 1] = l_run[ct];
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ncols * hd; i += kBlock) {
    const int col = i / hd;
    const int d = i % hd;
    float mw[4], lw[4];
    float mstar = kNegInf;
#pragma unroll
    for (int wv = 0; wv < 4; wv++) {
      mw[wv] = merge[(wv * NC + col) * (hd + 2) + hd];
      lw[wv] = merge[(wv * NC + col) * (hd + 2) + hd + 1];
      mstar = fmaxf(mstar, mw[wv]);
    }
    float lsum = 0.f, asum = 0.f;
#pragma unroll
    for (int wv = 0; wv < 4; wv++) {
      const float corr = (lw[wv] > 0.f) ? __expf(mw[wv] - mstar) : 0.f;
      lsum += lw[wv] * corr;
      asum += merge[(wv * NC + col) * (hd + 2) + d] * corr;
    }
    const int64_t rh = (int64_t)irow[col / G] * Hq + h * G + col % G;
    partial[(rh * C + c) * hd + d] = asum;
    if (d == 0) {
      ml[(rh * C + c) * 2] = mstar;
      ml[(rh * C + c) * 2 + 1] = lsum;
    }
  }
}

}  // namespace

void paged_attention_decode_shared(
    torch::Tensor out, torch::Tensor q, torch::Tensor kcache,
    torch::Tensor vcache, torch::Tensor page_table, torch::Tensor ctx_lens,
    torch::Tensor item_rows, torch::Tensor item_range, torch::Tensor partial,
    torch::Tensor ml, double scale, int64_t chunk_tokens,
    int64_t max_members) {
  TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kBFloat16 && q.dim() == 3 &&
                  q.is_contiguous(),
              "q must be a contiguous bf16 [B, Hq, hd] device tensor");
  TORCH_CHECK(out.dtype() == torch::kBFloat16 && out.is_contiguous() &&
                  out.sizes() == q.sizes(), "out must match q");
  const bool fp8 = kcache.dtype() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || kcache.dtype() == torch::kBFloat16,
              "kv cache must be bf16 or float8_e4m3fn");
  TORCH_CHECK(vcache.dtype() == kcache.dtype() && kcache.dim() == 4 &&
                  vcache.dim() == 4 && kcache.is_contiguous() &&
                  vcache.is_contiguous());
  const int B = q.size(0);
  const int Hq = q.size(1);
  const int hd = q.size(2);
  const int Hkv = kcache.size(1);
  const int ps = kcache.size(2);
  TORCH_CHECK(hd == 128 && kcache.size(3) == hd,
              "shared-prefix attention needs head_dim == 128");
  TORCH_CHECK(ps % 32 == 0 && (ps & (ps - 1)) == 0,
              "shared-prefix attention needs page_size a power of 2, "
              "% 32 == 0");
  TORCH_CHECK(vcache.size(0) == kcache.size(0) && vcache.size(1) == Hkv &&
                  vcache.size(2) == hd && vcache.size(3) == ps,
              "shared-prefix attention reads d-major V pages "
              "[P, Hkv, hd, ps]");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "Hq must be a multiple of Hkv");
  const int G = Hq / Hkv;
  TORCH_CHECK(G >= 2 && G <= 16, "shared-prefix attention needs 2 <= G <= 16 "
              "(got G=", G, ")");
  TORCH_CHECK(max_members >= 1 && max_members * G <= kSpMaxCols,
              "shared-prefix attention takes max_members * G <= ", kSpMaxCols,
              " (got max_members=", max_members, ", G=", G, ")");
  for (const torch::Tensor* t : {&page_table, &ctx_lens, &item_rows,
                                 &item_range})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kInt32 &&
                    t->is_contiguous(), "index tensors must be int32, "
                "contiguous, on the device");
  TORCH_CHECK(page_table.dim() == 2 && page_table.size(0) == B &&
                  ctx_lens.numel() == B,
              "page_table / ctx_lens must have one row per batch row");
  const int R = kSpMaxCols / G;
  const int W = item_rows.size(0);
  TORCH_CHECK(item_rows.dim() == 2 && item_rows.size(1) == R,
              "item_rows must be [W, ", R, "] (64 / G members per item)");
  TORCH_CHECK(item_range.dim() == 2 && item_range.size(0) == W &&
                  item_range.size(1) == 2, "item_range must be [W, 2]");
  const int C = ml.size(2);
  TORCH_CHECK(partial.dtype() == torch::kFloat32 && partial.is_contiguous() &&
                  partial.dim() == 4 && partial.size(0) >= B &&
                  partial.size(1) == Hq && partial.size(2) == C &&
                  partial.size(3) == hd, "partial must be [>= B, Hq, C, hd]");
  TORCH_CHECK(ml.dtype() == torch::kFloat32 && ml.is_contiguous() &&
                  ml.dim() == 4 && ml.size(0) >= B && ml.size(1) == Hq &&
                  ml.size(3) == 2, "ml must be [>= B, Hq, C, 2]");
  const int chunk = (int)chunk_tokens;
  TORCH_CHECK(chunk >= 128 && chunk % 128 == 0, "bad chunk_tokens ", chunk);
  if (B == 0) return;
  int log2_ps = 0; while ((1 << log2_ps) < ps) log2_ps++;
  const int max_pages = page_table.size(1);
  auto stream = at::cuda::getCurrentHIPStream();

  auto launch = [&](auto* kern, int lds) {
    if (lds > 65536)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds);
    kern<<<dim3(W, Hkv, C), kBlock, lds, stream>>>(
        partial.data_ptr<float>(), ml.data_ptr<float>(),
        (const short*)q.data_ptr(), (const short*)kcache.data_ptr(),
        (const short*)vcache.data_ptr(), page_table.data_ptr<int32_t>(),
        ctx_lens.data_ptr<int32_t>(), item_rows.data_ptr<int32_t>(),
        item_range.data_ptr<int32_t>(), (float)scale, chunk, G, B, Hkv, C,
        max_pages, log2_ps, R);
  };
  if (W > 0) {
    // column tiles: ceil(max_members * G / 16), 3 rounded up to 4
    const int cols = (int)max_members * G;
    if (cols <= 16) {
      if (fp8) launch(&paged_sp_phase1<1, 1>, sp_lds_bytes<1>());
      else launch(&paged_sp_phase1<0, 1>, sp_lds_bytes<1>());
    } else if (cols <= 32) {
      if (fp8) launch(&paged_sp_phase1<1, 2>, sp_lds_bytes<2>());
      else launch(&paged_sp_phase1<0, 2>, sp_lds_bytes<2>());
    } else {
      if (fp8) launch(&paged_sp_phase1<1, 4>, sp_lds_bytes<4>());
      else launch(&paged_sp_phase1<0, 4>, sp_lds_bytes<4>());
    }
    HIP_CHECK_KERNEL();
  }
  paged_decode_phase2<<<dim3(B, Hq), 128, 0, stream>>>(
      (short*)out.data_ptr(), partial.data_ptr<float>(), ml.data_ptr<float>(),
      ctx_lens.data_ptr<int32_t>(), chunk, Hq, C, hd);
  HIP_CHECK_KERNEL();
}
