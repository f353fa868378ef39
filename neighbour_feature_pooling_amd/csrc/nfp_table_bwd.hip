// nfp_table_bwd.hip — the table kernels' backward: bwd_fast (nfp_fast.h) in its vector form and its two matrix-core forms,
// with their launchers (interface: nfp_launch.h::table_backward).
#include "nfp_launch.h"
#include "nfp_fast.h"

using namespace nfp;

namespace nfp_host {
namespace {

#ifndef NFP_BWD_SLAB_KB
#define NFP_BWD_SLAB_KB 60
#endif
constexpr int kSlabBudgetBwd = NFP_BWD_SLAB_KB * 1024;

// channels per LDS chunk: bounded by the slab budget and by what one staging round-set can carry
int chunk_channels(const KP& g, int total, int T, int G, bool nhwc, int budget) {
  int ncq = budget / (nfp::bwd_row_slots(g.P, nhwc) * 16);
  if (nhwc) {
    if (ncq > kRN * G) ncq = kRN * G;
  } else {  // ceil(P/4) blocks per channel row, the last one overlapping (nfp_fast.h: StagedOvl)
    const int NQb = (g.P + 3) >> 2;
    if (ncq > (kRB * T) / NQb) ncq = (kRB * T) / NQb;
  }
  if (ncq > 2047) ncq = 2047;  // fast_div quotient bound
  if (ncq < 1) ncq = 1;
  int cmax = 4 * ncq;
  int nch = (total + cmax - 1) / cmax;
  return round4((total + nch - 1) / nch);
}

// LDS of bwd_fast's phase A: tables that live to the end of the kernel (Wt, Dt, two norm factors per pixel), and
// the per-pair values, which are dead once Wt is built (nfp_fast.h::bwd_fast)
size_t bwd_fixed_bytes(const KP& g, int K2) { return ((size_t)(2 * g.P * K2 + 2 * g.P) * 4 + 15) & ~(size_t)15; }
size_t bwd_pair_bytes(const KP& g, int M, int N) {
  return ((size_t)((M == NFP_COSINE ? 2 : 1) * (N * g.P + 1)) * 4 + 15) & ~(size_t)15;   // (+ the zero an empty list entry reads)
}
constexpr size_t kEarlyBudget = 96 * 1024;  // slab beside the pair values (committed during phase A) up to this much LDS

template <int R, int M, bool BF, bool NHWC, int POOL = kPoolNone, bool MF = false>   // MF: float32 maps beside bf16 x
int launch_bwd_fast_t(KP g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                      hipStream_t st, const BwdTail& t) {
  constexpr int N = Win<R>::N, K2 = Win<R>::K2;
#ifndef NFP_BWD_WGS
#define NFP_BWD_WGS 256
#endif
  int S = (NFP_BWD_WGS + g.B - 1) / g.B;  // channel blocks per image so that >= NFP_BWD_WGS workgroups exist
  // ... and twice as many while a workgroup's block stays large ([256,960,7,7]: 22.9 -> 21.5 us, [256,192,14,14]: 21.3 ->
  // 20.2 us; not [256,512,7,7]: 13.8 -> 14.0 us): phase A is repeated per block, the streaming part is what splits.
  // k = 3 only: a 5x5 window's phase A is a third of the kernel ([256,192,14,14] L2 k = 5 f32: 41.0 -> 49.6 us split)
  if (K2 <= 9 && (long long)g.C * g.P / S >= 32768 && (long long)g.B * S < 2 * NFP_BWD_WGS)
    S = (2 * NFP_BWD_WGS + g.B - 1) / g.B;
  if (S > g.C / 4) S = g.C / 4;
  if (S < 1) S = 1;
  g.Cwg = round4((g.C + S - 1) / S);
  S = (g.C + g.Cwg - 1) / g.Cwg;
  // From four workgroups per CU on (k = 3): quarter-size workgroups, four per CU (128 registers: 1024 threads per CU
  // either way) — they overlap each other's phases better than two of 512: [4096,64,7,7] 45 -> 33 us, [4096,512,7,7] 176 ->
  // 168, [1024,256,14,14] 100 -> 94.  Not k = 5: its 13-entry-per-pixel phase A on 256 threads doubles the kernel
  // ([2048,192,14,14] 290 -> 486 us).  (-DNFP_BWD_SAT_T=512 builds the old arm.)
#ifndef NFP_BWD_SAT_T
#define NFP_BWD_SAT_T 256
#endif
#ifndef NFP_BWD_SAT_SLAB
#define NFP_BWD_SAT_SLAB 2
#endif
  // (channels-last, lanes along a pixel's channel groups since round 4: a quarter-size workgroup has G = 5 groups at 7x7 —
  // 80-byte runs of a 2 KB pixel; with 512 threads G = 10: [4096,512,7,7] 209 -> 147 us, [1024,512,7,7] 45 -> 38; narrow
  // pixels keep the quarter size: [4096,64,7,7] 27 vs 32 us — profiles/r04_p_…)
  const bool satb = K2 <= 9 && (long long)g.B * S >= 1024 && g.P <= NFP_BWD_SAT_T && NFP_BWD_SAT_T < kBwdThreads &&
                    !(NHWC && g.C > 128);
  g.G = (satb ? NFP_BWD_SAT_T : kBwdThreads) / g.P;
  if (g.G < 1) g.G = 1;
  if (g.G > g.Cwg / 4) g.G = g.Cwg / 4;
  int T = ((g.P * g.G + 63) / 64) * 64;
  // large batches (one workgroup per image, several images per CU over time): fewer, larger chunks win
  const int bbudget = satb ? NFP_BWD_SAT_SLAB * kSlabBudgetBwd / 2 : ((S == 1 && g.B > 256) ? 2 * kSlabBudgetBwd : kSlabBudgetBwd);
  g.Cc = chunk_channels(g, g.Cwg, T, g.G, NHWC, bbudget);
  g.G = even_groups(g.Cc / 4, g.G);
  T = ((g.P * g.G + 63) / 64) * 64;
  g.Cc = chunk_channels(g, g.Cwg, T, g.G, NHWC, bbudget);
  const size_t fixed = bwd_fixed_bytes(g, K2), pairs = bwd_pair_bytes(g, M, N);
  const size_t slab = (size_t)(g.Cc / 4) * nfp::bwd_row_slots(g.P, NHWC) * 16;
  g.early = fixed + pairs + slab <= kEarlyBudget ? 1 : 0;
  const size_t lds = g.early ? fixed + pairs + slab : fixed + std::max(pairs, slab);
  if (lds > (size_t)kLdsMax) return kNotApplicable;  // tables + slab do not fit: the generic kernels serve it
  snprintf(g_variant, sizeof(g_variant), "bwd_fast<R%s,%s,%s,%s%s>", R == 12 ? "1+2" : (R == 1 ? "1" : "2"),
           hot_name(g), MF ? "mix" : (BF ? "bf16" : "f32"), NHWC ? "nhwc" : "nchw", pool_tag(POOL));
  // NCHW staging form (nfp_fast.h: StagedRows).  By pixel rows for ONE class: float32, k = 3, plain maps, the cosine and L2
  // instantiations (with their dot / gfc / rmse riders; Norm p = 1 and the symmetric-term measures keep the blocks: an
  // instantiation more each for measures no in-tree model uses), a single chunk (Cc covers the workgroup's channels), at
  // most one workgroup per CU (beyond that latency no longer counts) and at most kRS slots per thread.  Everything else:
  // 4 x 4 blocks, as before.  NFP_STAGE_BLOCKS=1 forces the blocks; the two forms agree bitwise.
  // (the slot bound is this change's own, a register budget: kRS slots are 24 staging registers against the blocks' 48;
  // a single-chunk launch beyond it — [128,512,7,7]: 64 quads on 10 groups, 7 slots — keeps the blocks)
  const uint32_t hgeom = nfp::bwd_head_geom(g.P, g.mode, g.unit, g.G, T);
  if constexpr (R == 1 && !BF && !NHWC && POOL == kPoolNone && (M == NFP_COSINE || M == NFP_NORM)) {
    if (!satb && g.Cc >= g.Cwg && ceil_div(g.Cwg / 4, g.G) <= nfp::kRS && !g_sw.stage_blocks.load(std::memory_order_relaxed))
      return launch_staged(true, "bwd_fast", bwd_fast<R, M, BF, NHWC, POOL, 0, true>, dim3(g.B, S), dim3(T), lds, st, x, go, out,
                           saved, g.ws, hgeom, g.C, g.Cwg, g.Cc, gx, t.ggap, t.gnfpm, g);
  }
  if constexpr (!NHWC)
    return launch_staged(false, "bwd_fast", bwd_fast<R, M, BF, NHWC, POOL, 0, false, MF>, dim3(g.B, S), dim3(T), lds, st, x, go, out, saved,
                         g.ws, hgeom, g.C, g.Cwg, g.Cc, gx, t.ggap, t.gnfpm, g);
  else
    return launch("bwd_fast", bwd_fast<R, M, BF, NHWC, POOL, 0, false, MF>, dim3(g.B, S), dim3(T), lds, st, x, go, out, saved, g.ws, hgeom,
                  g.C, g.Cwg, g.Cc, gx, t.ggap, t.gnfpm, g);
}

// Phase B of the backward on the matrix cores (nfp_fast.h::bwd_gemm_phase): bf16 storage, C a multiple of 32.
template <int R, int M, bool NHWC, int POOL = kPoolNone>
int launch_bwd_gemm_t(KP g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                      hipStream_t st, const BwdTail& t) {
  constexpr int N = Win<R>::N, K2 = Win<R>::K2;
  if (!mfma_enabled() || g.dtype != NFP_BF16 || (g.C & 31) || mixed_maps(g)) return kNotApplicable;
  if (NHWC && (((uintptr_t)x & 15) || ((g.sB * 2) & 15) || ((uintptr_t)gx & 15) || ((g.gB * 2) & 15)))
    return kNotApplicable;  // 16-byte staging loads and grad_x stores
  int S = (NFP_BWD_WGS + g.B - 1) / g.B;  // channel blocks per image, whole 32-channel tiles each
  if (S > g.C / 32) S = g.C / 32;
  if (S < 1) S = 1;
  g.Cwg = ((g.C / 32 + S - 1) / S) * 32;
  S = (g.C + g.Cwg - 1) / g.Cwg;
  // NCHW rows that are not 8-byte aligned (H*W % 4 != 0) are staged and stored 2 bytes at a time: that only pays
  // while the batch is small enough for the channel split (measured: 7.2 vs 8.4 us at B = 64, 16.1 vs 14.0 at 256)
  if (!NHWC && (g.P & 3) && S < 2) return kNotApplicable;
  // the matrix-core variant keeps nothing of x in registers, so it may run 16 wavefronts: that pays when phase A has
  // thousands of table entries to build (k = 5 at 14x14: 36 -> 29.5 us), not at 7x7 with k = 3 (7.2 -> 7.7 us)
  g.G = (g.P * K2 > 2048 ? 1024 : kBwdThreads) / g.P;
  if (g.G < 1) g.G = 1;
  if (g.G > g.Cwg / 4) g.G = g.Cwg / 4;
  int T = ((g.P * g.G + 63) / 64) * 64;
  // phase A of this variant is loop-free (nfp_fast.h): one round of pair values, at most kGemmPre gather rounds
  const int NJ = Win<R>::RAD >= 2 ? Win<R>::NF + 1 : K2, NE = g.P * NJ, NO = N * g.P;
  if (NE > nfp::kGemmPre * T || NO > 8 * T) T = 1024;
  if (NE > nfp::kGemmPre * T || NO > 8 * T) return kNotApplicable;
  g.Cc = g.Cwg;
  const int band = g.R * g.W + g.R, KW = nfp::gemm_kw(band);
  const size_t xq = (size_t)((((g.P + 15) >> 4 << 1) + 1) | 1), wq = (size_t)((2 * KW + 1) | 1);
  // row tiles whose densified weights sit in LDS together (fewer rounds of zero / scatter / barrier): all that fit
  const int nt = (g.P + 31) / 32;
  // LDS of this variant (nfp_fast.h::bwd_fast, GEMM): Wt | ipn | dfn live to the end; Dt and the pair values are dead once
  // the diagonal is folded — the operand images lie over both
  const size_t xt = (size_t)g.Cwg * xq * 16, wd1 = (size_t)2 * 32 * wq * 16;
  const size_t fixed = ((size_t)(g.P * K2 + 2 * g.P) * 4 + 15) & ~(size_t)15, dtb = ((size_t)g.P * K2 * 4 + 15) & ~(size_t)15;
  const size_t ggb = POOL != kPoolNone ? (size_t)g.Cwg * 4 : 0;   // grad(GAP(x)) of the block, staged behind Wd
  int rt = fixed + xt + ggb < (size_t)kLdsMax ? (int)(((size_t)kLdsMax - fixed - xt - ggb) / wd1) : 0;
  rt = std::min(rt, nt);
  // Second form (round 4): Wd of ALL row tiles, written by phase A itself, x in chunks of `ctr` channel tiles (about one output
  // tile per wavefront and chunk), two buffers — where that fits
  // (measured, profiles/r04_zb_…: 17.4 -> 16.2 us at config 5, where the first form takes two rounds; where the first form
  // holds every row tile in ONE round — 7 x 7 maps — it stays: 10.2 vs 12.2 us at [256,512,7,7], 5.96 vs 6.5 at [64,512,7,7])
  if (const int g3 = g_sw.gemm3.load(std::memory_order_relaxed); g3 == 2 || (g3 == 1 && rt < nt)) {
    const int nw = T / 64, nct = g.Cwg / 32;
    int ctr = std::max(1, std::min(nct, nw / nt));
    const int nch = (nct + ctr - 1) / ctr;
    ctr = (nct + nch - 1) / nch;   // even chunks
    const size_t fixed3 = ((size_t)(3 * g.P + (POOL != kPoolNone ? g.Cwg : 0)) * 4 + 15) & ~(size_t)15;
    const size_t xtc = (size_t)32 * ctr * xq * 16;
    const size_t lds3 = fixed3 + (size_t)nt * wd1 + std::max((size_t)(nch > 1 ? 2 : 1) * xtc, bwd_pair_bytes(g, M, N) + dtb);
    if (lds3 <= (size_t)kLdsMax) {
      g.Tc = ctr;
      g.early = 0;
      snprintf(g_variant, sizeof(g_variant), "bwd_fast<R%d,%s,bf16,%s,mfma2%s>", R, hot_name(g), NHWC ? "nhwc" : "nchw",
               pool_tag(POOL));
      return launch("bwd_fast_mfma2", bwd_fast<R, M, true, NHWC, POOL, 2>, dim3(g.B, S), dim3(T), lds3, st, x, go, out, saved,
                    g.ws, nfp::bwd_head_geom(g.P, g.mode, g.unit, g.G, T), g.C, g.Cwg, g.Cc, gx, t.ggap, t.gnfpm, g);
    }
  }
  if (rt >= 2 && rt < nt) rt = (nt + ((nt + rt - 1) / rt) - 1) / ((nt + rt - 1) / rt);  // even rounds
  if (rt < std::min(2, nt)) return kNotApplicable;
  g.Tc = rt;
  const size_t images = xt + (size_t)rt * wd1 + ggb;
  const size_t lds = fixed + std::max(dtb + bwd_pair_bytes(g, M, N), images);
  g.early = 0;
  if (lds > (size_t)kLdsMax) return kNotApplicable;
  snprintf(g_variant, sizeof(g_variant), "bwd_fast<R%d,%s,bf16,%s,mfma%s>", R, hot_name(g),
           NHWC ? "nhwc" : "nchw", pool_tag(POOL));
  return launch("bwd_fast_mfma", bwd_fast<R, M, true, NHWC, POOL, 1>, dim3(g.B, S), dim3(T), lds, st, x, go, out, saved,
                g.ws, nfp::bwd_head_geom(g.P, g.mode, g.unit, g.G, T), g.C, g.Cwg, g.Cc, gx, t.ggap, t.gnfpm, g);
}

// The table backward: phase B on the matrix cores where that form exists (bf16 maps, one radius, cosine / L2) and applies,
// else the vector (VALU) form, which serves every radius spec.  (float32 maps beside bf16 x: the vector form — the
// matrix-core backward stages grad_out / out under an LDS budget sized for 2-byte values.)
template <int R, int M, int POOL = kPoolNone>
int launch_bwd_fast(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                    hipStream_t st, const BwdTail& t) {
  return with_storage_mixed<R, M, POOL>(g, [&](auto bf, auto nhwc, auto mf) {
    if constexpr (bf() && !mf() && R != 12 && (M == NFP_COSINE || M == NFP_NORM))
      if (int rc = launch_bwd_gemm_t<R, M, nhwc(), POOL>(g, x, go, out, saved, gx, st, t); rc != kNotApplicable)
        return rc;
    return launch_bwd_fast_t<R, M, bf(), nhwc(), POOL, mf()>(g, x, go, out, saved, gx, st, t);
  });
}

}  // namespace

int table_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st,
                   const BwdTail& t) {
  return with_radius<true>(g, [&](auto r) { return with_hot<true>(g, [&](auto m) { return with_pool(t.mode, [&](auto p) {
    constexpr int R = decltype(r)::value, M = decltype(m)::value, POOL = decltype(p)::value;
    if constexpr (kHasTable<R, M, POOL>)
      return launch_bwd_fast<R, M, POOL>(g, x, go, out, saved, gx, st, t);
    else
      return kNotApplicable;
  }); }); });
}

}  // namespace nfp_host

NFP_STAMP_SETTER(table_bwd)
