// nfp_table_fwd.hip — the table kernels' forward: the row-banded fwd_band (nfp_band.h) and the matrix-core fwd_gram
// (nfp_mfma.h) with their launchers (interface: nfp_launch.h::table_fwd_gram / table_fwd_band).
#include "nfp_launch.h"
#include "nfp_band.h"
#include "nfp_mfma.h"

using namespace nfp;

namespace nfp_host {
namespace {

// ---- fast-path launches (nfp_fast.h) ----------------------------------------------------------
#ifndef NFP_FWD_SLAB_KB
#define NFP_FWD_SLAB_KB 128
#endif

// Row-banded forward (nfp_band.h): needs the descriptor's workspace tables.
#ifndef NFP_BAND_WGS
#define NFP_BAND_WGS 256
#endif
template <int R, int M, bool BF, bool NHWC, int POOL = kPoolNone, bool MF = false>   // MF: float32 maps beside bf16 x
int launch_fwd_band_t(KP g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t) {
  constexpr int NF = Win<R>::NF;
  int nb = std::min(g.H, (NFP_BAND_WGS + g.B - 1) / g.B);   // bands per image so that >= NFP_BAND_WGS workgroups exist
  // two workgroups per CU overlap each other's load and sum phases — worth it while a band's R halo rows stay a small
  // part of what it stages (14x14, k = 3 at B = 256: 12.8 -> 10.8 us; not 7x7: 7.3 -> 8.2 us)
  nb = std::max(nb, std::min((2 * NFP_BAND_WGS + g.B - 1) / g.B, g.H / (6 * g.R)));
  // The pooled outputs are sums over the whole image.  One workgroup per image writes them itself; several bands per image
  // write partial sums that a second launch (pool_fold) joins.  Measured at [64,512,7,7] (profiles/r03_i_fused_callers.jsonl):
  // four bands + fold 9.5 us against 8.1 us for one band — the second launch costs more than the bands save — so the table
  // kernels keep one band (-DNFP_POOL_BANDS=1 builds the other arm; the row-band kernels of nfp_tile.h, whose maps do not
  // fit one workgroup, always fold).
#ifndef NFP_POOL_BANDS
#define NFP_POOL_BANDS 0
#endif
  // Round 4: with the workspace's arrival counters the last band to finish folds them all inside the SAME launch
  // (nfp_common.h::pool_last_band): the bands come back.  Without counters: one band, as before.
  if (POOL && (t.part == nullptr || !(NFP_POOL_BANDS || g.tickets != nullptr))) nb = 1;
  const int rb = (g.H + nb - 1) / nb;
  nb = (g.H + rb - 1) / rb;
  const int psm = std::min(g.P, (rb + g.R) * g.W);          // most pixels a band stages
  // channel groups: a power of two (adjacent lanes, joined by DPP), as many as kBandT threads and C allow, <= 32
  // (up to one workgroup per CU, latency counts: all the threads a workgroup may have.  Beyond one workgroup per CU latency no longer counts and every extra thread's index work is paid for: half the
  // threads on half-size slabs, two workgroups per CU; from four workgroups per CU on, a quarter — four 256-thread
  // workgroups overlap each other's load / sum phases better than two of 512: [4096,512,7,7] cold 91.5 -> 85.4 us, [1024,…]
  // 27.5 -> 26.2; an eighth is no better.  -DNFP_BAND_SAT_SHIFT=1 builds the old arm)
#ifndef NFP_BAND_SAT_SHIFT
#define NFP_BAND_SAT_SHIFT 2
#endif
  // (a band of more pixels than a quarter workgroup has threads stays at two per CU — the registers of 104-VGPR wavefronts
  // hold 1024 threads per CU, whatever the slabs: [2048,64,20,20] 63 vs 73 us)
  const long long nwg = (long long)g.B * nb;
  const int sat = nwg > 256 ? ((nwg >= 1024 && psm <= (kBandT >> NFP_BAND_SAT_SHIFT)) ? NFP_BAND_SAT_SHIFT : 1) : 0;
  const int tcap = kBandT >> sat;
  int lg = 0;
  while (lg < 5 && (2 << lg) * psm <= tcap && (2 << lg) <= g.C / 4) ++lg;
  g.G = 1 << lg;
  g.Tc = lg;
  const int T = ((g.G * psm + 63) / 64) * 64;
  const int nqb = (psm + 3) / 4 + 1, ppb = ((psm + 3 + 8) & ~3) + 4;   // blocks / slots per slab row, alignment slack and
                                                                       // the bank padding of band_row_slots included
  // up to one workgroup per CU the whole band is staged at once; beyond that, half-size slabs let two workgroups share a
  // CU and overlap each other's load / sum phases ([4096,512,7,7]: 91 vs 118 us)
  const int budget = (NFP_FWD_SLAB_KB * 1024) >> sat;
  int ncq = budget / (ppb * 16);
  ncq = std::min(ncq, NHWC ? kBandRN * g.G : (kBandRB * T) / nqb);
  if (ncq < 1) return kNotApplicable;
  const int total = g.C / 4, nch = (total + ncq - 1) / ncq;
  g.Cc = 4 * ((total + nch - 1) / nch);
#ifndef NFP_BAND_PF
#define NFP_BAND_PF 1
#endif
  // (measured, profiles/r04_a_…: [4096,512,7,7] forward 84.8 -> 83.1 us cold, 81.6 -> 80.0 resident; k = 5 loses 1-3 %:
  // its sums already hide the next chunk's latency behind four times the LDS reads)
  g.pf = (NFP_BAND_PF && nch > 1 && Win<R>::RAD == 1) ? 1 : 0;
  const size_t slab = (size_t)(g.Cc / 4) * ppb * 16;
  const size_t tail = (size_t)psm * (NF + 1) * 4 + (POOL == kPoolBoth ? (size_t)Win<R>::N * psm * 4 : 0);   // Tt (+ pooled-map staging)
  const size_t lds = slab + tail;
  if (lds > (size_t)kLdsMax) return kNotApplicable;
  snprintf(g_variant, sizeof(g_variant), "fwd_band<R%s,%s,%s,%s%s>x%d", R == 12 ? "1+2" : (R == 1 ? "1" : "2"), hot_name(g),
           MF ? "mix" : (BF ? "bf16" : "f32"), NHWC ? "nhwc" : "nchw", pool_tag(POOL), nb);
  if (t.nb) *t.nb = nb;
  // the kernel's preloadable head (nfp_common.h): what stands in front of its first x request
  const uint32_t sB_lo = (uint32_t)((unsigned long long)g.sB & 0xFFFFFFFFull), sB_hi = (uint32_t)((unsigned long long)g.sB >> 32);
  const uint32_t hchunk = nfp::band_head_chunk(g.Cc, lg, g.R, T), hgeom = nfp::band_head_geom(g.H, g.W, rb);
  // (NCHW staging: always the 4 x 4 blocks here.  The pixel-row form bwd_fast takes — launch_bwd_fast_t — was built for this
  // kernel too and measured no faster at the headline shape, 4.80 -> 4.86 us: profiles/r05_b_nchw_row_staging_ab.txt)
  auto go = [&](auto kernel) {
    if constexpr (NHWC)
      return launch("fwd_band", kernel, dim3(g.B, nb), dim3(T), lds, st, x, g.ws, sB_lo, sB_hi, g.C, hchunk, hgeom, out, saved,
                    t.gap, t.nfpm, t.part, g);
    else
      return launch_staged(false, "fwd_band", kernel, dim3(g.B, nb), dim3(T), lds, st, x, g.ws, sB_lo, sB_hi, g.C, hchunk,
                           hgeom, out, saved, t.gap, t.nfpm, t.part, g);
  };
  // (pooled, several bands: the bands' partial sums go to t.part; the caller folds them — nfp_hip.hip::fused_forward)
  if constexpr (M != kSymTerm)
  if (g.unit || g.gfc || g.d2s != 1.f)   // DotProduct / GFC / RMSE: the finalize with the run-time constants
    return go(fwd_band<R, M, BF, NHWC, POOL, true, MF>);
  return go(fwd_band<R, M, BF, NHWC, POOL, false, MF>);
}

template <int R, int M, int POOL = kPoolNone>
int launch_fwd_band(const KP& g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t) {
  if (g.ws == nullptr) return kNotApplicable;
  return with_storage_mixed<R, M, POOL>(g, [&](auto bf, auto nhwc, auto mf) {
    return launch_fwd_band_t<R, M, bf(), nhwc(), POOL, mf()>(g, x, out, saved, st, t);
  });
}

// Matrix-core forward (nfp_mfma.h): bf16, dense channels-last, C a multiple of 16.  Of the tail it takes the two outputs alone.
template <int R, int M>
int launch_fwd_gram(const KP& g, const void* x, void* out, float* saved, hipStream_t st, float* gap, float* nfpm) {
  if (!mfma_enabled() || g.dtype != NFP_BF16 || (g.C & 15) || g.P > 512) return kNotApplicable;
  if (mixed_maps(g)) return kNotApplicable;   // (the Gram-form L2 loses digits a float32 map would show: DESIGN §4)
  if (g.unit || g.gfc || g.d2s != 1.f) return kNotApplicable;   // (DotProduct / GFC / RMSE: the vector kernels' run-time constants)
  if (!g.contig && (((uintptr_t)x & 15) || ((g.sB * 2) & 15))) return kNotApplicable;  // 16-byte fragment loads
  const int nt = (g.P + 31) / 32, D = std::min(nt - 1, (g.R * g.W + g.R + 31) / 32);
  const size_t tiles = (((size_t)nt * (D + 1) * 32 * kGramLd + 3) & ~(size_t)3) * 4;
  const size_t image = (size_t)g.P * (g.C / 8 + 1) * 16;
  if (tiles > (size_t)kLdsMax) return kNotApplicable;
  if (g.contig && tiles + image > (size_t)kLdsMax) return kNotApplicable;  // NCHW is transposed through LDS only
  if (tiles + (size_t)g.P * 8 > (size_t)kLdsMax) return kNotApplicable;  // (the norm tables reuse the image's words)
  // the pooled variant takes its sums from the LDS image and stages the map values in it afterwards; GAP(x) alone (gap set,
  // nfpm null: nfp_gap_forward) needs the LDS image too, and nothing behind it
  if (gap != nullptr && nfpm == nullptr && tiles + image > (size_t)kLdsMax) return kNotApplicable;
  if (nfpm != nullptr && (tiles + image > (size_t)kLdsMax || image < (size_t)(2 + Win<R>::N) * g.P * 4)) return kNotApplicable;
  snprintf(g_variant, sizeof(g_variant), "fwd_gram<R%d,%s,bf16,%s%s>", R, hot_name(g),
           g.contig ? "nchw" : "nhwc", nfpm != nullptr ? ",pool" : (gap != nullptr ? ",gap" : ""));
  if (g.contig)
    return launch("fwd_gram", fwd_gram<R, M, true, true>, dim3(g.B), dim3(1024), tiles + image, st, g, x, out, saved, D, g.ws,
                  gap, nfpm);
  if (tiles + image <= (size_t)kLdsMax)
    return launch("fwd_gram", fwd_gram<R, M, true>, dim3(g.B), dim3(1024), tiles + image, st, g, x, out, saved, D, g.ws, gap,
                  nfpm);
  return launch("fwd_gram", fwd_gram<R, M, false>, dim3(g.B), dim3(1024), tiles + (size_t)g.P * 8, st, g, x, out, saved, D, g.ws,
                (float*)nullptr, (float*)nullptr);
}

}  // namespace

int table_fwd_gram(const KP& g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t) {
  return with_radius<true>(g, [&](auto r) { return with_hot<true>(g, [&](auto m) {
    constexpr int R = decltype(r)::value, M = decltype(m)::value;
    if constexpr (R != 12 && (M == NFP_COSINE || M == NFP_NORM))   // the matrix-core forward has these two forms alone
      return launch_fwd_gram<R, M>(g, x, out, saved, st, t.gap, t.nfpm);
    else
      return kNotApplicable;
  }); });
}

int table_fwd_band(const KP& g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t) {
  return with_radius<true>(g, [&](auto r) { return with_hot<true>(g, [&](auto m) { return with_pool(t.mode, [&](auto p) {
    constexpr int R = decltype(r)::value, M = decltype(m)::value, POOL = decltype(p)::value;
    if constexpr (kHasTable<R, M, POOL>)
      return launch_fwd_band<R, M, POOL>(g, x, out, saved, st, t);
    else
      return kNotApplicable;
  }); }); });
}

}  // namespace nfp_host

NFP_STAMP_SETTER(table_fwd)
