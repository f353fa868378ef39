// nfp_tile_fwd.hip — the row-band forward of nfp_tile.h (fwd_tile, and pool_fold behind its pooled forms) with its launcher
// (interface: nfp_launch.h::tile_forward / tile_pool_fold; sizing shared with the backward: nfp_tile_launch.h).
// Compiled twice: as itself for radii 1 and 2, and — included by nfp_tile_r3_fwd.hip with NFP_TILE_R3_UNIT — for radius 3
// (tile_forward_r3), so that the k = 7 instantiations compile beside the others and not behind them.
#include "nfp_tile_launch.h"

using namespace nfp;

namespace nfp_host {
namespace {

// MF: float32 maps beside bf16 x (mixed_maps, nfp_launch.h) — the register-staged kernel, not the LDS-DMA one
template <int R, int M, bool BF, bool NHWC, int POOL = nfp::kPoolNone, bool MF = false>
int launch_fwd_tile_t(KP g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t) {
  constexpr int NF = Win<R>::NF, N = Win<R>::N;
  constexpr int NP = POOL == nfp::kPoolBoth ? N : 0;   // map sums behind the channel sums of a scratch row
  const int Wu = g.W + 2 * R;
  for (int attempt = 0; attempt < 2; ++attempt) {
    // first choice: two workgroups of up to 1024 threads per compute unit — half of LDS each, 64 registers.
    // Second: one workgroup and all of LDS.
    const size_t budget = attempt == 0 ? tile_lds() : (size_t)kLdsMax;
    const int kCap = tile_cap(1024);                           // threads per workgroup (64 registers either radius)
    for (int rb0 = tile_rows_wanted(g, kCap); rb0 >= 1; --rb0) {
      int nb = 1;
      const int rb = tile_bands(g, rb0, nb);
      if (rb < 1) break;
      const int rows = rb + 2 * R, npu = rows * Wu, nbp = rb * g.W;
      const int lg = tile_groups(g, nb, npu, kCap, g.C / 4), G = 1 << lg;
      const int ppb = nfp::band_row_slots((npu + 3) & ~3, lg);
      const size_t tail = 16 + (size_t)(NF + 1) * npu * 4;                      // spare slot, pair sums, factors
      const size_t vmb = POOL == nfp::kPoolBoth ? (((size_t)N * nbp + 3) / 4) * 16 : 0;            // pooled: the band's maps, over the slab
      constexpr size_t SB = BF ? 8 : 16;   // bytes of a slab slot (four channels of a position in the storage type: nfp_tile.h::Quad)
      if (tail + std::max((size_t)ppb * SB, vmb) > budget) continue;
      int ncq = (int)((budget - tail) / ((size_t)ppb * SB));
      ncq = std::min(ncq, std::min(nfp::Quad<BF>::KQ * G, g.C / 4));
      if (ncq < 1) continue;
      const int total = g.C / 4, nch = ceil_div(total, ncq);
      g.Cc = 4 * ceil_div(total, nch);
      g.G = G;
      g.Tc = -1;
      if (NHWC && G == 1) {   // wavefront-shared staging: chunks of 1, 2, 4 (bf16: 8) quads (nfp_tile.h::TileStage)
        g.Tc = (BF && ncq >= 8) ? 3 : (ncq >= 4 ? 2 : (ncq >= 2 ? 1 : 0));
        g.Cc = 4 << g.Tc;
      }
      size_t lds = std::max((size_t)(g.Cc / 4) * ppb * SB, vmb) + tail;
      // Round 4 (default: bf16 maps of >= 64 channels, where it measured faster; NFP_TILE_DMA=1 / 0 force it on / off —
      // nfp_launch.h): channels-last, one thread per position, plain maps -> LDS-DMA into a position-major slab in the
      // storage type (nfp_tile.h::fwd_tile, DMA): PC =
      // 16-byte pieces per position and chunk, the largest power of two <= 8 that divides a pixel's pieces and fits (two
      // slabs when there are several chunks).
      bool dma = false;
      const int dma_sw = g_sw.tile_dma.load(std::memory_order_relaxed);
      const bool dma_auto = BF && (g.C * 2) % 128 == 0;   // (8 pieces per position and chunk: where it measured faster)
      if (!MF && R != 3 && (dma_sw == 1 || (dma_sw < 0 && dma_auto)) && M != nfp::kSymTerm && NHWC && !POOL && G == 1 && !g.gfc && (g.C * (BF ? 2 : 4)) % 16 == 0 &&
          !(((uintptr_t)x) & 15) && !((g.sB * (BF ? 2 : 4)) & 15)) {
        const int tp = g.C * (BF ? 2 : 4) / 16, npu64 = (npu + 63) & ~63;
        for (int lpc = 3; lpc >= 0; --lpc) {
          const int pc = 1 << lpc;
          if (tp % pc) continue;
          const size_t slabs = (size_t)(tp > pc ? 2 : 1) * npu64 * pc * 16;
          const size_t slack = (size_t)(R * Wu + R + 1) * pc * 16;   // (taps past the band read whatever lies there)
          if (slabs + tail + slack > budget) continue;
          g.Tc = lpc;
          g.Cc = pc * (BF ? 8 : 4);
          lds = slabs + tail + slack;
          dma = true;
          break;
        }
      }
      nfp::TileGeo tg = {nb, rows, Wu, ppb, 1, g.H / nb, g.H % nb, (int)(lds / 4)};
      if (t.nb) *t.nb = POOL ? nb * nfp::kPoolSub : nb;   // (pooled: rows of partial sums per image)
      snprintf(g_variant, sizeof(g_variant), "fwd_tile<R%d,%s,%s,%s%s%s>x%d", R, hot_name(g), MF ? "mix" : (BF ? "bf16" : "f32"),
               NHWC ? "nhwc" : "nchw", dma ? ",dma" : "", pool_tag(POOL), nb);
      const dim3 block(G, Wu, rows);
      // (tile_ids' exact range: batches beyond kTileMaxGrid workgroups go out as several launches, images in order)
      const int es = BF ? 2 : 4, oes = MF ? 4 : es, bmax = std::max(8, (tile_max_grid() / nb) & ~7);
      for (int b0 = 0; b0 < g.B; b0 += bmax) {
        KP gs = g;
        gs.B = std::min(bmax, g.B - b0);
        const dim3 grid((unsigned)(gs.B * nb));
        const void* xs = (const char*)x + (long long)b0 * g.sB * es;
        void* os = (char*)out + (long long)b0 * N * g.P * oes;
        float* ss = saved ? saved + (long long)b0 * g.P : nullptr;
        float* ps = t.part ? t.part + (long long)b0 * nb * nfp::kPoolSub * (g.C + NP) : nullptr;
        float* gs_ = t.gap ? t.gap + (long long)b0 * g.C : nullptr;
        float* ns_ = t.nfpm ? t.nfpm + (long long)b0 * N : nullptr;
        int rc;
        if (M == NFP_COSINE && g.gfc) {
          rc = launch("fwd_tile", fwd_tile<R, M, BF, NHWC, POOL, M == NFP_COSINE, false, MF>, grid, block, lds, st, gs, tg, xs, os, ss, ps, gs_, ns_);
        } else if (dma) {
          if constexpr (NHWC && !POOL && !MF && R != 3)   // (no LDS-DMA form at k = 7)
            rc = launch("fwd_tile_dma", fwd_tile<R, M, BF, true, false, false, true>, grid, block, lds, st, gs, tg, xs, os, ss, ps, gs_, ns_);
          else
            rc = kNotApplicable;
        } else {
          rc = launch("fwd_tile", fwd_tile<R, M, BF, NHWC, POOL, false, false, MF>, grid, block, lds, st, gs, tg, xs, os, ss, ps, gs_, ns_);
        }
        if (rc != NFP_OK) return rc;
      }
      return NFP_OK;
    }
  }
  return kNotApplicable;
}

}  // namespace

#ifdef NFP_TILE_R3_UNIT
int tile_forward_r3(const KP& g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t) {
#else
int tile_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t) {
#endif
  if (!tile_ok(g, x, x)) return kNotApplicable;
#ifndef NFP_TILE_R3_UNIT
  if (g.R == 3) return tile_forward_r3(g, x, out, saved, st, t);
#endif
  // (the symmetric-term measures below 14 x 14: the any-geometry forward spreads the same arithmetic over more threads:
  // [64,512,7,7] 9 vs 14 us; the backward wins at every size: 17.6-22.9 vs 20.9-28.6 us there — profiles/r04_zd_…)
  if (hot_sym(g) && g.P < 196) return kNotApplicable;
  return with_tile_radius(g, [&](auto r) { return with_hot<true>(g, [&](auto m) { return with_pool(t.mode, [&](auto p) {
    constexpr int R = decltype(r)::value, M = decltype(m)::value, POOL = decltype(p)::value;
    if constexpr (kHasTile<R, M, POOL>)
      return with_storage_mixed<R, M, POOL>(g, [&](auto bf, auto nhwc, auto mf) {
        return launch_fwd_tile_t<R, M, bf(), nhwc(), POOL, mf()>(g, x, out, saved, st, t);
      });
    else
      return kNotApplicable;
  }); }); });
}

#ifndef NFP_TILE_R3_UNIT
int tile_pool_fold(const KP& g, const float* part, float* gap, float* nfpm, int nb, hipStream_t st) {
  const long long n = (long long)g.B * (g.C + g.N);
  return launch("pool_fold", pool_fold<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, gap, nfpm, g.B, nb, g.C, g.N,
                g.invP);
}
#endif

}  // namespace nfp_host

#ifdef NFP_TILE_R3_UNIT
NFP_STAMP_SETTER(tile_r3_fwd)
#else
NFP_STAMP_SETTER(tile_fwd)
#endif
