// nfp_tile_bwd.hip — the row-band backward of nfp_tile.h (bwd_tile) with its launcher (interface: nfp_launch.h::tile_backward;
// sizing shared with the forward: nfp_tile_launch.h).
// Compiled twice, as nfp_tile_fwd.hip: nfp_tile_r3_bwd.hip includes it with NFP_TILE_R3_UNIT for radius 3 (tile_backward_r3).
#include "nfp_tile_launch.h"

using namespace nfp;

namespace nfp_host {
namespace {

template <int R, int M, bool BF, bool NHWC, int POOL = nfp::kPoolNone, bool MF = false>
int launch_bwd_tile_t(KP g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st,
                      const BwdTail& t) {
  constexpr int N = Win<R>::N, K2 = Win<R>::K2;
  const int Wu = g.W + 2 * R;
  for (int attempt = 0; attempt < 2; ++attempt) {
    // first choice: two workgroups per compute unit (k = 3: 64 registers, up to 1024 threads each; k = 5: 128, up to 512)
    // k = 7: 512 threads either time — the kernel's launch bound (nfp_tile.h; nfp_launch.h::tile_r3_geometry admits what fits it)
    const size_t budget = attempt == 0 ? tile_lds() : (size_t)kLdsMax;
    const int kCap = R == 3 ? std::min(tile_cap(nfp::kTileBwdCapR3), nfp::kTileBwdCapR3) : tile_cap((R == 1 || attempt == 1) ? 1024 : 512);
    for (int rb0 = tile_rows_wanted(g, kCap); rb0 >= 1; --rb0) {
      int nb = 1;
      const int rb = tile_bands(g, rb0, nb);
      if (rb < 1) break;
      const int rows = rb + 2 * R, npu = rows * Wu, PL = (rows + 2 * R) * Wu;
      const size_t fixed = (size_t)((PL + 3) & ~3) * 4;                       // ipn
      const size_t pv = (size_t)(N * PL + 4) * 4;                             // pair values, every plane with its zero rows; guard
      const size_t wr = 16 + (size_t)((rows * 2 * R + 2 * R * g.W) * K2 + 4 * K2) * 4;   // spare slot, ring rows (+ slack)
      if (fixed + pv > budget) continue;
      // channel blocks: enough workgroups to fill the chip when images x bands do not
      int S = ceil_div(tile_block_wgs(R), g.B * nb);
      if (S > g.C / 4) S = g.C / 4;
      if (S < 1) S = 1;
      g.Cwg = round4(ceil_div(g.C, S));
      S = ceil_div(g.C, g.Cwg);
      const int lg = tile_groups(g, nb * S, npu, kCap, g.Cwg / 4), G = 1 << lg;
      const int ppb = nfp::band_row_slots((npu + 3) & ~3, lg);
      constexpr size_t SB = BF ? 8 : 16;   // bytes of a slab slot (nfp_tile.h::Quad)
      if (fixed + wr + (size_t)ppb * SB > budget) continue;
      int ncq = (int)((budget - fixed - wr) / ((size_t)ppb * SB));
      ncq = std::min(ncq, std::min(nfp::Quad<BF>::KQ * G, g.Cwg / 4));
      if (ncq < 1) continue;
      const int total = g.Cwg / 4, nch = ceil_div(total, ncq);
      g.Cc = 4 * ceil_div(total, nch);
      g.G = G;
      g.Tc = -1;
      if (NHWC && G == 1) {
        g.Tc = (BF && ncq >= 8) ? 3 : (ncq >= 4 ? 2 : (ncq >= 2 ? 1 : 0));
        g.Cc = 4 << g.Tc;
      }
      const size_t lds = fixed + std::max(pv, (size_t)(g.Cc / 4) * ppb * SB + wr);
      nfp::TileGeo tg = {nb, rows, Wu, ppb, S, g.H / nb, g.H % nb, (int)(lds / 4)};
      const dim3 block(G, Wu, rows);
      // dense grad_x stores through LDS (nfp_tile.h, phase B): channels-last with one thread per position, pixels of 256
      // bytes and more (below, the scattered 16-byte stores of a pixel complete their cache lines soon enough: measured
      // at 96 / 160 bytes, profiles/r03_w_tile_backward_stores_ab.txt), workgroups of up to 640 threads (the variant
      // takes 96 registers: two such workgroups per compute unit)
      // (round 4, PMC: the scattered stores of bf16 pixels leave as partial sectors — WRITE_SIZE 2.6x the bytes of grad_x at
      // [256,24,56,56] bf16, profiles/r04_j_…; same-box A/B of the dense form per pixel size, profiles/r04_k_…: bf16 128-byte
      // pixels 123.6 -> 102.5 us, 80-byte 23.7 -> 20.9; 48-byte pixels and float32 below 256 bytes lose or tie)
#ifndef NFP_TILE_CST_MINB
#define NFP_TILE_CST_MINB (BF ? 80 : 256)
#endif
      // (k = 7: no dense form — the sizes that would take it are not among the measured ones)
      const bool cst = R != 3 && NHWC && G == 1 && g.C * (BF ? 2 : 4) >= NFP_TILE_CST_MINB && npu <= 640;
      snprintf(g_variant, sizeof(g_variant), "bwd_tile<R%d,%s,%s,%s%s%s>x%d", R, hot_name(g), MF ? "mix" : (BF ? "bf16" : "f32"),
               NHWC ? "nhwc" : "nchw", cst ? ",dense" : "", pool_tag(POOL), nb);
      const std::true_type T_;
      const std::false_type F_;
      const int es = BF ? 2 : 4, oes = MF ? 4 : es, bmax = std::max(8, (tile_max_grid() / (nb * S)) & ~7);
      for (int b0 = 0; b0 < g.B; b0 += bmax) {   // (tile_ids' exact range: see launch_fwd_tile_t)
        KP gs = g;
        gs.B = std::min(bmax, g.B - b0);
        const dim3 grid((unsigned)(gs.B * nb * S));
        const void* xs = (const char*)x + (long long)b0 * g.sB * es;
        const void* gos = go ? (const char*)go + (long long)b0 * N * g.P * oes : nullptr;
        const void* os = (const char*)out + (long long)b0 * N * g.P * oes;
        const float* ss = saved ? saved + (long long)b0 * g.P : nullptr;
        void* gxs = (char*)gx + (long long)b0 * g.gB * es;
        const float* ggs = t.ggap ? t.ggap + (long long)b0 * g.C : nullptr;
        const float* gns = t.gnfpm ? t.gnfpm + (long long)b0 * N : nullptr;
        auto go_ = [&](auto gfc, auto cstv) {
          return launch("bwd_tile", bwd_tile<R, M, BF, NHWC, POOL, decltype(gfc)::value, decltype(cstv)::value, MF>, grid, block, lds, st,
                        gs, tg, xs, gos, os, ss, gxs, ggs, gns);
        };
        int rc;
        if (M == NFP_COSINE && g.gfc) {
          if constexpr (M == NFP_COSINE) {
            if constexpr (NHWC && R != 3) rc = cst ? go_(T_, T_) : go_(T_, F_);
            else rc = go_(T_, F_);
          } else {
            rc = go_(F_, F_);
          }
        } else {
          if constexpr (NHWC && R != 3) rc = cst ? go_(F_, T_) : go_(F_, F_);
          else rc = go_(F_, F_);
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
int tile_backward_r3(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st,
                     const BwdTail& t) {
#else
int tile_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st,
                  const BwdTail& t) {
#endif
  if (!tile_ok(g, x, gx)) return kNotApplicable;
#ifndef NFP_TILE_R3_UNIT
  if (g.R == 3) return tile_backward_r3(g, x, go, out, saved, gx, st, t);
#endif
  return with_tile_radius(g, [&](auto r) { return with_hot<true>(g, [&](auto m) { return with_pool(t.mode, [&](auto p) {
    constexpr int R = decltype(r)::value, M = decltype(m)::value, POOL = decltype(p)::value;
    if constexpr (kHasTile<R, M, POOL>)   // (grad_out of kPoolGap is a map; grad(GAP) joins in the store)
      return with_storage_mixed<R, M, POOL>(g, [&](auto bf, auto nhwc, auto mf) {
        return launch_bwd_tile_t<R, M, bf(), nhwc(), POOL, mf()>(g, x, go, out, saved, gx, st, t);
      });
    else
      return kNotApplicable;
  }); }); });
}

}  // namespace nfp_host

#ifdef NFP_TILE_R3_UNIT
NFP_STAMP_SETTER(tile_r3_bwd)
#else
NFP_STAMP_SETTER(tile_bwd)
#endif
