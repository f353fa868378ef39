// nfp_tile_launch.h — sizing shared by the two launchers of the row-band kernels (nfp_tile_fwd.hip, nfp_tile_bwd.hip);
// tile_geometry / tile_ok, which the dispatcher asks too, are in nfp_launch.h.
#pragma once
#include "nfp_launch.h"
#include "nfp_tile.h"

namespace nfp_host {

// ---- row-band kernels on a padded slab (nfp_tile.h): "same" maps of any size, no tables ----------------------------
#ifndef NFP_TILE_WGS
#define NFP_TILE_WGS 512
#endif
#ifndef NFP_TILE_THREADS
#define NFP_TILE_THREADS 480   // threads per workgroup the band height aims at
#endif
#ifndef NFP_TILE_LDS_KB
#define NFP_TILE_LDS_KB 78     // per workgroup, so that two share a compute unit
#endif
inline int tile_wgs() { return g_sw.tile_wgs > 0 ? (int)g_sw.tile_wgs : NFP_TILE_WGS; }
#ifndef NFP_TILE_WGS_R3
#define NFP_TILE_WGS_R3 256    // k = 7, the backward's channel blocks: every extra block repeats a phase A over 2 x 48 maps — half
#endif                         // the target measured best at [64 / 128 / 192 / 256,512,7,7]: 86 / 108 / 171 / 151 us against 109 / 130 / 194 / 173
inline int tile_block_wgs(int R) { return g_sw.tile_wgs > 0 ? (int)g_sw.tile_wgs : (R == 3 ? NFP_TILE_WGS_R3 : NFP_TILE_WGS); }
inline size_t tile_lds() { return (size_t)(g_sw.tile_lds_kb > 0 ? (int)g_sw.tile_lds_kb : NFP_TILE_LDS_KB) * 1024; }
inline int tile_max_grid() { return g_sw.tile_max_grid > 0 ? std::min((int)g_sw.tile_max_grid, nfp::kTileMaxGrid) : nfp::kTileMaxGrid; }
inline int tile_cap(int dflt) { return g_sw.tile_cap > 0 ? std::min((int)g_sw.tile_cap, 1024) : dflt; }

// Bands.  Every band re-reads and re-sums its 2R halo rows, so rows per band >= 6R keeps that at a third; beyond that,
// SMALLER workgroups win (one thread per padded position: ~480 threads, three or four workgroups per compute unit
// overlapping each other's load / sum / store phases) — measured on the MultiStage maps at B = 256
// (profiles/r03_v_tile_launch_constants.jsonl): 112x112 best at 6 rows (912 threads), 56x56 at 6 (464), 28x28 at 14 (480).
// At least tile_wgs() workgroups on the chip; every band at least R + 1 rows (the ring rows a border pixel collects
// from lie in its own band's halo).  Returns the rows of the largest band, or 0.
inline int tile_bands(const KP& g, int rb_cap, int& nb) {
  if (rb_cap < std::min(g.H, g.R + 1)) return 0;
  const int nb_max = std::max(1, g.H / (g.R + 1));
  nb = std::max(ceil_div(g.H, rb_cap), std::min(nb_max, ceil_div(tile_wgs(), g.B)));
  if (nb > nb_max) return 0;
  return ceil_div(g.H, nb);
}
inline int tile_rows_wanted(const KP& g, int cap) {
  const int Wu = g.W + 2 * g.R;
  const int want = std::max(6 * g.R, NFP_TILE_THREADS / Wu - 2 * g.R);
  return std::max(1, std::min(std::min(g.H, cap / Wu - 2 * g.R), want));
}
// channel groups per position: one, unless the chip would be short of threads (small batches)
inline int tile_groups(const KP& g, int nb, int npu, int cap, int cq) {
  int lg = 0;
  while (lg < 5 && (2 << lg) * npu <= cap && (2 << lg) <= cq && (long long)g.B * nb * npu * (1 << lg) < 128LL * 1024) ++lg;
  return lg;
}

// Norm p = 1 (the class default, nfp.py:16; and EMD: make_kp) and the symmetric-term measures: plain maps only, and not
// at radius 3 (k = 7: the product and squared-difference families alone — tile_ok asks hot_measure there)
template <int R, int M, int POOL>
constexpr bool kHasTile = (M == NFP_COSINE || M == NFP_NORM) || (POOL == nfp::kPoolNone && R != 3);

// The radius of a row-band launch: 1 or 2 here; 3 in the units of its own (nfp_tile_r3_fwd.hip / nfp_tile_r3_bwd.hip, which
// compile this unit's launcher with NFP_TILE_R3_UNIT).  with_radius itself is shared with the table launchers, which have
// no k = 7 form.
template <typename F>
int with_tile_radius(const KP& g, F&& f) {
#ifdef NFP_TILE_R3_UNIT
  return f(Int<3>{});
#else
  return with_radius(g, f);
#endif
}

}  // namespace nfp_host
