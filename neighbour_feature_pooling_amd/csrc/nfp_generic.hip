// nfp_generic.hip — the any-geometry kernels of nfp_gather.h / nfp_direct.h and their launchers: every measure, every
// geometry, any map size (interface: nfp_launch.h::generic_forward / generic_backward / attn_softmax_*).
#include "nfp_launch.h"
#include "nfp_gather.h"
#include "nfp_direct.h"

using namespace nfp;

namespace nfp_host {
namespace {

// ---- generic launches -----------------------------------------------------------------------
// Forward of nfp_gather.h (fwd_pairs): one workgroup per (image, tile of outputs); declines only when not even
// one channel quad of the map fits next to its tables, then the chunked scalar kernel below serves the call.
bool force_scalar_fwd() { return g_sw.fwd_scalar.load(std::memory_order_relaxed) != 0; }

template <int M, int NN>
int launch_fwd_pairs_t(const KP& g, const void* x, void* out, float* saved, hipStream_t st) {
  constexpr int T = 512;
  const int Q = (g.C + 3) / 4;
  // output tiles: every CU busy at small batch; at most T outputs per tile, whole output rows when there are
  // several tiles per image anyway (a tile stages only the input rows it reads)
  int tiles = (256 + g.B - 1) / g.B;
  if (tiles > (g.O + 7) / 8) tiles = (g.O + 7) / 8;
  if (tiles < 1) tiles = 1;
  PairsLds L;
  L.Ot = (g.O + tiles - 1) / tiles;
  if (L.Ot > T) L.Ot = g.Wo <= T ? (T / g.Wo) * g.Wo : T;
  tiles = (g.O + L.Ot - 1) / L.Ot;
  // rows of x a tile can read: its output rows through stride / dilation, plus what padding folds back in
  // (inside that window when pad <= R*dilation; circular wraps and over-padding may reach anywhere)
  int rows = g.H;
  if (g.mode != NFP_PAD_CIRCULAR && g.pad <= g.R * g.dil) {
    const int orows = std::min(g.Ho, (L.Ot + g.Wo - 2) / g.Wo + 1);  // a tile may start and end mid-row
    rows = std::min(g.H, (orows - 1) * g.stride + 2 * g.R * g.dil + 1);
  }
  L.PSm = rows * g.W + 1;
  L.G = T / L.Ot;
  if (L.G > Q) L.G = Q;
  L.Gs = T / (L.PSm - 1);
  if (L.Gs > 16) L.Gs = 16;
  if (L.Gs > Q) L.Gs = Q;
  if (L.Gs < 1) L.Gs = 1;
  long long w = 0;
  L.st = (int)w;  w += 2LL * L.PSm;
  L.piv = (int)w; w += L.PSm;
  L.mm = (int)w;  w += 2;
  L.tap = (int)w; w += ((long long)(g.N + 1) * L.Ot + 1) / 2;
  L.red = (int)w; w += std::max((long long)L.G * NN * L.Ot, 2LL * L.Gs * (L.PSm - 1));
  w = (w + 3) & ~3LL;
  L.xs = (int)w;
  const long long quad_bytes = (long long)L.PSm * 16, room = (long long)kLdsMax - w * 4;
  if (room < quad_bytes) return kNotApplicable;
  long long Cq = room / quad_bytes;
  if (Cq > Q) Cq = Q;
  if (Cq < Q) {  // several chunks: make them even
    const long long nch = (Q + Cq - 1) / Cq;
    Cq = (Q + nch - 1) / nch;
  }
  L.Cq = (int)Cq;
  // wavefronts for the index tables vs the first slab: balance ~350*k clk per pass of 64 (output, kernel row)
  // items against ~2.5 B/clk of staging per wavefront (measured on MI355X, scripts/diag_stamps.py)
  double best = 1e30;
  L.Tt = 64;
  for (int nt = 1; nt <= 4; ++nt) {
    const double tt = (double)((L.Ot * g.k + 64 * nt - 1) / (64 * nt)) * 350.0 * g.k;
    const double ts = (double)Cq * (double)quad_bytes / ((T / 64 - nt) * 2.5);
    if (std::max(tt, ts) < best) {
      best = std::max(tt, ts);
      L.Tt = 64 * nt;
    }
  }
  const size_t lds = (size_t)w * 4 + (size_t)Cq * quad_bytes;
  snprintf(g_variant, sizeof(g_variant), "fwd_pairs");
  return launch("fwd_pairs", fwd_pairs<M, NN>, dim3(g.B, tiles), dim3(T), lds, st, g, L, x, out, saved);
}

template <int M>
int launch_fwd_pairs(const KP& g, const void* x, void* out, float* saved, hipStream_t st) {
  if (force_scalar_fwd() || g.P > 65534) return kNotApplicable;
  return g.N <= 8 ? launch_fwd_pairs_t<M, 8>(g, x, out, saved, st) : launch_fwd_pairs_t<M, 24>(g, x, out, saved, st);
}

template <int M>
int launch_fwd_generic(KP g, const void* x, void* out, float* saved, hipStream_t st) {
  if (int rc = launch_fwd_pairs<M>(g, x, out, saved, st); rc != kNotApplicable) return rc;
  // last resort (nfp_direct.h): no LDS tables, any map size
  snprintf(g_variant, sizeof(g_variant), "fwd_direct");
  return launch("fwd_direct", fwd_direct<M>, dim3((unsigned)((g.O + 255) / 256), (g.N + kGroup - 1) / kGroup, g.B), dim3(256),
                0, st, g, x, out, saved);
}

// Gather-form backward (nfp_gather.h): both kernels are one structure over bands of grad_x rows, bwd_gather with one
// band.  The tables + one slab of >= QB channel quads must fit in LDS and the packed indices must hold; otherwise
// nfp_direct.h::bwd_direct serves the call.
bool force_atomic() { return g_sw.bwd_atomic.load(std::memory_order_relaxed) != 0; }
// tests: NFP_BWD_BANDS=n sends every call through the banded kernel with >= n bands
int force_bands() { return g_sw.bwd_bands.load(std::memory_order_relaxed); }

#ifndef NFP_GATHER_WGS
#define NFP_GATHER_WGS 512
#endif
#ifndef NFP_GATHER_QB
#define NFP_GATHER_QB 4
#endif
#ifndef NFP_GATHER_SLAB_KB
#define NFP_GATHER_SLAB_KB 48
#endif

// index ranges the packed reader entries hold, whatever the bands (nfp_gather.h::axis_reader_raw, pack_reader)
bool gather_packs(const KP& g) {
  return g.k <= 15 && g.pad <= 8 && g.H < 16383 && g.W < 16383 && (long long)(g.H + g.W) * (2 * g.pad + 1) * g.k < (1 << 20);
}

// What the two launchers share, for bands of RB rows of grad_x whose tables hold at most ONm pairs and whose window
// holds at most PSm - 1 pixels: the reader-list capacities, the walk over the tables cf .. xc and the channel split;
// grid = (B, channel blocks, bands).  Returns the word offset behind xc — the launcher appends its own tables, then
// the slab — or -1 where the 16-bit pair / pixel indices do not hold.
long long gather_layout(const KP& g, int NC, int RB, long long ONm, long long PSm, GatherLds& L, dim3& grid) {
  constexpr int QB = NFP_GATHER_QB;
  if (ONm > 65535 || PSm > 65535) return -1;
  auto folds = [&](int n) {  // padded coordinates that can fold onto one coordinate of an axis of size n
    if (g.pad == 0 || g.mode == NFP_PAD_ZEROS) return 1;
    if (g.mode == NFP_PAD_REPLICATE) return n == 1 ? 2 * g.pad + 1 : g.pad + 1;
    return 3;
  };
  L.RB = RB;
  L.ONm = (int)ONm;
  L.PSm = (int)PSm;
  L.capY = g.k * folds(g.H);
  L.capX = g.k * folds(g.W);
  long long w = 0;
  L.cf = (int)w;  w += NC * ONm;
  L.nbq = (int)w; w += (ONm + 1) / 2;
  w = (w + 1) & ~1LL;  // uint2 lists
  L.yl = (int)w;  w += 2LL * RB * L.capY;
  L.xl = (int)w;  w += 2LL * g.W * L.capX;
  L.yc = (int)w;  w += RB;
  L.xc = (int)w;  w += g.W;
  // channel split: enough workgroups to fill the chip at small batch, whole QB blocks per workgroup
  const int Q = (g.C + 3) / 4, bands = (g.H + RB - 1) / RB, maxS = (Q + QB - 1) / QB;
  int S = (NFP_GATHER_WGS + g.B * bands - 1) / (g.B * bands);
  if (S > maxS) S = maxS;
  if (S < 1) S = 1;
  L.Qwg = (((Q + S - 1) / S) + QB - 1) / QB * QB;
  grid = dim3(g.B, (Q + L.Qwg - 1) / L.Qwg, bands);
  return w;
}

// One band: the slots have a table of their own, a quarter of the threads stage the first slab under the table build,
// and the slab is capped by a budget that keeps several workgroups per CU.
template <int M>
int launch_bwd_gather(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                      hipStream_t st) {
  constexpr int QB = NFP_GATHER_QB;
  if (force_bands() > 0 || !gather_packs(g)) return kNotApplicable;
  GatherLds L{};
  dim3 grid;
  long long w = gather_layout(g, NCoef<M>::v, g.H, (long long)g.O * g.N, (long long)g.P + 1, L, grid);
  if (w < 0) return kNotApplicable;
  w = (w + 1) & ~1LL;
  L.sl = (int)w;  w += 2LL * (g.H + g.W) * (2 * g.pad + 1) * g.k;
  w = (w + 3) & ~3LL;
  if (w * 4 > kLdsMax) return kNotApplicable;
  L.xs = (int)w;
  L.Ts = NFP_GATHER_T / 4;
  const size_t table_bytes = (size_t)w * 4, quad_bytes = (size_t)L.PSm * 16;
  if (table_bytes + QB * quad_bytes > (size_t)kLdsMax) return kNotApplicable;
  size_t budget = (size_t)NFP_GATHER_SLAB_KB * 1024;
  if (budget < QB * quad_bytes) budget = QB * quad_bytes;
  if (budget > (size_t)kLdsMax - table_bytes) budget = (size_t)kLdsMax - table_bytes;
  L.Cq = std::min((int)(budget / quad_bytes) / QB * QB, L.Qwg);
  const size_t lds = table_bytes + (size_t)L.Cq * quad_bytes;
  snprintf(g_variant, sizeof(g_variant), "bwd_gather");
  return launch("bwd_gather", bwd_gather<M, QB>, grid, dim3(NFP_GATHER_T), lds, st, g, L, x, go, out, saved, gx);
}

// Maps whose whole-image tables exceed LDS (nfp_gather.h::bwd_gather_banded): the fewest bands whose tables take at
// most half of LDS; the rest is the slab (at least one block of QB quads), which holds the slots first.
template <int M>
int launch_bwd_gather_banded(const KP& g, const void* x, const void* go, const void* out, const float* saved,
                             void* gx, hipStream_t st) {
  constexpr int QB = NFP_GATHER_QB;
  if (!gather_packs(g)) return kNotApplicable;
  const bool local = g.mode != NFP_PAD_CIRCULAR && g.pad <= g.R * g.dil;  // an output reads near its centre only
  const int reach = 2 * g.R * g.dil, nslot = (2 * g.pad + 1) * g.k;
  GatherLds L{};
  dim3 grid;
  size_t table_bytes = 0, quad_bytes = 0, slot_bytes = 0;
  bool found = false;
  const int nb0 = local ? std::min(std::max(force_bands(), 1), g.H) : 1;
  for (int nb = nb0; nb <= g.H && !found; nb = local ? nb + 1 : g.H + 1) {
    const int RB = (g.H + nb - 1) / nb;
    const int orows = local ? std::min(g.Ho, (RB - 1 + reach) / g.stride + 2) : g.Ho;
    const int wrows = local ? std::min(g.H, RB + reach) : g.H;
    long long w = gather_layout(g, NCoef<M>::v, RB, (long long)g.N * orows * g.Wo, (long long)wrows * g.W + 1, L, grid);
    if (w < 0) continue;
    L.mm = (int)w;  w += 4;
    w = (w + 3) & ~3LL;
    L.xs = (int)w;
    table_bytes = (size_t)w * 4;
    quad_bytes = (size_t)L.PSm * 16;
    slot_bytes = (size_t)(RB + g.W) * nslot * 8;
    found = table_bytes <= (size_t)kLdsMax / 2 && table_bytes + std::max(QB * quad_bytes, slot_bytes) <= (size_t)kLdsMax;
  }
  if (!found) return kNotApplicable;
  L.Cq = std::min((int)(((size_t)kLdsMax - table_bytes) / quad_bytes) / QB * QB, L.Qwg);
  const size_t lds = table_bytes + std::max((size_t)L.Cq * quad_bytes, slot_bytes);
  snprintf(g_variant, sizeof(g_variant), "bwd_gather_banded");
  return launch("bwd_gather_banded", bwd_gather_banded<M, QB>, grid, dim3(512), lds, st, g, L, x, go, out, saved, gx);
}

template <int M>
int launch_bwd_generic(KP g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                       hipStream_t st) {
  if (!force_atomic()) {
    if (int rc = launch_bwd_gather<M>(g, x, go, out, saved, gx, st); rc != kNotApplicable) return rc;
    if (int rc = launch_bwd_gather_banded<M>(g, x, go, out, saved, gx, st); rc != kNotApplicable) return rc;
  }
  // last resort (nfp_direct.h): no LDS tables, any map size, still one writer per element in a fixed order
  snprintf(g_variant, sizeof(g_variant), "bwd_direct");
  return launch("bwd_direct", bwd_direct<M>, dim3((unsigned)((g.P + 255) / 256), (g.C + kDirectCB - 1) / kDirectCB, g.B),
                dim3(256), 0, st, g, x, go, out, saved, gx);
}

}  // namespace

int generic_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st) {
  return with_measure(g, [&](auto m) { return launch_fwd_generic<m()>(g, x, out, saved, st); });
}

int generic_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st) {
  return with_measure(g, [&](auto m) { return launch_bwd_generic<m()>(g, x, go, out, saved, gx, st); });
}

int attn_softmax_forward(const KP& g, const float* dots, void* out, hipStream_t st) {
  const long long n = (long long)g.B * g.O;
  return launch("attn_softmax_fwd", attn_softmax_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, dots, out);
}

int attn_softmax_backward(const KP& g, const void* go, const void* out, float* gd, hipStream_t st) {
  const long long n = (long long)g.B * g.O;
  return launch("attn_softmax_bwd", attn_softmax_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, go, out, gd);
}

}  // namespace nfp_host

NFP_STAMP_SETTER(generic)
