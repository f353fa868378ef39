// nfp_hip.hip — C ABI of libnfp_hip.so (include/nfp.h) and kernel dispatch.
//
// Stands in for models/pooling/nfp.py::NFPPooling.forward (nfp.py:132-134) and its
// autograd backward.  gfx950 only; no CPU path lives here — the library fails
// loudly (NFP_E_HIP / NFP_E_UNSUPPORTED) rather than fall back.
#include "nfp_launch.h"
#include "nfp_fast.h"
#include "nfp_band.h"
#include "nfp_gather.h"
#include "nfp_mfma.h"
#include "nfp_direct.h"

using namespace nfp;
using namespace nfp_host;

namespace {

struct EnvInit {
  EnvInit() { read_env(); }
} g_env_init;

// Validate the descriptor the way nn.Conv2d / F.pad would and fill the kernel parameter block.
int make_kp(const nfp_desc* d, KP* g) {
  if (!d) return fail(NFP_E_INVALID, "null descriptor");
  if (d->B < 0 || d->C < 1 || d->H < 1 || d->W < 1) return fail(NFP_E_INVALID, "bad shape [%d,%d,%d,%d]", d->B, d->C, d->H, d->W);
  if (d->R < 1 || d->stride < 1 || d->dilation < 1 || d->pad < 0)
    return fail(NFP_E_INVALID, "bad conv geometry R=%d stride=%d dilation=%d pad=%d", d->R, d->stride, d->dilation, d->pad);
  if (d->pad_mode < 0 || d->pad_mode > 3) return fail(NFP_E_INVALID, "bad pad_mode %d", d->pad_mode);
  if (d->measure < 0 || d->measure >= NFP_MEASURE_COUNT) return fail(NFP_E_INVALID, "bad measure %d", d->measure);
  if (d->dtype != NFP_F32 && d->dtype != NFP_BF16) return fail(NFP_E_INVALID, "bad dtype %d", d->dtype);
  if (d->map_f32 != 0 && d->map_f32 != 1) return fail(NFP_E_INVALID, "bad map_f32 %d (0 or 1)", d->map_f32);
  if (d->map_f32 == 1 && d->dtype != NFP_BF16)
    return fail(NFP_E_INVALID, "map_f32 = 1 goes with dtype = NFP_BF16 (float32 storage already has float32 maps)");
  const int k = 2 * d->R + 1;
  const int span = d->dilation * (k - 1) + 1;
  if (d->H + 2 * d->pad < span || d->W + 2 * d->pad < span)
    return fail(NFP_E_INVALID, "kernel span %d exceeds padded input %dx%d", span, d->H + 2 * d->pad, d->W + 2 * d->pad);
  if (d->pad_mode == NFP_PAD_REFLECT && (d->pad >= d->H || d->pad >= d->W))
    return fail(NFP_E_INVALID, "reflect padding %d must be smaller than the input %dx%d", d->pad, d->H, d->W);
  if (d->pad_mode == NFP_PAD_CIRCULAR && (d->pad > d->H || d->pad > d->W))
    return fail(NFP_E_INVALID, "circular padding %d must not exceed the input %dx%d", d->pad, d->H, d->W);
  // LA.norm(ord=p) also takes inf, 0 and negative orders (max / count / min semantics): no kernel for those.
  if (d->measure == NFP_NORM && !(d->p > 0.f && d->p <= 3.0e38f))
    return fail(NFP_E_UNSUPPORTED, "norm order p=%g has no HIP kernel (finite p > 0 only)", (double)d->p);
  if (!(d->eps >= 0.f)) return fail(NFP_E_INVALID, "bad eps %g", (double)d->eps);
  memset(g, 0, sizeof(*g));
  g->B = d->B; g->C = d->C; g->H = d->H; g->W = d->W; g->P = d->H * d->W;
  g->R = d->R; g->k = k; g->N = k * k - 1; g->pad = d->pad; g->stride = d->stride; g->dil = d->dilation;
  g->rs = d->R;
  if (d->inner_R != 0) {
    // both radii from one pass (nfp_heads.py:80-118): the hot-path kernels only, radii (1, 2), "same" maps
    if (d->inner_R != 1 || d->R != 2 || d->pad != 2 || d->stride != 1 || d->dilation != 1)
      return fail(NFP_E_UNSUPPORTED, "multi-radius: radii (1, 2) with padding = R, stride 1, dilation 1 only");
    g->rs = 12;
    g->N = (k * k - 1) + 8;
  }
  g->mode = d->pad_mode;
  g->Ho = (d->H + 2 * d->pad - span) / d->stride + 1;
  g->Wo = (d->W + 2 * d->pad - span) / d->stride + 1;
  g->O = g->Ho * g->Wo;
  g->measure = d->measure; g->similarity = d->similarity != 0; g->diff = d->diff_weights != 0; g->dtype = d->dtype;
  // EMD (nfp.py:207-216) = -+ sum_c |centre - neighbour|: the pure-neighbour conv output subtracted from the centre by the
  // measure itself — value and autograd gradient (abs: sign, 0 at 0) are those of Norm p = 1 on the difference weights
  // (nfp.py:141-148: LA.norm(ord=1) = sum |.|, backward sgn), so every kernel serves it as that
  if (d->measure == NFP_EMD) { g->measure = NFP_NORM; g->diff = 1; }
  // map_f32 (the torch.autocast call): out / grad_out in float32 beside bf16 x / grad_x — nfp_launch.h::mixed_maps
  g->godtype = d->map_f32 ? NFP_F32 : d->dtype;
  g->odtype = d->map_f32 ? NFP_F32 : d->dtype;
  g->p = d->measure == NFP_EMD ? 1.f : d->p; g->eps = d->eps; g->q_scs = d->q_scs;
  g->sB = d->sxB; g->sC = d->sxC; g->sH = d->sxH; g->sW = d->sxW;
  g->gB = d->sgB != 0 ? d->sgB : d->sxB;
  // the descriptor's workspace: kTicketBytes of per-image arrival counters (pooled kernels with several row bands per
  // image: nfp_common.h::pool_last_band), then — for the table kernels' geometries — the constant tables
  g->tickets = (g_sw.pool_ticket.load(std::memory_order_relaxed) && d->B <= kTicketWords) ? (unsigned int*)d->ws : nullptr;
  g->ws = d->ws != nullptr ? (const unsigned char*)d->ws + kTicketBytes : nullptr;
  g->contig = (d->sxW == 1 && d->sxH == d->W && d->sxC == (int64_t)d->H * d->W) ? 1 : 0;
  g->invP = 1.0f / (float)g->P;
  g->invW = 1.0f / (float)g->W;
  g->invNQ = 1.0f / (float)((g->P >> 2) > 0 ? (g->P >> 2) : 1);
  g->invPT = 1.0f / (float)((g->P & 3) > 0 ? (g->P & 3) : 1);
  g->inv_eps = 1.0f / g->eps;
  // run-time constants of the hot-path kernels (nfp_common.h): products out = osa * s + osb, distances out = osa * sqrt(d2 * d2s)
  const bool prod = d->measure == NFP_COSINE || d->measure == NFP_DOT || d->measure == NFP_GFC;
  g->gfc = d->measure == NFP_GFC ? 1 : 0;
  g->gf = (float)g->gfc;
  g->ngf = 1.0f - g->gf;
  g->unit = d->measure == NFP_DOT ? 1 : 0;
  g->uf = (float)g->unit;
  g->nuf = 1.0f - g->uf;
  g->osa = prod ? (g->similarity ? 1.f : -1.f) : (g->similarity ? -1.f : 1.f);
  g->osb = (d->measure == NFP_COSINE && !g->similarity) ? 1.f : 0.f;
  g->pool_gap = g->pool_map = 1;
  g->d2s = d->measure == NFP_RMSE ? 1.0f / (float)d->C : 1.0f;
  g->zero0 = d->measure == NFP_RMSE ? 0 : 1;
  if (!(g->stride == 1 && g->dil == 1 && g->pad == g->R && g->mode != NFP_PAD_CIRCULAR && (g->R == 1 || g->R == 2) &&
        g->P <= kBwdThreads && g->P >= 4))
    g->ws = nullptr;   // (not a table geometry — fast_geometry below: its workspace holds the counters alone)
  // index arithmetic of the general kernels: coordinates in 15 bits, pair indices in 31
  if (d->H > 32767 || d->W > 32767 || (int64_t)g->P > (1 << 26) || (int64_t)g->N * g->O >= (1LL << 31) || d->B > 65535)
    return fail(NFP_E_UNSUPPORTED, "feature map [%d,%d,%d,%d] with k = %d exceeds the index range of the kernels", d->B,
                d->C, d->H, d->W, k);
  return NFP_OK;
}

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

// Gather-form backward (nfp_gather.h): tables + one slab of >= QB channel quads must fit in LDS and the
// packed 16-bit indices must hold; otherwise the LDS-atomic kernel below serves the call.
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

template <int M>
int launch_bwd_gather(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                      hipStream_t st) {
  constexpr int QB = NFP_GATHER_QB, NC = NCoef<M>::v;
  const long long ON = (long long)g.O * g.N;
  // index ranges the packed tables hold (nfp_gather.h)
  if (force_atomic() || force_bands() > 0 || ON > 65535 || g.P > 65534 || g.k > 15 || g.pad > 8 || g.H >= 16383 ||
      g.W >= 16383 || (long long)(g.H + g.W) * (2 * g.pad + 1) * g.k >= (1 << 20))
    return kNotApplicable;
  auto folds = [&](int n) {  // padded coordinates that can fold onto one coordinate of an axis of size n
    if (g.pad == 0 || g.mode == NFP_PAD_ZEROS) return 1;
    if (g.mode == NFP_PAD_REPLICATE) return n == 1 ? 2 * g.pad + 1 : g.pad + 1;
    return 3;
  };
  GatherLds L;
  L.ON = (int)ON;
  L.capY = g.k * folds(g.H);
  L.capX = g.k * folds(g.W);
  long long w = 0;
  L.cf = (int)w;  w += (long long)NC * L.ON;
  L.nbq = (int)w; w += (L.ON + 1) / 2;
  w = (w + 1) & ~1LL;  // uint2 lists
  L.yl = (int)w;  w += 2LL * g.H * L.capY;
  L.xl = (int)w;  w += 2LL * g.W * L.capX;
  L.yc = (int)w;  w += g.H;
  L.xc = (int)w;  w += g.W;
  w = (w + 1) & ~1LL;
  L.sl = (int)w;  w += 2LL * (g.H + g.W) * (2 * g.pad + 1) * g.k;
  w = (w + 3) & ~3LL;
  if (w * 4 > kLdsMax) return kNotApplicable;
  L.xs = (int)w;
  L.Ts = NFP_GATHER_T / 4;  // a quarter of the threads stage
  const size_t table_bytes = (size_t)w * 4, quad_bytes = (size_t)(g.P + 1) * 16;
  if (table_bytes + QB * quad_bytes > (size_t)kLdsMax) return kNotApplicable;
  const int Q = (g.C + 3) / 4;
  // channel split: enough workgroups to fill the chip at small batch, whole QB blocks per workgroup
  int S = (NFP_GATHER_WGS + g.B - 1) / g.B;
  const int maxS = (Q + QB - 1) / QB;
  if (S > maxS) S = maxS;
  if (S < 1) S = 1;
  L.Qwg = (((Q + S - 1) / S) + QB - 1) / QB * QB;
  S = (Q + L.Qwg - 1) / L.Qwg;
  // slab: what the workgroup needs, capped by a budget that keeps several workgroups per CU, then by LDS
  size_t budget = (size_t)NFP_GATHER_SLAB_KB * 1024;
  if (budget < QB * quad_bytes) budget = QB * quad_bytes;
  if (budget > (size_t)kLdsMax - table_bytes) budget = (size_t)kLdsMax - table_bytes;
  int Cq = (int)(budget / quad_bytes) / QB * QB;
  if (Cq > L.Qwg) Cq = L.Qwg;
  L.Cq = Cq;
  const size_t lds = table_bytes + (size_t)Cq * quad_bytes;
  snprintf(g_variant, sizeof(g_variant), "bwd_gather");
  return launch("bwd_gather", bwd_gather<M, QB>, dim3(g.B, S), dim3(NFP_GATHER_T), lds, st, g, L, x, go, out, saved, gx);
}

// Banded variant for maps whose whole-image tables exceed LDS (nfp_gather.h::bwd_gather_banded).
template <int M>
int launch_bwd_gather_banded(const KP& g, const void* x, const void* go, const void* out, const float* saved,
                             void* gx, hipStream_t st) {
  constexpr int QB = NFP_GATHER_QB, NC = NCoef<M>::v;
  if (force_atomic() || g.k > 15 || g.pad > 8 || g.H >= 16383 || g.W >= 16383 ||
      (long long)(g.H + g.W) * (2 * g.pad + 1) * g.k >= (1 << 20))
    return kNotApplicable;
  auto folds = [&](int n) {
    if (g.pad == 0 || g.mode == NFP_PAD_ZEROS) return 1;
    if (g.mode == NFP_PAD_REPLICATE) return n == 1 ? 2 * g.pad + 1 : g.pad + 1;
    return 3;
  };
  const bool local = g.mode != NFP_PAD_CIRCULAR && g.pad <= g.R * g.dil;  // an output reads near its centre only
  const int reach = 2 * g.R * g.dil, nslot = (2 * g.pad + 1) * g.k, Q = (g.C + 3) / 4;
  BandLds L;
  L.capY = g.k * folds(g.H);
  L.capX = g.k * folds(g.W);
  long long w = 0;
  size_t table_bytes = 0, quad_bytes = 0, slot_bytes = 0;
  int bands = 0;
  const int nb0 = local ? std::min(std::max(force_bands(), 1), g.H) : 1;
  for (int nb = nb0; nb <= g.H; nb = local ? nb + 1 : g.H + 1) {
    const int RB = (g.H + nb - 1) / nb;
    const int orows = local ? std::min(g.Ho, (RB - 1 + reach) / g.stride + 2) : g.Ho;
    const int wrows = local ? std::min(g.H, RB + reach) : g.H;
    const long long ONm = (long long)g.N * orows * g.Wo, PSm = (long long)wrows * g.W + 1;
    if (PSm > 65535) continue;
    w = 0;
    L.cf = (int)w;  w += NC * ONm;
    L.nbq = (int)w; w += (ONm + 1) / 2;
    w = (w + 1) & ~1LL;
    L.yl = (int)w;  w += 2LL * RB * L.capY;
    L.xl = (int)w;  w += 2LL * g.W * L.capX;
    L.yc = (int)w;  w += RB;
    L.xc = (int)w;  w += g.W;
    L.mm = (int)w;  w += 4;
    w = (w + 3) & ~3LL;
    table_bytes = (size_t)w * 4;
    quad_bytes = (size_t)PSm * 16;
    slot_bytes = (size_t)(RB + g.W) * nslot * 8;
    // tables may take half of LDS; the rest is the slab (at least one block of QB quads) or the slots
    if (table_bytes <= (size_t)kLdsMax / 2 && table_bytes + std::max(QB * quad_bytes, slot_bytes) <= (size_t)kLdsMax) {
      L.RB = RB;
      L.ONm = (int)ONm;
      L.PSm = (int)PSm;
      L.xs = (int)w;
      bands = (g.H + RB - 1) / RB;
      break;
    }
  }
  if (bands == 0) return kNotApplicable;
  int S = (NFP_GATHER_WGS + g.B * bands - 1) / (g.B * bands);
  const int maxS = (Q + QB - 1) / QB;
  if (S > maxS) S = maxS;
  if (S < 1) S = 1;
  L.Qwg = (((Q + S - 1) / S) + QB - 1) / QB * QB;
  S = (Q + L.Qwg - 1) / L.Qwg;
  size_t room = (size_t)kLdsMax - table_bytes;
  int Cq = (int)(room / quad_bytes) / QB * QB;
  if (Cq > L.Qwg) Cq = L.Qwg;
  L.Cq = Cq;
  const size_t lds = table_bytes + std::max((size_t)Cq * quad_bytes, slot_bytes);
  snprintf(g_variant, sizeof(g_variant), "bwd_gather_banded");
  return launch("bwd_gather_banded", bwd_gather_banded<M, QB>, dim3(g.B, S, bands), dim3(512), lds, st, g, L, x, go, out,
                saved, gx);
}

template <int M>
int launch_bwd_generic(KP g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                       hipStream_t st) {
  if (int rc = launch_bwd_gather<M>(g, x, go, out, saved, gx, st); rc != kNotApplicable) return rc;
  if (int rc = launch_bwd_gather_banded<M>(g, x, go, out, saved, gx, st); rc != kNotApplicable) return rc;
  // last resort (nfp_direct.h): no LDS tables, any map size, still one writer per element in a fixed order
  snprintf(g_variant, sizeof(g_variant), "bwd_direct");
  return launch("bwd_direct", bwd_direct<M>, dim3((unsigned)((g.P + 255) / 256), (g.C + kDirectCB - 1) / kDirectCB, g.B),
                dim3(256), 0, st, g, x, go, out, saved, gx);
}

// ---- fast-path launches (nfp_fast.h) ----------------------------------------------------------
#ifndef NFP_FWD_SLAB_KB
#define NFP_FWD_SLAB_KB 128
#endif
#ifndef NFP_BWD_SLAB_KB
#define NFP_BWD_SLAB_KB 60
#endif
constexpr int kSlabBudgetBwd = NFP_BWD_SLAB_KB * 1024;


// Geometry of the hot path: "same" maps (stride 1, dilation 1, pad = R) small enough for one workgroup per image.
// These are the descriptors that have workspace tables (nfp_tables.h).
bool fast_geometry(const KP& g) {
  if (g.stride != 1 || g.dil != 1 || g.pad != g.R || g.mode == NFP_PAD_CIRCULAR) return false;
  if (g.R != 1 && g.R != 2) return false;
  return g.P <= kBwdThreads && g.P >= 4;
}

// Which calls the hot-path kernels serve; everything else runs on the generic kernels.
// sym: also the five measures of nfp_measures.h::kSymTerm (plain single-radius maps only: their callers pass it)
bool fast_ok(const KP& g, const void* x, const void* gx, bool sym = false) {
  if (force_generic()) return false;
  if (!fast_geometry(g) || (g.C & 3)) return false;
  if (!hot_measure(g) && !hot_l1(g) && !(sym && hot_sym(g))) return false;
  const bool nhwc = g.sC == 1 && g.sW == g.C && g.sH == (long long)g.W * g.C;
  if (!g.contig && !nhwc) return false;
  if (!g.contig) {  // vector loads of 4 channels need natural alignment
    const uintptr_t m = g.dtype == NFP_F32 ? 15 : 7;
    const int es = g.dtype == NFP_F32 ? 4 : 2;
    if (((uintptr_t)x & m) || ((uintptr_t)gx & m) || ((g.sB * es) & m) || ((g.gB * es) & m)) return false;
  }
  return true;
}


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

// Row-banded forward (nfp_band.h): needs the descriptor's workspace tables.
#ifndef NFP_BAND_WGS
#define NFP_BAND_WGS 256
#endif
template <int R, int M, bool BF, bool NHWC, int POOL = kPoolNone, bool MF = false>   // MF: float32 maps beside bf16 x
int launch_fwd_band_t(KP g, const void* x, void* out, float* saved, hipStream_t st, float* gap = nullptr,
                      float* nfpm = nullptr, float* part = nullptr, int* nb_out = nullptr) {
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
  if (POOL && (part == nullptr || !(NFP_POOL_BANDS || g.tickets != nullptr))) nb = 1;
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
  if (nb_out) *nb_out = nb;
  // the kernel's preloadable head (nfp_common.h): what stands in front of its first x request
  const uint32_t sB_lo = (uint32_t)((unsigned long long)g.sB & 0xFFFFFFFFull), sB_hi = (uint32_t)((unsigned long long)g.sB >> 32);
  const uint32_t hchunk = nfp::band_head_chunk(g.Cc, lg, g.R, T), hgeom = nfp::band_head_geom(g.H, g.W, rb);
  // (NCHW staging: always the 4 x 4 blocks here.  The pixel-row form bwd_fast takes — launch_bwd_fast_t — was built for this
  // kernel too and measured no faster at the headline shape, 4.80 -> 4.86 us: profiles/r05_b_nchw_row_staging_ab.txt)
  auto go = [&](auto kernel) {
    if constexpr (NHWC)
      return launch("fwd_band", kernel, dim3(g.B, nb), dim3(T), lds, st, x, g.ws, sB_lo, sB_hi, g.C, hchunk, hgeom, out, saved,
                    gap, nfpm, part, g);
    else
      return launch_staged(false, "fwd_band", kernel, dim3(g.B, nb), dim3(T), lds, st, x, g.ws, sB_lo, sB_hi, g.C, hchunk,
                           hgeom, out, saved, gap, nfpm, part, g);
  };
  // (pooled, several bands: the bands' partial sums go to `part`; the caller folds them — pool_forward_rm)
  if constexpr (M != kSymTerm)
  if (g.unit || g.gfc || g.d2s != 1.f)   // DotProduct / GFC / RMSE: the finalize with the run-time constants
    return go(fwd_band<R, M, BF, NHWC, POOL, true, MF>);
  return go(fwd_band<R, M, BF, NHWC, POOL, false, MF>);
}

template <int R, int M, int POOL = kPoolNone>
int launch_fwd_band(const KP& g, const void* x, void* out, float* saved, hipStream_t st, float* gap = nullptr,
                    float* nfpm = nullptr, float* part = nullptr, int* nb_out = nullptr) {
  if (g.ws == nullptr) return kNotApplicable;
  return with_storage_mixed<R, M, POOL>(g, [&](auto bf, auto nhwc, auto mf) {
    return launch_fwd_band_t<R, M, bf(), nhwc(), POOL, mf()>(g, x, out, saved, st, gap, nfpm, part, nb_out);
  });
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
                      hipStream_t st, const float* ggap = nullptr, const float* gnfpm = nullptr) {
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
                           saved, g.ws, hgeom, g.C, g.Cwg, g.Cc, gx, ggap, gnfpm, g);
  }
  if constexpr (!NHWC)
    return launch_staged(false, "bwd_fast", bwd_fast<R, M, BF, NHWC, POOL, 0, false, MF>, dim3(g.B, S), dim3(T), lds, st, x, go, out, saved,
                         g.ws, hgeom, g.C, g.Cwg, g.Cc, gx, ggap, gnfpm, g);
  else
    return launch("bwd_fast", bwd_fast<R, M, BF, NHWC, POOL, 0, false, MF>, dim3(g.B, S), dim3(T), lds, st, x, go, out, saved, g.ws, hgeom,
                  g.C, g.Cwg, g.Cc, gx, ggap, gnfpm, g);
}

// Matrix-core forward (nfp_mfma.h): bf16, dense channels-last, C a multiple of 16.
bool mfma_enabled() { return g_sw.mfma.load(std::memory_order_relaxed) != 0; }

template <int R, int M>
int launch_fwd_gram(const KP& g, const void* x, void* out, float* saved, hipStream_t st, float* gap = nullptr,
                    float* nfpm = nullptr) {
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

// Phase B of the backward on the matrix cores (nfp_fast.h::bwd_gemm_phase): bf16 storage, C a multiple of 32.
template <int R, int M, bool NHWC, int POOL = kPoolNone>
int launch_bwd_gemm_t(KP g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                      hipStream_t st, const float* ggap = nullptr, const float* gnfpm = nullptr) {
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
                    g.ws, nfp::bwd_head_geom(g.P, g.mode, g.unit, g.G, T), g.C, g.Cwg, g.Cc, gx, ggap, gnfpm, g);
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
                g.ws, nfp::bwd_head_geom(g.P, g.mode, g.unit, g.G, T), g.C, g.Cwg, g.Cc, gx, ggap, gnfpm, g);
}

// The table backward: phase B on the matrix cores where that form exists (bf16 maps, one radius, cosine / L2) and applies,
// else the vector (VALU) form, which serves every radius spec.  (float32 maps beside bf16 x: the vector form — the
// matrix-core backward stages grad_out / out under an LDS budget sized for 2-byte values.)
template <int R, int M, int POOL = kPoolNone>
int launch_bwd_fast(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                    hipStream_t st, const float* ggap = nullptr, const float* gnfpm = nullptr) {
  return with_storage_mixed<R, M, POOL>(g, [&](auto bf, auto nhwc, auto mf) {
    if constexpr (bf() && !mf() && R != 12 && (M == NFP_COSINE || M == NFP_NORM))
      if (int rc = launch_bwd_gemm_t<R, M, nhwc(), POOL>(g, x, go, out, saved, gx, st, ggap, gnfpm); rc != kNotApplicable)
        return rc;
    return launch_bwd_fast_t<R, M, bf(), nhwc(), POOL, mf()>(g, x, go, out, saved, gx, st, ggap, gnfpm);
  });
}

}  // namespace

#ifdef NFP_STAMPS
extern "C" int nfp_debug_set_stamp_buffer_tile(void* dev_ptr);
extern "C" int nfp_debug_set_stamp_buffer(void* dev_ptr) {
  unsigned long long* p = (unsigned long long*)dev_ptr;
  if (int rc = nfp_debug_set_stamp_buffer_tile(dev_ptr)) return rc;
  return hip_ok(hipMemcpyToSymbol(HIP_SYMBOL(nfp::nfp_stamp_buf), &p, sizeof(p)), "set stamp buffer");
}
#endif

extern "C" {

int nfp_abi_version(void) { return NFP_ABI_VERSION; }
const char* nfp_last_error(void) { return g_err; }
const char* nfp_last_variant(void) {
  std::lock_guard<std::mutex> lock(g_variant_mu);
  memcpy(t_variant_out, g_variant_last, sizeof(t_variant_out));
  return t_variant_out;
}
void nfp_reload_env(void) { read_env(); }
void nfp_time_next_launch(void* start_event, void* stop_event) {
  g_time_stop.store(stop_event);
  g_time_start.store(start_event);
}
uint64_t nfp_launch_count(void) { return g_launches.load(); }

int nfp_output_shape(const nfp_desc* d, int32_t* N, int32_t* Ho, int32_t* Wo) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (N) *N = g.N;
  if (Ho) *Ho = g.Ho;
  if (Wo) *Wo = g.Wo;
  return NFP_OK;
}

int64_t nfp_saved_floats(const nfp_desc* d) {
  KP g;
  if (make_kp(d, &g)) return -1;
  if (g.measure == NFP_ATTENTION) return (int64_t)g.B * g.N * g.O;  // backward scratch: grad wrt the dots
  return (int64_t)stats_of(g.measure) * g.B * g.P;
}

}  // extern "C"

#ifndef NFP_SYM_TABLE_BWD
#define NFP_SYM_TABLE_BWD 1   // 0 = the five kSymTerm measures keep the row-band backward below 512 pixels too (A/B)
#endif
namespace {

// What leaves the library is 0 or a negative NFP_E_* code: a launcher's internal "not applicable" can only mean
// that no kernel serves the descriptor.
int finish(int rc, const char* what) {
  if (rc == kNotApplicable) return fail(NFP_E_UNSUPPORTED, "%s: no kernel serves this descriptor", what);
  if (rc == NFP_OK && !t_dry) publish_variant();
  return rc;
}

// The hot-path forward of a plain single-radius map, or kNotApplicable: table kernels (matrix cores first for bf16), then the
// row-band kernels.
int hot_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st) {
  if (g_sw.tile_first.load(std::memory_order_relaxed))
    if (int rc = tile_forward(g, x, out, saved, st, false, nullptr, nullptr, nullptr, nullptr); rc != kNotApplicable) return rc;
  // (Geman / Canberra / Hellinger / Jeffrey / squared chord / chi-squared 1 share the kSymTerm instantiation)
  if (fast_ok(g, x, x, true)) {
    const int rc = with_radius(g, [&](auto r) {
      return with_hot<true>(g, [&](auto m) {
        constexpr int R = decltype(r)::value, M = decltype(m)::value;
        if constexpr (M == NFP_COSINE || M == NFP_NORM)   // the matrix-core forward has these two forms alone
          if (int rc = launch_fwd_gram<R, M>(g, x, out, saved, st); rc != kNotApplicable) return rc;
        return launch_fwd_band<R, M>(g, x, out, saved, st);
      });
    });
    if (rc != kNotApplicable) return rc;
  }
  // maps above the table kernels' 512 pixels, or a descriptor without its tables: the row-band kernels (nfp_tile.hip)
  if (int rc = tile_forward(g, x, out, saved, st, false, nullptr, nullptr, nullptr, nullptr); rc != kNotApplicable) return rc;
  return kNotApplicable;
}

// Attention (nfp.py:195-205) = DotProduct's sums + a softmax over the neighbours: the descriptor's parameter block as
// DotProduct's (make_kp's run-time constants of the hot-path kernels), raw dots in float32
KP as_dot(const KP& g) {
  KP d = g;
  d.measure = NFP_DOT;
  d.similarity = 1;   // raw dots first; the sign belongs to the softmax output (nfp.py:203-204)
  d.diff = 0;
  d.gfc = 0; d.gf = 0.f; d.ngf = 1.f;
  d.unit = 1; d.uf = 1.f; d.nuf = 0.f;
  d.osa = 1.f; d.osb = 0.f; d.d2s = 1.f; d.zero0 = 1;
  d.odtype = NFP_F32;
  return d;
}

// map_f32 descriptors nfp_forward / nfp_backward do not serve (include/nfp.h): the caller keeps its float32 copy of x
int mixed_refused(const nfp_desc* d) {
  if (!d->map_f32) return NFP_OK;
  if (d->inner_R != 0 || d->measure == NFP_ATTENTION || d->measure == NFP_SCS)
    return fail(NFP_E_UNSUPPORTED, "map_f32: one radius, every measure but Attention / SharpenedCosine");
  return NFP_OK;
}

int forward_impl(const nfp_desc* d, const void* x, void* out, float* saved, void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (!x || !out) return fail(NFP_E_INVALID, "null tensor pointer");
  if (int rc = mixed_refused(d)) return rc;
  if (g.B == 0) return NFP_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  if (g.rs == 12) {
    if (g.ws == nullptr || !fast_ok(g, x, x))
      return fail(NFP_E_UNSUPPORTED, "multi-radius: cosine / dot / gfc / L2 / rmse / norm p=1 / emd on maps of at most %d pixels, "
                  "C %% 4 == 0, dense layout, descriptor with a workspace", kBwdThreads);
    const int rc = with_hot<true>(g, [&](auto m) {
      if constexpr (m() == kSymTerm) return kNotApplicable;   // (fast_ok above has refused these)
      else return launch_fwd_band<12, m()>(g, x, out, saved, st);
    });
    return rc == kNotApplicable ? fail(NFP_E_UNSUPPORTED, "multi-radius: the map does not fit the hot-path forward") : rc;
  }
  if (int rc = hot_forward(g, x, out, saved, st); rc != kNotApplicable) return rc;
  if (g.measure == NFP_ATTENTION) {
    // raw dots in f32: in `out` itself for float32 maps, in the caller's scratch (nfp_saved_floats) for bf16
    if (g.dtype != NFP_F32 && !saved)
      return fail(NFP_E_INVALID, "attention on bf16 maps needs the scratch of nfp_saved_floats (also without a backward)");
    float* dots = g.dtype == NFP_F32 ? (float*)out : saved;
    const KP gd = as_dot(g);
    // float32 maps: DotProduct's hot-path kernels write the raw dots (round 4; bf16 maps keep float32 dots in the scratch, which
    // only the any-geometry kernels write)
    int rc = g.dtype == NFP_F32 ? hot_forward(gd, x, dots, nullptr, st) : kNotApplicable;
    if (rc == kNotApplicable) rc = launch_fwd_generic<NFP_DOT>(gd, x, dots, nullptr, st);
    if (rc) return rc;
    const long long n = (long long)g.B * g.O;
    variant_suffix("+attn_softmax");
    return launch("attn_softmax_fwd", attn_softmax_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g,
                  (const float*)dots, out);
  }
  const int rc = with_measure(g, [&](auto m) { return launch_fwd_generic<m()>(g, x, out, saved, st); });
  if (rc == kNotApplicable)
    return fail(NFP_E_UNSUPPORTED, "measure %d (SharpenedCosine mixes batch elements in the reference, "
                "nfp.py:359-374) has no HIP kernel", g.measure);
  return rc;
}

// The hot-path backward of a plain single-radius map, or kNotApplicable (as hot_forward).
int hot_backward(const KP& g, const void* x, const void* grad_out, const void* out, const float* saved, void* grad_x,
                 hipStream_t st) {
  if (g_sw.tile_first.load(std::memory_order_relaxed))
    if (int rc = tile_backward(g, x, grad_out, out, saved, grad_x, st, false, nullptr, nullptr); rc != kNotApplicable) return rc;
  // k = 5, float32 NCHW, maps of 14 x 14 and more: the row-band backward (window weights in registers, no 13-entry-per-pixel
  // gather phase) beats the table kernel — [256,192,14,14] L2 40.9 -> 35.7 us, cosine 41.1 -> 37.1, [256,256,14,14] 50.5 ->
  // 44.1 (profiles/r04_n_…; the FORWARD stays on the tables: 19 vs 28 us; channels-last and bf16 stay too).  Same saved
  // state (the map and |x| per pixel), so the two mix.
  if (g.R == 2 && g.rs != 12 && g.dtype == NFP_F32 && g.contig && g.P >= 196 && hot_measure(g))
    if (int rc = tile_backward(g, x, grad_out, out, saved, grad_x, st, false, nullptr, nullptr); rc != kNotApplicable) return rc;
  // The table kernels.  The kSymTerm measures only below 14 x 14: from there up the row-band backward is ahead ([256,192,14,14]
  // k = 5 97.5 vs 101.9 us, [256,64,20,20] 37.5 vs 41.4; at 7 x 7 the table kernel: [64,512,7,7] 10.1-12.3 vs 18.2-22.5 us —
  // profiles/r04_zd_…; the forward stays on the tables up to 512 pixels: 52.7 vs 66.8 us at [256,192,14,14])
  if (g.ws != nullptr && fast_ok(g, x, grad_x, true) && !(hot_sym(g) && !(NFP_SYM_TABLE_BWD && g.P < 196))) {
    const int rc = with_radius(g, [&](auto r) {
      return with_hot<true>(g, [&](auto m) { return launch_bwd_fast<decltype(r)::value, m()>(g, x, grad_out, out, saved, grad_x, st); });
    });
    if (rc != kNotApplicable) return rc;
  }
  if (int rc = tile_backward(g, x, grad_out, out, saved, grad_x, st, false, nullptr, nullptr); rc != kNotApplicable) return rc;
  return kNotApplicable;
}

int backward_impl(const nfp_desc* d, const void* x, const void* grad_out, const void* out, const float* saved,
                  void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (!x || !grad_out || !out || !grad_x) return fail(NFP_E_INVALID, "null tensor pointer");
  if ((stats_of(g.measure) > 0 || g.measure == NFP_ATTENTION) && !saved) return fail(NFP_E_INVALID, "measure %d needs the saved state of nfp_forward", g.measure);
  if (int rc = mixed_refused(d)) return rc;
  if (g.B == 0) return NFP_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  if (g.rs == 12) {
    if (g.ws == nullptr || !fast_ok(g, x, grad_x))
      return fail(NFP_E_UNSUPPORTED, "multi-radius: cosine / dot / gfc / L2 / rmse / norm p=1 / emd on maps of at most %d pixels, "
                  "C %% 4 == 0, dense layout, descriptor with a workspace", kBwdThreads);
    const int rc = with_hot<true>(g, [&](auto m) {
      if constexpr (m() == kSymTerm) return kNotApplicable;   // (fast_ok above has refused these)
      else return launch_bwd_fast<12, m()>(g, x, grad_out, out, saved, grad_x, st);
    });
    return rc == kNotApplicable ? fail(NFP_E_UNSUPPORTED, "multi-radius: the map does not fit the hot-path backward") : rc;
  }
  if (int rc = hot_backward(g, x, grad_out, out, saved, grad_x, st); rc != kNotApplicable) return rc;
  if (g.measure == NFP_ATTENTION) {
    float* gd = const_cast<float*>(saved);  // scratch handed over by nfp_forward's caller (nfp_saved_floats)
    const long long n = (long long)g.B * g.O;
    if (int rc = launch("attn_softmax_bwd", attn_softmax_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g,
                        grad_out, out, gd))
      return rc;
    KP gdot = as_dot(g);
    gdot.odtype = g.odtype;
    gdot.godtype = NFP_F32;
    // float32 maps: DotProduct's hot-path backward on the gradient with respect to the dots (it keeps no saved state: `out` is
    // only read in bounds)
    if (g.dtype == NFP_F32) {
      if (int rc = hot_backward(gdot, x, gd, out, nullptr, grad_x, st); rc != kNotApplicable) return rc;
    }
    return launch_bwd_generic<NFP_DOT>(gdot, x, gd, out, nullptr, grad_x, st);
  }
  const int rc = with_measure(g, [&](auto m) { return launch_bwd_generic<m()>(g, x, grad_out, out, saved, grad_x, st); });
  if (rc == kNotApplicable) return fail(NFP_E_UNSUPPORTED, "measure %d (SharpenedCosine) has no HIP kernel", g.measure);
  return rc;
}

// Floats of scratch behind the per-pixel state in `saved` that the row-band pooled forward needs: every band's share of
// the two pooled sums (nfp_tile.h::fwd_tile<POOL> -> pool_fold).  Set by pool_forward_rm (also in plan mode).
thread_local long long t_pool_scratch = 0;

template <int R, int M>
int pool_forward_rm(const KP& g, const void* x, void* out_map, float* saved, hipStream_t st, float* gap, float* nfpm) {
  t_pool_scratch = 0;
  if (g.ws != nullptr && fast_ok(g, x, x)) {
    // the matrix-core forward where it applies, as in nfp_forward (it declines float32 storage itself)
    if (int rc = launch_fwd_gram<R, M>(g, x, out_map, saved, st, gap, nfpm); rc != kNotApplicable) return rc;
    // row bands at small batches: each band's share of the pooled sums goes to the scratch behind the norms
    float* part = saved != nullptr ? saved + (long long)stats_of(g.measure) * g.B * g.P : nullptr;
    int nb = 1;
    const int rc = launch_fwd_band<R, M, kPoolBoth>(g, x, out_map, saved, st, gap, nfpm, part, &nb);
    if (rc == NFP_OK && nb > 1) {
      t_pool_scratch = (long long)g.B * nb * (g.C + g.N);
      if (g.tickets != nullptr) return rc;   // (the last band to arrive folded them inside the launch)
      variant_suffix("+pool_fold");
      return tile_pool_fold(g, part, gap, nfpm, nb, st);
    }
    if (rc != kNotApplicable) return rc;
  }
  if (!tile_ok(g, x, x)) return kNotApplicable;
  // row bands (any map size): per-band partial sums into the scratch behind the norms, joined by pool_fold
  if (saved == nullptr) return fail(NFP_E_INVALID, "fused pooling tail on this map needs the scratch of nfp_pool_saved_floats");
  float* part = saved + (long long)stats_of(g.measure) * g.B * g.P;
  int nb = 0;
  if (int rc = tile_forward(g, x, out_map, saved, st, kPoolBoth, part, &nb, gap, nfpm); rc != NFP_OK) return rc;
  t_pool_scratch = (long long)g.B * nb * (g.C + g.N);
  if (g.tickets != nullptr) return NFP_OK;   // (single launch: the last band to arrive folds, nfp_common.h::pool_last_band)
  variant_suffix("+pool_fold");
  return tile_pool_fold(g, part, gap, nfpm, nb, st);
}
template <int R, int M>
int pool_backward_rm(const KP& g, const void* x, const void* out_map, const float* saved, void* gx, hipStream_t st,
                     const float* ggap, const float* gnfpm) {
  if (g.ws != nullptr && fast_ok(g, x, gx))
    if (int rc = launch_bwd_fast<R, M, kPoolBoth>(g, x, nullptr, out_map, saved, gx, st, ggap, gnfpm); rc != kNotApplicable) return rc;
  return tile_backward(g, x, nullptr, out_map, saved, gx, st, kPoolBoth, ggap, gnfpm);
}

// ---- GAP(x) beside the maps (nfp_gap_*): the pass of an NFP head (nfp_heads.py: gap(fmap) and nfp(fmap) of one feature map) ----
// Forward: the pooled kernels' channel sums without their map sums (kPoolGap); several bands per image write rows of C
// partial sums to the scratch behind the norms, joined in band order by pool_fold — never by the arrival counters (no
// atomics on this path).  Backward: grad_out read as a map, ggap[b,c] / P added in the same store.
// bf16: fwd_gram (its channel sums are a run-time option) and the matrix-core backwards serve this mode as well.
// R = 12 (radii 1 and 2 from one pass, MultiRadiusNFPHead): the table kernels alone — the two-radius window has no
// matrix-core and no row-band form, so bf16 runs on the vector kernels (as nfp_forward's) and maps above 512 pixels are
// not served; one band per image (no counters on this path), so no pool_fold launch either.
template <int R, int M>
int gap_forward_rm(KP g, const void* x, void* out_map, float* saved, hipStream_t st, float* gap) {
  t_pool_scratch = 0;
  g.tickets = nullptr;
  g.pool_gap = g.pool_map = 1;
  if (saved == nullptr) return fail(NFP_E_INVALID, "GAP beside the maps needs the scratch of nfp_gap_saved_floats");
  float* part = saved + (long long)stats_of(g.measure) * g.B * g.P;
  KP gfold = g;
  gfold.N = 0;   // (rows of C floats: pool_fold joins the channel sums alone)
  if (g.ws != nullptr && fast_ok(g, x, x)) {
    if constexpr (R != 12)
      if (int rc = launch_fwd_gram<R, M>(g, x, out_map, saved, st, gap, nullptr); rc != kNotApplicable) return rc;
    int nb = 1;
    const int rc = launch_fwd_band<R, M, kPoolGap>(g, x, out_map, saved, st, gap, nullptr, part, &nb);
    if (rc == NFP_OK && nb > 1) {
      t_pool_scratch = (long long)g.B * nb * g.C;
      variant_suffix("+pool_fold");
      return tile_pool_fold(gfold, part, gap, nullptr, nb, st);
    }
    if (rc != kNotApplicable) return rc;
  }
  if (R == 12 || !tile_ok(g, x, x)) return kNotApplicable;
  int nb = 0;
  if (int rc = tile_forward(g, x, out_map, saved, st, kPoolGap, part, &nb, gap, nullptr); rc != NFP_OK) return rc;
  t_pool_scratch = (long long)g.B * nb * g.C;
  variant_suffix("+pool_fold");
  return tile_pool_fold(gfold, part, gap, nullptr, nb, st);
}
template <int R, int M>
int gap_backward_rm(KP g, const void* x, const void* go, const void* out_map, const float* saved, void* gx, hipStream_t st,
                    const float* ggap) {
  g.pool_gap = ggap != nullptr ? 1 : 0;   // NULL: GAP(x) took no part in the loss — nothing is added, nothing is read
  if (g.ws != nullptr && fast_ok(g, x, gx))
    if (int rc = launch_bwd_fast<R, M, kPoolGap>(g, x, go, out_map, saved, gx, st, ggap, nullptr); rc != kNotApplicable) return rc;
  if (R == 12) return kNotApplicable;
  return tile_backward(g, x, go, out_map, saved, gx, st, kPoolGap, ggap, nullptr);
}

// the four of them by the descriptor's radius and family; the gap calls also take radii (1, 2) together (inner_R = 1)
int pool_forward(const KP& g, const void* x, void* out_map, float* saved, hipStream_t st, float* gap, float* nfpm) {
  return with_radius(g, [&](auto r) {
    return with_hot(g, [&](auto m) { return pool_forward_rm<decltype(r)::value, m()>(g, x, out_map, saved, st, gap, nfpm); });
  });
}
int pool_backward(const KP& g, const void* x, const void* out_map, const float* saved, void* gx, hipStream_t st,
                  const float* ggap, const float* gnfpm) {
  return with_radius(g, [&](auto r) {
    return with_hot(g, [&](auto m) { return pool_backward_rm<decltype(r)::value, m()>(g, x, out_map, saved, gx, st, ggap, gnfpm); });
  });
}
int gap_forward(const KP& g, const void* x, void* out_map, float* saved, hipStream_t st, float* gap) {
  return with_radius<true>(g, [&](auto r) {
    return with_hot(g, [&](auto m) { return gap_forward_rm<decltype(r)::value, m()>(g, x, out_map, saved, st, gap); });
  });
}
int gap_backward(const KP& g, const void* x, const void* go, const void* out_map, const float* saved, void* gx,
                 hipStream_t st, const float* ggap) {
  return with_radius<true>(g, [&](auto r) {
    return with_hot(g, [&](auto m) { return gap_backward_rm<decltype(r)::value, m()>(g, x, go, out_map, saved, gx, st, ggap); });
  });
}

}  // namespace

extern "C" {

// Exact maximum number of (pixel, tap) pairs linking two pixels, by enumeration on the host: the link rows of the
// workspace have the fixed width ws_link_width(); a geometry that would overflow it gets no tables.
static int max_links(const KP& g) {
  auto fold = [&](int v, int n) {
    const bool lo = v < 0, hi = v >= n;
    if (!lo && !hi) return v;
    if (g.mode == NFP_PAD_REFLECT) return lo ? -v : 2 * (n - 1) - v;
    if (g.mode == NFP_PAD_REPLICATE) return lo ? 0 : n - 1;
    return -1;
  };
  const int K = g.k, R = g.R;
  // per axis: cnt[a][b] = taps d in [-R, R] with fold(a + d) == b
  auto axis = [&](int n, int rad, std::vector<int>& cnt) {
    cnt.assign((size_t)n * n, 0);
    for (int a = 0; a < n; ++a)
      for (int dd = -rad; dd <= rad; ++dd) {
        const int f = fold(a + dd, n);
        if (f >= 0) cnt[(size_t)a * n + f]++;
      }
  };
  std::vector<int> cy, cx, iy, ix;  // taps of the window radius; of the inner radius 1 when both are produced
  axis(g.H, R, cy);
  axis(g.W, R, cx);
  if (g.rs == 12) {
    axis(g.H, 1, iy);
    axis(g.W, 1, ix);
  }
  int best = 0;
  for (int ry = 0; ry < g.H; ++ry)
    for (int ty = std::max(0, ry - R); ty <= std::min(g.H - 1, ry + R); ++ty)
      for (int rx = 0; rx < g.W; ++rx)
        for (int tx = std::max(0, rx - R); tx <= std::min(g.W - 1, rx + R); ++tx) {
          if (ry == ty && rx == tx) continue;
          int n = cy[(size_t)ry * g.H + ty] * cx[(size_t)rx * g.W + tx]     // taps of r that read t
                  + cy[(size_t)ty * g.H + ry] * cx[(size_t)tx * g.W + rx];  // taps of t that read r
          if (g.rs == 12)
            n += iy[(size_t)ry * g.H + ty] * ix[(size_t)rx * g.W + tx] + iy[(size_t)ty * g.H + ry] * ix[(size_t)tx * g.W + rx];
          best = std::max(best, n);
        }
  (void)K;
  return best;
}

int64_t nfp_workspace_bytes(const nfp_desc* d) {
  KP g;
  if (make_kp(d, &g)) return -1;
  if (!fast_geometry(g)) {
    // no tables; "same" maps the row-band kernels serve still get the arrival counters of their fused pooling tail
    return (g.stride == 1 && g.dil == 1 && g.pad == g.R && g.mode != NFP_PAD_CIRCULAR && (g.R == 1 || g.R == 2) && g.rs != 12)
               ? (int64_t)kTicketBytes : 0;
  }
  const WsLayout L = ws_layout(g.P, g.rs, g.mode);
  if (max_links(g) > L.LW) return 0;
  return (int64_t)kTicketBytes + (int64_t)L.bytes;
}

int nfp_workspace_init(const nfp_desc* d, void* ws, void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (nfp_workspace_bytes(d) <= 0) return fail(NFP_E_UNSUPPORTED, "this descriptor has no workspace tables");
  if (!ws || ((uintptr_t)ws & 15)) return fail(NFP_E_INVALID, "workspace pointer must be non-null and 16-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  if (!t_dry)   // the arrival counters of the pooled kernels: zero between launches (nfp_common.h::pool_last_band)
    if (int rc = hip_ok(hipMemsetAsync(ws, 0, kTicketBytes, st), "zero the workspace's counters")) return rc;
  if (!fast_geometry(g)) return NFP_OK;   // (no tables for this geometry)
  unsigned char* tables = (unsigned char*)ws + kTicketBytes;
  const int items = g.P * g.k * g.k, blocks = std::min(64, (items + 255) / 256);
  return with_radius<true>(g, [&](auto r) {
    return launch("#fill_workspace", fill_workspace<r()>, dim3(blocks), dim3(256), 0, st, g, tables);
  });
}

int nfp_forward(const nfp_desc* d, const void* x, void* out, float* saved, void* hip_stream) {
  return finish(forward_impl(d, x, out, saved, hip_stream), "nfp_forward");
}

int nfp_backward(const nfp_desc* d, const void* x, const void* grad_out, const void* out, const float* saved,
                 void* grad_x, void* hip_stream) {
  return finish(backward_impl(d, x, grad_out, out, saved, grad_x, hip_stream), "nfp_backward");
}

// What would nfp_forward / nfp_backward launch for this descriptor?  Nothing touches the GPU: the dispatcher runs
// in plan mode with 4 KiB-aligned stand-in pointers and the launches are described into `buf` as
//   "<variant> | <kernel> grid=(x,y,z) block=t lds=bytes[; <kernel> ...]".
int nfp_plan(const nfp_desc* d, int32_t backward, char* buf, int32_t buflen) {
  if (!buf || buflen < 1) return fail(NFP_E_INVALID, "null plan buffer");
  buf[0] = 0;
  const DryFlag dry;  // (thread-local, like the variant and plan buffers: concurrent calls do not see each other)
  t_plan[0] = 0;
  void* const fake = kStandIn;
  nfp_desc dd = *d;  // as the caller would run it: with the workspace the descriptor is entitled to
  if (dd.ws == nullptr && nfp_workspace_bytes(&dd) > 0) dd.ws = fake;
  d = &dd;
  const int rc = finish(backward ? backward_impl(d, fake, fake, fake, (const float*)fake, fake, nullptr)
                                 : forward_impl(d, fake, fake, (float*)fake, nullptr),
                        "nfp_plan");
  if (rc == NFP_OK) snprintf(buf, (size_t)buflen, "%s | %s", g_variant, t_plan);
  return rc;
}

// ---- fused nfp_pooling tail (models/NFP_Pooling.py:27-31) ----------------------------------------------
// Both launchers run in plan mode (nothing touches the GPU): the answer is exactly "nfp_pool_forward AND
// nfp_pool_backward would launch", whatever the LDS sizing rules of the kernels are this week.  (Round 2 re-derived
// the backward's table size here and forgot the forward's slab: 576 descriptors with R = 2 and P >= 256 were promised
// and then refused — ADVICE round 2.)
static int pool_plan(const KP& g, bool backward) {
  const DryRun dry;
  void* const fake = kStandIn;
  const float* cf = (const float*)fake;
  return backward ? pool_backward(g, fake, fake, cf, fake, nullptr, cf, cf)
                  : pool_forward(g, fake, fake, (float*)fake, nullptr, (float*)fake, (float*)fake);
}

static bool pool_measure_ok(const KP& g) {
  return g.rs != 12 && hot_measure(g) && !mixed_maps(g);   // (map_f32: nfp_forward / nfp_backward only)
}

int nfp_pool_supported(const nfp_desc* d) {
  KP g;
  if (make_kp(d, &g)) return 0;
  // cosine / L2 on "same" maps, either layout, float32 or bf16: the table kernels (<= 512 pixels, descriptor with its
  // workspace) or the row-band kernels (any size).  Pointer alignment is the caller's: channels-last maps need 16-byte
  // aligned images (as nfp_forward's hot path).
  if (!pool_measure_ok(g)) return 0;
  if (g.B == 0) return 1;
  return pool_plan(g, false) == NFP_OK && pool_plan(g, true) == NFP_OK ? 1 : 0;
}

int64_t nfp_pool_saved_floats(const nfp_desc* d) {
  KP g;
  if (make_kp(d, &g)) return -1;
  if (!pool_measure_ok(g) || g.B == 0) return 0;
  if (pool_plan(g, false) != NFP_OK) return 0;
  return (int64_t)stats_of(g.measure) * g.B * g.P + t_pool_scratch;
}

int nfp_pool_forward(const nfp_desc* d, const void* x, float* gap, float* nfpm, void* out_map, float* saved,
                     void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (!x || !nfpm) return fail(NFP_E_INVALID, "null tensor pointer");
  if (!pool_measure_ok(g)) return fail(NFP_E_UNSUPPORTED, "fused pooling tail: cosine / dot / gfc / L2 (norm p=2) / rmse, one radius");
  if (g.B == 0) return NFP_OK;
  g.pool_gap = gap != nullptr ? 1 : 0;       // NULL: GAP(x) is not wanted (texture_pooling.py:251-252)
  g.pool_map = out_map != nullptr ? 1 : 0;   // NULL: no backward will follow, nobody reads the maps
  hipStream_t st = (hipStream_t)hip_stream;
  return finish(pool_forward(g, x, out_map, saved, st, gap, nfpm), "nfp_pool_forward");
}

int nfp_pool_backward(const nfp_desc* d, const void* x, const float* grad_gap, const float* grad_nfpm,
                      const void* out_map, const float* saved, void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (!x || !grad_nfpm || !out_map || !grad_x) return fail(NFP_E_INVALID, "null tensor pointer");
  if (!pool_measure_ok(g)) return fail(NFP_E_UNSUPPORTED, "fused pooling tail: cosine / dot / gfc / L2 (norm p=2) / rmse, one radius");
  if (stats_of(g.measure) > 0 && !saved) return fail(NFP_E_INVALID, "missing saved state");
  if (g.B == 0) return NFP_OK;
  g.pool_gap = grad_gap != nullptr ? 1 : 0;  // NULL: GAP(x) took no part in the loss (or was never produced)
  hipStream_t st = (hipStream_t)hip_stream;
  return finish(pool_backward(g, x, out_map, saved, grad_x, st, grad_gap, grad_nfpm), "nfp_pool_backward");
}

// ---- GAP(x) beside the full maps: the first step of an NFP head (nfp_heads.py) -------------------------------------------
// As pool_plan: both launchers in plan mode, so that a 1 means nfp_gap_forward AND nfp_gap_backward will launch.
static int gap_plan(const KP& g, bool backward) {
  const DryRun dry;
  void* const fake = kStandIn;
  const float* cf = (const float*)fake;
  return backward ? gap_backward(g, fake, fake, fake, cf, fake, nullptr, cf)
                  : gap_forward(g, fake, fake, (float*)fake, nullptr, (float*)fake);
}

// The gap calls also take radii (1, 2) together (inner_R = 1: make_kp); Norm p = 1 / EMD are outside hot_measure.
static bool gap_measure_ok(const KP& g) { return hot_measure(g) && !mixed_maps(g); }   // (map_f32: nfp_forward / nfp_backward only)

int nfp_gap_supported(const nfp_desc* d) {
  KP g;
  if (make_kp(d, &g)) return 0;
  if (!gap_measure_ok(g)) return 0;
  if (g.B == 0) return 1;
  return gap_plan(g, false) == NFP_OK && gap_plan(g, true) == NFP_OK ? 1 : 0;
}

int64_t nfp_gap_saved_floats(const nfp_desc* d) {
  KP g;
  if (make_kp(d, &g)) return -1;
  if (!gap_measure_ok(g) || g.B == 0) return 0;
  if (gap_plan(g, false) != NFP_OK) return 0;
  return (int64_t)stats_of(g.measure) * g.B * g.P + t_pool_scratch;
}

int nfp_gap_forward(const nfp_desc* d, const void* x, float* gap, void* out_map, float* saved, int64_t saved_floats,
                    void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (!gap_measure_ok(g)) return fail(NFP_E_UNSUPPORTED, "GAP beside the maps: cosine / dot / gfc / L2 (norm p=2) / rmse");
  if (g.B == 0) return NFP_OK;
  if (!x || !gap || !out_map) return fail(NFP_E_INVALID, "null tensor pointer");
  const int64_t need = std::max<int64_t>(nfp_gap_saved_floats(d), 1);
  if (saved == nullptr || saved_floats < need)
    return fail(NFP_E_INVALID, "saved holds %lld floats, nfp_gap_saved_floats is %lld", (long long)(saved ? saved_floats : 0),
                (long long)need);
  hipStream_t st = (hipStream_t)hip_stream;
  return finish(gap_forward(g, x, out_map, saved, st, gap), "nfp_gap_forward");
}

int nfp_gap_backward(const nfp_desc* d, const void* x, const float* grad_gap, const void* grad_out, const void* out_map,
                     const float* saved, int64_t saved_floats, void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (!gap_measure_ok(g)) return fail(NFP_E_UNSUPPORTED, "GAP beside the maps: cosine / dot / gfc / L2 (norm p=2) / rmse");
  if (g.B == 0) return NFP_OK;
  if (!x || !grad_out || !out_map || !grad_x) return fail(NFP_E_INVALID, "null tensor pointer");
  const int64_t need = (int64_t)stats_of(g.measure) * g.B * g.P;   // (the backward reads the per-pixel state alone)
  if (need > 0 && (saved == nullptr || saved_floats < need))
    return fail(NFP_E_INVALID, "saved holds %lld floats, the backward reads %lld", (long long)(saved ? saved_floats : 0), (long long)need);
  hipStream_t st = (hipStream_t)hip_stream;
  return finish(gap_backward(g, x, grad_out, out_map, saved, grad_x, st, grad_gap), "nfp_gap_backward");
}

// ---- valid maps (padding 0): nfp_valid.hip ---------------------------------------------------------------------------------
// Both launchers in plan mode, so that a 1 means nfp_valid_forward AND nfp_valid_backward will launch (4 KiB-aligned
// buffers assumed, as nfp_plan does); nothing of the calling thread's variant / plan / error strings changes.
static int valid_plan(const KP& g, bool backward) {
  const DryRun dry;
  void* const fake = kStandIn;
  return backward ? valid_backward(g, fake, fake, fake, (const float*)fake, fake, nullptr)
                  : valid_forward(g, fake, fake, (float*)fake, nullptr);
}

int nfp_valid_supported(const nfp_desc* d) {
  KP g;
  const DryRun dry;   // (make_kp and valid_refusal's callers write the error string too)
  return make_kp(d, &g) == NFP_OK && valid_refusal(g) == nullptr &&
                 (g.B == 0 || (valid_plan(g, false) == NFP_OK && valid_plan(g, true) == NFP_OK))
             ? 1 : 0;
}

int64_t nfp_valid_saved_floats(const nfp_desc* d) {
  KP g;
  if (make_kp(d, &g)) return -1;
  if (valid_refusal(g) != nullptr) return 0;
  return (int64_t)stats_of(g.measure) * g.B * g.P;   // |x| per input pixel (cosine / gfc)
}

static int valid_kp(const nfp_desc* d, KP* g) {
  if (int rc = make_kp(d, g)) return rc;
  if (const char* why = valid_refusal(*g)) return fail(NFP_E_UNSUPPORTED, "valid maps: %s", why);
  return NFP_OK;
}

int nfp_valid_forward(const nfp_desc* d, const void* x, void* out, float* saved, int64_t saved_floats, void* hip_stream) {
  KP g;
  if (int rc = valid_kp(d, &g)) return rc;
  if (g.B > 0 && (!x || !out)) return fail(NFP_E_INVALID, "null tensor pointer");
  const int64_t need = nfp_valid_saved_floats(d);
  if (saved != nullptr && saved_floats < need)
    return fail(NFP_E_INVALID, "saved holds %lld floats, nfp_valid_saved_floats is %lld", (long long)saved_floats, (long long)need);
  if (g.B == 0) return NFP_OK;
  return finish(valid_forward(g, x, out, saved, (hipStream_t)hip_stream), "nfp_valid_forward");
}

int nfp_valid_backward(const nfp_desc* d, const void* x, const void* grad_out, const void* out, const float* saved,
                       int64_t saved_floats, void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = valid_kp(d, &g)) return rc;
  if (g.B > 0 && (!x || !grad_out || !out || !grad_x)) return fail(NFP_E_INVALID, "null tensor pointer");
  const int64_t need = nfp_valid_saved_floats(d);
  if (need > 0 && (saved == nullptr || saved_floats < need))
    return fail(NFP_E_INVALID, "saved holds %lld floats, nfp_valid_saved_floats is %lld", (long long)(saved ? saved_floats : 0),
                (long long)need);
  if (g.B == 0) return NFP_OK;
  return finish(valid_backward(g, x, grad_out, out, saved, grad_x, (hipStream_t)hip_stream), "nfp_valid_backward");
}

// ---- ABI 7: NFPPooling(bias=True) — nfp_bias.hip ---------------------------------------------------------------------
// The descriptor's own measure: make_kp serves EMD as Norm p = 1 on the difference weights, which a bias on the
// neighbour side breaks (|(a + bc) - (x_n + beta)| is not |(a - x_n) + beta|).  The difference weights are applied by the
// kernels (dw); the measures then see g.diff = 0.
static int bias_kp(const nfp_desc* d, KP* g, int* dw) {
  if (int rc = make_kp(d, g)) return rc;
  if (d->inner_R != 0) return fail(NFP_E_UNSUPPORTED, "biased NFP: one radius per call (inner_R = 0)");
  if (d->map_f32 != 0) return fail(NFP_E_UNSUPPORTED, "biased NFP: maps in the storage type (map_f32 = 0)");
  if (d->measure == NFP_SCS)
    return fail(NFP_E_UNSUPPORTED, "biased NFP: measure %d (SharpenedCosine mixes batch elements) has no HIP kernel", d->measure);
  g->measure = d->measure;
  g->p = d->p;
  g->diff = 0;
  *dw = d->diff_weights != 0 ? 1 : 0;
  return NFP_OK;
}
static bool bias_no_centre(const KP& g) { return g.measure == NFP_NORM || g.measure == NFP_RMSE; }

int64_t nfp_bias_saved_floats(const nfp_desc* d) {
  KP g;
  int dw;
  if (bias_kp(d, &g, &dw)) return -1;
  const int64_t bno = (int64_t)g.B * g.N * g.O;
  if (g.measure == NFP_ATTENTION) return bno;  // the raw dots (float32), also without a backward
  return 2LL * stats_of(g.measure) * bno;      // per-pair stats of the centre and the neighbour side
}

int64_t nfp_bias_scratch_floats(const nfp_desc* d) {
  KP g;
  int dw;
  if (bias_kp(d, &g, &dw)) return -1;
  const int64_t bno = (int64_t)g.B * g.N * g.O;
  const bool attn = g.measure == NFP_ATTENTION;
  return bno * bias_coef_floats(attn ? as_dot(g) : g) + (int64_t)g.B * g.C * (g.N + 1) + (attn ? bno : 0);
}

int nfp_bias_forward(const nfp_desc* d, const void* x, const float* centre_bias, const float* neighbour_bias, void* out,
                     float* saved, int64_t saved_floats, void* hip_stream) {
  KP g;
  int dw;
  if (int rc = bias_kp(d, &g, &dw)) return rc;
  // (an empty batch: x and out hold no element, and torch hands such tensors over as NULL)
  if ((g.B > 0 && (!x || !out)) || !neighbour_bias || (!centre_bias && !bias_no_centre(g)))
    return fail(NFP_E_INVALID, "null tensor pointer");
  const int64_t need = nfp_bias_saved_floats(d);
  if ((saved != nullptr || g.measure == NFP_ATTENTION) && need > 0 && (saved == nullptr || saved_floats < need))
    return fail(NFP_E_INVALID, "saved holds %lld floats, nfp_bias_saved_floats is %lld", (long long)saved_floats, (long long)need);
  if (g.B == 0) return NFP_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  if (g.measure == NFP_ATTENTION) {
    if (int rc = bias_forward(as_dot(g), dw, x, centre_bias, neighbour_bias, nullptr, nullptr, saved, st)) return rc;
    const long long n = (long long)g.B * g.O;
    variant_suffix("+attn_softmax");
    return finish(launch("attn_softmax_fwd", attn_softmax_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g,
                         (const float*)saved, out), "nfp_bias_forward");
  }
  return finish(bias_forward(g, dw, x, centre_bias, neighbour_bias, out, saved, nullptr, st), "nfp_bias_forward");
}

int nfp_bias_backward(const nfp_desc* d, const void* x, const float* centre_bias, const float* neighbour_bias,
                      const void* grad_out, const void* out, const float* saved, int64_t saved_floats, void* grad_x,
                      float* grad_centre_bias, float* grad_neighbour_bias, float* scratch, int64_t scratch_floats,
                      void* hip_stream) {
  KP g;
  int dw;
  if (int rc = bias_kp(d, &g, &dw)) return rc;
  const bool nc = bias_no_centre(g);
  if ((g.B > 0 && (!x || !grad_out || !out || !grad_x)) || !neighbour_bias || !grad_neighbour_bias ||
      (!nc && (!centre_bias || !grad_centre_bias)))
    return fail(NFP_E_INVALID, "null tensor pointer");
  const int64_t need = nfp_bias_saved_floats(d), need_s = nfp_bias_scratch_floats(d);
  if (need > 0 && (saved == nullptr || saved_floats < need))
    return fail(NFP_E_INVALID, "saved holds %lld floats, nfp_bias_saved_floats is %lld", (long long)saved_floats, (long long)need);
  if ((need_s > 0 && scratch == nullptr) || scratch_floats < need_s)
    return fail(NFP_E_INVALID, "scratch holds %lld floats, nfp_bias_scratch_floats is %lld", (long long)scratch_floats,
                (long long)need_s);
  hipStream_t st = (hipStream_t)hip_stream;
  if (g.measure == NFP_ATTENTION) {
    // gradient with respect to the dots behind the scratch's coefficient and partial-sum parts, then DotProduct's backward
    const long long bno = (long long)g.B * g.N * g.O, n = (long long)g.B * g.O;
    KP gdot = as_dot(g);
    gdot.godtype = NFP_F32;
    float* gd = scratch + bno * bias_coef_floats(gdot) + (long long)g.B * g.C * (g.N + 1);
    if (g.B > 0)
      if (int rc = launch("attn_softmax_bwd", attn_softmax_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, grad_out,
                          out, gd))
        return rc;
    const int rc = bias_backward(gdot, dw, x, centre_bias, neighbour_bias, gd, saved, nullptr, grad_x, grad_centre_bias,
                                 grad_neighbour_bias, scratch, st);
    if (rc == NFP_OK) variant_suffix("+attn_softmax");
    return finish(rc, "nfp_bias_backward");
  }
  return finish(bias_backward(g, dw, x, centre_bias, neighbour_bias, grad_out, out, saved, grad_x, nc ? nullptr : grad_centre_bias,
                              grad_neighbour_bias, scratch, st),
                "nfp_bias_backward");
}

}  // extern "C"
