// nfp_hip.hip — C ABI of libnfp_hip.so (include/nfp.h) and kernel dispatch.
//
// Stands in for models/pooling/nfp.py::NFPPooling.forward (nfp.py:132-134) and its
// autograd backward.  gfx950 only; no CPU path lives here — the library fails
// loudly (NFP_E_HIP / NFP_E_UNSUPPORTED) rather than fall back.  The kernels and their launchers live in the other units,
// behind the interfaces of nfp_launch.h; this one launches fill_workspace alone.
#include "nfp_launch.h"
#include "nfp_tables.h"

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
  if (!fast_geometry(*g)) g->ws = nullptr;   // (not a table geometry: its workspace holds the counters alone)
  // index arithmetic of the general kernels: coordinates in 15 bits, pair indices in 31
  if (d->H > 32767 || d->W > 32767 || (int64_t)g->P > (1 << 26) || (int64_t)g->N * g->O >= (1LL << 31) || d->B > 65535)
    return fail(NFP_E_UNSUPPORTED, "feature map [%d,%d,%d,%d] with k = %d exceeds the index range of the kernels", d->B,
                d->C, d->H, d->W, k);
  return NFP_OK;
}

}  // namespace

#ifdef NFP_STAMPS
// (every unit whose kernels stamp has its own copy of the device-side stamp pointer, and a setter for it; this unit's
// kernels — fill_workspace — do not stamp)
extern "C" int nfp_debug_set_stamp_buffer_generic(void* dev_ptr);
extern "C" int nfp_debug_set_stamp_buffer_table_fwd(void* dev_ptr);
extern "C" int nfp_debug_set_stamp_buffer_table_bwd(void* dev_ptr);
extern "C" int nfp_debug_set_stamp_buffer_tile_fwd(void* dev_ptr);
extern "C" int nfp_debug_set_stamp_buffer_tile_bwd(void* dev_ptr);
extern "C" int nfp_debug_set_stamp_buffer_tile_r3_fwd(void* dev_ptr);
extern "C" int nfp_debug_set_stamp_buffer_tile_r3_bwd(void* dev_ptr);
extern "C" int nfp_debug_set_stamp_buffer(void* dev_ptr) {
  for (auto set : {nfp_debug_set_stamp_buffer_generic, nfp_debug_set_stamp_buffer_table_fwd, nfp_debug_set_stamp_buffer_table_bwd,
                   nfp_debug_set_stamp_buffer_tile_fwd, nfp_debug_set_stamp_buffer_tile_bwd,
                   nfp_debug_set_stamp_buffer_tile_r3_fwd, nfp_debug_set_stamp_buffer_tile_r3_bwd})
    if (int rc = set(dev_ptr)) return rc;
  return NFP_OK;
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

// Checks the entry points share.  The ORDER in which an entry applies them is its own, and observable: where two checks
// fail at once the caller sees the first (tests/test_entry_refusals_host.py).
// One of `tensors` is null although required (the valid and biased entries: x / out only for B > 0)
bool missing(std::initializer_list<const void*> tensors, bool required = true) {
  for (const void* p : tensors)
    if (required && !p) {
      fail(NFP_E_INVALID, "null tensor pointer");
      return true;
    }
  return false;
}

// a caller buffer shorter than its size query says.  `query`: "<size function> is", or what reads it
int short_buffer(const char* what, int64_t have, const char* query, int64_t need) {
  return fail(NFP_E_INVALID, "%s holds %lld floats, %s %lld", what, (long long)have, query, (long long)need);
}

// The hot-path forward of a plain single-radius map, or kNotApplicable: table kernels (matrix cores first for bf16), then the
// row-band kernels.
int hot_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st) {
  if (g_sw.tile_first.load(std::memory_order_relaxed))
    if (int rc = tile_forward(g, x, out, saved, st); rc != kNotApplicable) return rc;
  // (Geman / Canberra / Hellinger / Jeffrey / squared chord / chi-squared 1 share the kSymTerm instantiation)
  if (fast_ok(g, x, x, true)) {
    // (the matrix-core forward has the cosine and L2 forms alone)
    if (int rc = table_fwd_gram(g, x, out, saved, st); rc != kNotApplicable) return rc;
    if (int rc = table_fwd_band(g, x, out, saved, st); rc != kNotApplicable) return rc;
  }
  // maps above the table kernels' 512 pixels, or a descriptor without its tables: the row-band kernels (nfp_tile_fwd.hip)
  if (int rc = tile_forward(g, x, out, saved, st); rc != kNotApplicable) return rc;
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

// Radii (1, 2) from one pass (g.rs == 12): the table kernels' two-radius form or a refusal — `table` is its launcher,
// `which` the direction its refusal names
template <typename F>
int multi_radius(const KP& g, const void* x, const void* gx, const char* which, F&& table) {
  if (g.ws == nullptr || !fast_ok(g, x, gx))
    return fail(NFP_E_UNSUPPORTED, "multi-radius: cosine / dot / gfc / L2 / rmse / norm p=1 / emd on maps of at most %d pixels, "
                "C %% 4 == 0, dense layout, descriptor with a workspace", kBwdThreads);
  const int rc = table();
  return rc == kNotApplicable ? fail(NFP_E_UNSUPPORTED, "multi-radius: the map does not fit the hot-path %s", which) : rc;
}

int forward_impl(const nfp_desc* d, const void* x, void* out, float* saved, void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (missing({x, out})) return NFP_E_INVALID;
  if (int rc = mixed_refused(d)) return rc;
  if (g.B == 0) return NFP_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  if (g.rs == 12) return multi_radius(g, x, x, "forward", [&] { return table_fwd_band(g, x, out, saved, st); });
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
    if (rc == kNotApplicable) rc = generic_forward(gd, x, dots, nullptr, st);
    if (rc) return rc;
    variant_suffix("+attn_softmax");
    return attn_softmax_forward(g, dots, out, st);
  }
  const int rc = generic_forward(g, x, out, saved, st);
  if (rc == kNotApplicable)
    return fail(NFP_E_UNSUPPORTED, "measure %d (SharpenedCosine mixes batch elements in the reference, "
                "nfp.py:359-374) has no HIP kernel", g.measure);
  return rc;
}

// The hot-path backward of a plain single-radius map, or kNotApplicable (as hot_forward).
int hot_backward(const KP& g, const void* x, const void* grad_out, const void* out, const float* saved, void* grad_x,
                 hipStream_t st) {
  if (g_sw.tile_first.load(std::memory_order_relaxed))
    if (int rc = tile_backward(g, x, grad_out, out, saved, grad_x, st); rc != kNotApplicable) return rc;
  // k = 5, float32 NCHW, maps of 14 x 14 and more: the row-band backward (window weights in registers, no 13-entry-per-pixel
  // gather phase) beats the table kernel — [256,192,14,14] L2 40.9 -> 35.7 us, cosine 41.1 -> 37.1, [256,256,14,14] 50.5 ->
  // 44.1 (profiles/r04_n_…; the FORWARD stays on the tables: 19 vs 28 us; channels-last and bf16 stay too).  Same saved
  // state (the map and |x| per pixel), so the two mix.
  if (g.R == 2 && g.rs != 12 && g.dtype == NFP_F32 && g.contig && g.P >= 196 && hot_measure(g))
    if (int rc = tile_backward(g, x, grad_out, out, saved, grad_x, st); rc != kNotApplicable) return rc;
  // The table kernels.  The kSymTerm measures only below 14 x 14: from there up the row-band backward is ahead ([256,192,14,14]
  // k = 5 97.5 vs 101.9 us, [256,64,20,20] 37.5 vs 41.4; at 7 x 7 the table kernel: [64,512,7,7] 10.1-12.3 vs 18.2-22.5 us —
  // profiles/r04_zd_…; the forward stays on the tables up to 512 pixels: 52.7 vs 66.8 us at [256,192,14,14])
  if (g.ws != nullptr && fast_ok(g, x, grad_x, true) && !(hot_sym(g) && !(NFP_SYM_TABLE_BWD && g.P < 196))) {
    if (int rc = table_backward(g, x, grad_out, out, saved, grad_x, st); rc != kNotApplicable) return rc;
  }
  if (int rc = tile_backward(g, x, grad_out, out, saved, grad_x, st); rc != kNotApplicable) return rc;
  return kNotApplicable;
}

int backward_impl(const nfp_desc* d, const void* x, const void* grad_out, const void* out, const float* saved,
                  void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (missing({x, grad_out, out, grad_x})) return NFP_E_INVALID;
  if ((stats_of(g.measure) > 0 || g.measure == NFP_ATTENTION) && !saved) return fail(NFP_E_INVALID, "measure %d needs the saved state of nfp_forward", g.measure);
  if (int rc = mixed_refused(d)) return rc;
  if (g.B == 0) return NFP_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  if (g.rs == 12)
    return multi_radius(g, x, grad_x, "backward", [&] { return table_backward(g, x, grad_out, out, saved, grad_x, st); });
  if (int rc = hot_backward(g, x, grad_out, out, saved, grad_x, st); rc != kNotApplicable) return rc;
  if (g.measure == NFP_ATTENTION) {
    float* gd = const_cast<float*>(saved);  // scratch handed over by nfp_forward's caller (nfp_saved_floats)
    if (int rc = attn_softmax_backward(g, grad_out, out, gd, st)) return rc;
    KP gdot = as_dot(g);
    gdot.odtype = g.odtype;
    gdot.godtype = NFP_F32;
    // float32 maps: DotProduct's hot-path backward on the gradient with respect to the dots (it keeps no saved state: `out` is
    // only read in bounds)
    if (g.dtype == NFP_F32) {
      if (int rc = hot_backward(gdot, x, gd, out, nullptr, grad_x, st); rc != kNotApplicable) return rc;
    }
    return generic_backward(gdot, x, gd, out, nullptr, grad_x, st);
  }
  const int rc = generic_backward(g, x, grad_out, out, saved, grad_x, st);
  if (rc == kNotApplicable) return fail(NFP_E_UNSUPPORTED, "measure %d (SharpenedCosine) has no HIP kernel", g.measure);
  return rc;
}

// ---- the fused tails: nfp_pool_* (kPoolBoth: both pooled sums) and nfp_gap_* (kPoolGap: GAP(x) beside the full maps, the
// pass of an NFP head — nfp_heads.py: gap(fmap) and nfp(fmap) of one feature map) ----
// Forward: the table kernels (matrix cores first, as in nfp_forward: fwd_gram's sums are a run-time option and it declines
// float32 storage itself), else the row bands.  One band per image writes its sums itself; several write rows of partial
// sums to the scratch behind the per-pixel state in `saved` (nfp_tile.h::fwd_tile<POOL>), joined in band order by pool_fold —
// or, in pool mode with the arrival counters, by the last band to arrive inside the same launch
// (nfp_common.h::pool_last_band).  *scratch (if asked for): the floats of those rows; it is written on that route alone.
// Radius 12 (radii 1 and 2 from one pass, MultiRadiusNFPHead; gap mode only: nfp_pool_* refuses it) has neither a
// matrix-core nor a row-band form: table_fwd_gram declines it itself and tile_ok refuses it through tile_geometry, so the
// vector table kernels serve bf16 too and maps above 512 pixels are not served.
int fused_forward(KP g, int mode, const void* x, void* out_map, float* saved, hipStream_t st, float* gap, float* nfpm,
                  long long* scratch = nullptr) {
  // what differs between the two tails:
  const bool gp = mode == kPoolGap;
  if (gp) g.tickets = nullptr;              // gap: never the arrival counters (no atomics on this path)
  if (gp) g.pool_gap = g.pool_map = 1;      //      both outputs always (pool: the entry's, NULL = not wanted)
  const int width = gp ? g.C : g.C + g.N;   // floats of a scratch row: the channel sums, and pool's map sums behind them
  KP gfold = g;
  if (gp) gfold.N = 0;                      // (pool_fold then joins the channel sums alone)
  // gap needs `saved` up front; pool only on the row-band route — without it the table route keeps one band (part = null)
  if (gp && saved == nullptr) return fail(NFP_E_INVALID, "GAP beside the maps needs the scratch of nfp_gap_saved_floats");

  float* part = saved != nullptr ? saved + (long long)stats_of(g.measure) * g.B * g.P : nullptr;
  int nb = 1;
  const FwdTail t{mode, gap, nfpm, part, &nb};
  int rc = kNotApplicable;
  if (g.ws != nullptr && fast_ok(g, x, x)) {
    if (int rcg = table_fwd_gram(g, x, out_map, saved, st, t); rcg != kNotApplicable) return rcg;
    rc = table_fwd_band(g, x, out_map, saved, st, t);
    if (rc != kNotApplicable && !(rc == NFP_OK && nb > 1)) return rc;
  }
  if (rc == kNotApplicable) {   // row bands (any map size): always partial sums, joined below
    if (!tile_ok(g, x, x)) return kNotApplicable;
    if (saved == nullptr) return fail(NFP_E_INVALID, "fused pooling tail on this map needs the scratch of nfp_pool_saved_floats");
    if (rc = tile_forward(g, x, out_map, saved, st, t); rc != NFP_OK) return rc;
  }
  if (scratch) *scratch = (long long)g.B * nb * width;
  if (g.tickets != nullptr) return NFP_OK;   // (the last band to arrive folded them inside the launch)
  variant_suffix("+pool_fold");
  return tile_pool_fold(gfold, part, gap, nfpm, nb, st);
}

// Backward: the table kernels, else the row bands (tile_backward refuses radius 12 itself: tile_ok).  pool: no grad_out
// (go = null), both pooled gradients; gap: grad_out read as a map, ggap[b,c] / P added in the same store.
int fused_backward(KP g, int mode, const void* x, const void* go, const void* out_map, const float* saved, void* gx,
                   hipStream_t st, const float* ggap, const float* gnfpm) {
  g.pool_gap = ggap != nullptr ? 1 : 0;   // NULL: GAP(x) took no part in the loss — nothing is added, nothing is read
  const BwdTail t{mode, ggap, gnfpm};
  if (g.ws != nullptr && fast_ok(g, x, gx))
    if (int rc = table_backward(g, x, go, out_map, saved, gx, st, t); rc != kNotApplicable) return rc;
  return tile_backward(g, x, go, out_map, saved, gx, st, t);
}

// "Would both launchers launch?" — both run in plan mode, on kStandIn pointers (4 KiB-aligned, as nfp_plan's; nothing
// touches the GPU), so the answer is exactly what the two entries would do, whatever the LDS sizing rules of the kernels
// are this week (round 2 re-derived the backward's table size for the pooled tail and forgot the forward's slab: 576
// descriptors with R = 2 and P >= 256 were promised and then refused — ADVICE round 2); nothing of the calling thread's
// variant / plan / error strings changes.
template <typename F, typename G>
bool both_launch(F&& forward, G&& backward) {
  const DryRun dry;
  return forward() == NFP_OK && backward() == NFP_OK;
}

// The measures of the two fused tails.  The gap calls also take radii (1, 2) together (inner_R = 1: make_kp); Norm p = 1 /
// EMD are outside hot_measure; map_f32 is nfp_forward's / nfp_backward's only.
bool tail_measure_ok(const KP& g, int mode) { return (mode == kPoolGap || g.rs != 12) && hot_measure(g) && !mixed_maps(g); }
int tail_refused(const KP& g, int mode) {
  if (tail_measure_ok(g, mode)) return NFP_OK;
  return fail(NFP_E_UNSUPPORTED, mode == kPoolGap ? "GAP beside the maps: cosine / dot / gfc / L2 (norm p=2) / rmse"
                                                  : "fused pooling tail: cosine / dot / gfc / L2 (norm p=2) / rmse, one radius");
}
// the forward of a tail as its dry runs make it (gap: no map sums)
int tail_try_forward(const KP& g, int mode, long long* scratch = nullptr) {
  void* const p = kStandIn;
  return fused_forward(g, mode, p, p, (float*)p, nullptr, (float*)p, mode == kPoolGap ? nullptr : (float*)p, scratch);
}

// nfp_pool_supported / nfp_gap_supported: cosine / L2 (and their riders) on "same" maps, either layout, float32 or bf16 — the
// table kernels (<= 512 pixels, descriptor with its workspace) or the row-band kernels (any size).  Pointer alignment is the
// caller's: channels-last maps need 16-byte aligned images (as nfp_forward's hot path).
int tail_supported(const nfp_desc* d, int mode) {
  KP g;
  if (make_kp(d, &g) || !tail_measure_ok(g, mode)) return 0;
  if (g.B == 0) return 1;
  const bool gp = mode == kPoolGap;
  return both_launch([&] { return tail_try_forward(g, mode); }, [&] {
    void* const p = kStandIn;
    const float* f = (const float*)p;
    return fused_backward(g, mode, p, gp ? p : nullptr, p, f, p, nullptr, f, gp ? nullptr : f);
  }) ? 1 : 0;
}
// ... and their saved_floats: the per-pixel state, and behind it the scratch rows the forward would write
int64_t tail_saved_floats(const nfp_desc* d, int mode) {
  KP g;
  if (make_kp(d, &g)) return -1;
  if (!tail_measure_ok(g, mode) || g.B == 0) return 0;
  long long scratch = 0;
  {
    const DryRun dry;
    if (tail_try_forward(g, mode, &scratch) != NFP_OK) return 0;
  }
  return (int64_t)stats_of(g.measure) * g.B * g.P + scratch;
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
  const int R = g.R;
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
  return best;
}

int64_t nfp_workspace_bytes(const nfp_desc* d) {
  KP g;
  if (make_kp(d, &g)) return -1;
  // no tables; "same" maps the row-band kernels serve still get the arrival counters of their fused pooling tail
  if (!fast_geometry(g)) return same_geometry(g) && g.rs != 12 ? (int64_t)kTicketBytes : 0;
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
int nfp_pool_supported(const nfp_desc* d) { return tail_supported(d, kPoolBoth); }
int64_t nfp_pool_saved_floats(const nfp_desc* d) { return tail_saved_floats(d, kPoolBoth); }

int nfp_pool_forward(const nfp_desc* d, const void* x, float* gap, float* nfpm, void* out_map, float* saved,
                     void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (missing({x, nfpm})) return NFP_E_INVALID;
  if (int rc = tail_refused(g, kPoolBoth)) return rc;
  if (g.B == 0) return NFP_OK;
  g.pool_gap = gap != nullptr ? 1 : 0;       // NULL: GAP(x) is not wanted (texture_pooling.py:251-252)
  g.pool_map = out_map != nullptr ? 1 : 0;   // NULL: no backward will follow, nobody reads the maps
  return finish(fused_forward(g, kPoolBoth, x, out_map, saved, (hipStream_t)hip_stream, gap, nfpm), "nfp_pool_forward");
}

// (grad_gap NULL: GAP(x) took no part in the loss, or was never produced)
int nfp_pool_backward(const nfp_desc* d, const void* x, const float* grad_gap, const float* grad_nfpm,
                      const void* out_map, const float* saved, void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (missing({x, grad_nfpm, out_map, grad_x})) return NFP_E_INVALID;
  if (int rc = tail_refused(g, kPoolBoth)) return rc;
  if (stats_of(g.measure) > 0 && !saved) return fail(NFP_E_INVALID, "missing saved state");
  if (g.B == 0) return NFP_OK;
  return finish(fused_backward(g, kPoolBoth, x, nullptr, out_map, saved, grad_x, (hipStream_t)hip_stream, grad_gap, grad_nfpm),
                "nfp_pool_backward");
}

// ---- GAP(x) beside the full maps: the first step of an NFP head (nfp_heads.py) -------------------------------------------
int nfp_gap_supported(const nfp_desc* d) { return tail_supported(d, kPoolGap); }
int64_t nfp_gap_saved_floats(const nfp_desc* d) { return tail_saved_floats(d, kPoolGap); }

int nfp_gap_forward(const nfp_desc* d, const void* x, float* gap, void* out_map, float* saved, int64_t saved_floats,
                    void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (int rc = tail_refused(g, kPoolGap)) return rc;
  if (g.B == 0) return NFP_OK;
  if (missing({x, gap, out_map})) return NFP_E_INVALID;
  const int64_t need = std::max<int64_t>(nfp_gap_saved_floats(d), 1);
  if (saved == nullptr || saved_floats < need) return short_buffer("saved", saved ? saved_floats : 0, "nfp_gap_saved_floats is", need);
  return finish(fused_forward(g, kPoolGap, x, out_map, saved, (hipStream_t)hip_stream, gap, nullptr), "nfp_gap_forward");
}

int nfp_gap_backward(const nfp_desc* d, const void* x, const float* grad_gap, const void* grad_out, const void* out_map,
                     const float* saved, int64_t saved_floats, void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = make_kp(d, &g)) return rc;
  if (int rc = tail_refused(g, kPoolGap)) return rc;
  if (g.B == 0) return NFP_OK;
  if (missing({x, grad_out, out_map, grad_x})) return NFP_E_INVALID;
  const int64_t need = (int64_t)stats_of(g.measure) * g.B * g.P;   // (the backward reads the per-pixel state alone)
  if (need > 0 && (saved == nullptr || saved_floats < need))
    return short_buffer("saved", saved ? saved_floats : 0, "the backward reads", need);
  return finish(fused_backward(g, kPoolGap, x, grad_out, out_map, saved, grad_x, (hipStream_t)hip_stream, grad_gap, nullptr),
                "nfp_gap_backward");
}

// ---- valid maps (padding 0): nfp_valid.hip ---------------------------------------------------------------------------------
int nfp_valid_supported(const nfp_desc* d) {
  KP g;
  const DryRun dry;   // (make_kp writes the error string too)
  void* const p = kStandIn;
  if (make_kp(d, &g) != NFP_OK || valid_refusal(g) != nullptr) return 0;
  return g.B == 0 || both_launch([&] { return valid_forward(g, p, p, (float*)p, nullptr); },
                                 [&] { return valid_backward(g, p, p, p, (const float*)p, p, nullptr); });
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
  if (missing({x, out}, g.B > 0)) return NFP_E_INVALID;
  const int64_t need = nfp_valid_saved_floats(d);
  if (saved != nullptr && saved_floats < need) return short_buffer("saved", saved_floats, "nfp_valid_saved_floats is", need);
  if (g.B == 0) return NFP_OK;
  return finish(valid_forward(g, x, out, saved, (hipStream_t)hip_stream), "nfp_valid_forward");
}

int nfp_valid_backward(const nfp_desc* d, const void* x, const void* grad_out, const void* out, const float* saved,
                       int64_t saved_floats, void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = valid_kp(d, &g)) return rc;
  if (missing({x, grad_out, out, grad_x}, g.B > 0)) return NFP_E_INVALID;
  const int64_t need = nfp_valid_saved_floats(d);
  if (need > 0 && (saved == nullptr || saved_floats < need))
    return short_buffer("saved", saved ? saved_floats : 0, "nfp_valid_saved_floats is", need);
  if (g.B == 0) return NFP_OK;
  return finish(valid_backward(g, x, grad_out, out, saved, grad_x, (hipStream_t)hip_stream), "nfp_valid_backward");
}

// ... and their L1 family: Norm p = 1 on the difference weights and EMD (make_kp: the same descriptor), x alone on the way back
int nfp_valid_abs_supported(const nfp_desc* d) {
  KP g;
  const DryRun dry;
  void* const p = kStandIn;
  if (make_kp(d, &g) != NFP_OK || valid_abs_refusal(g) != nullptr) return 0;
  return g.B == 0 || both_launch([&] { return valid_abs_forward(g, p, p, nullptr); },
                                 [&] { return valid_abs_backward(g, p, p, p, nullptr); });
}

static int valid_abs_kp(const nfp_desc* d, KP* g) {
  if (int rc = make_kp(d, g)) return rc;
  if (const char* why = valid_abs_refusal(*g)) return fail(NFP_E_UNSUPPORTED, "valid L1 maps: %s", why);
  return NFP_OK;
}

int nfp_valid_abs_forward(const nfp_desc* d, const void* x, void* out, void* hip_stream) {
  KP g;
  if (int rc = valid_abs_kp(d, &g)) return rc;
  if (missing({x, out}, g.B > 0)) return NFP_E_INVALID;
  if (g.B == 0) return NFP_OK;
  return finish(valid_abs_forward(g, x, out, (hipStream_t)hip_stream), "nfp_valid_abs_forward");
}

int nfp_valid_abs_backward(const nfp_desc* d, const void* x, const void* grad_out, void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = valid_abs_kp(d, &g)) return rc;
  if (missing({x, grad_out, grad_x}, g.B > 0)) return NFP_E_INVALID;
  if (g.B == 0) return NFP_OK;
  return finish(valid_abs_backward(g, x, grad_out, grad_x, (hipStream_t)hip_stream), "nfp_valid_abs_backward");
}

// ---- strided maps (stride 2 to 4): nfp_strided.hip — the valid-map quartet's signatures and length convention -------------
int nfp_strided_supported(const nfp_desc* d) {
  KP g;
  const DryRun dry;
  void* const p = kStandIn;
  if (make_kp(d, &g) != NFP_OK || strided_refusal(g) != nullptr) return 0;
  return g.B == 0 || both_launch([&] { return strided_forward(g, p, p, (float*)p, nullptr); },
                                 [&] { return strided_backward(g, p, p, p, (const float*)p, p, nullptr); });
}

int64_t nfp_strided_saved_floats(const nfp_desc* d) {
  KP g;
  if (make_kp(d, &g)) return -1;
  if (strided_refusal(g) != nullptr) return 0;
  return (int64_t)stats_of(g.measure) * g.B * g.P;   // |x| per input pixel (cosine / gfc)
}

static int strided_kp(const nfp_desc* d, KP* g) {
  if (int rc = make_kp(d, g)) return rc;
  if (const char* why = strided_refusal(*g)) return fail(NFP_E_UNSUPPORTED, "strided maps: %s", why);
  return NFP_OK;
}

int nfp_strided_forward(const nfp_desc* d, const void* x, void* out, float* saved, int64_t saved_floats, void* hip_stream) {
  KP g;
  if (int rc = strided_kp(d, &g)) return rc;
  if (missing({x, out}, g.B > 0)) return NFP_E_INVALID;
  const int64_t need = nfp_strided_saved_floats(d);
  if (saved != nullptr && saved_floats < need) return short_buffer("saved", saved_floats, "nfp_strided_saved_floats is", need);
  if (g.B == 0) return NFP_OK;
  return finish(strided_forward(g, x, out, saved, (hipStream_t)hip_stream), "nfp_strided_forward");
}

int nfp_strided_backward(const nfp_desc* d, const void* x, const void* grad_out, const void* out, const float* saved,
                         int64_t saved_floats, void* grad_x, void* hip_stream) {
  KP g;
  if (int rc = strided_kp(d, &g)) return rc;
  if (missing({x, grad_out, out, grad_x}, g.B > 0)) return NFP_E_INVALID;
  const int64_t need = nfp_strided_saved_floats(d);
  if (need > 0 && (saved == nullptr || saved_floats < need))
    return short_buffer("saved", saved ? saved_floats : 0, "nfp_strided_saved_floats is", need);
  if (g.B == 0) return NFP_OK;
  return finish(strided_backward(g, x, grad_out, out, saved, grad_x, (hipStream_t)hip_stream), "nfp_strided_backward");
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
  if (missing({x, out}, g.B > 0) || missing({neighbour_bias}) || missing({centre_bias}, !bias_no_centre(g))) return NFP_E_INVALID;
  const int64_t need = nfp_bias_saved_floats(d);
  if ((saved != nullptr || g.measure == NFP_ATTENTION) && need > 0 && (saved == nullptr || saved_floats < need))
    return short_buffer("saved", saved_floats, "nfp_bias_saved_floats is", need);
  if (g.B == 0) return NFP_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  if (g.measure == NFP_ATTENTION) {
    if (int rc = bias_forward(as_dot(g), dw, x, centre_bias, neighbour_bias, nullptr, nullptr, saved, st)) return rc;
    variant_suffix("+attn_softmax");
    return finish(attn_softmax_forward(g, saved, out, st), "nfp_bias_forward");
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
  if (missing({x, grad_out, out, grad_x}, g.B > 0) || missing({neighbour_bias, grad_neighbour_bias}) ||
      missing({centre_bias, grad_centre_bias}, !nc))
    return NFP_E_INVALID;
  const int64_t need = nfp_bias_saved_floats(d), need_s = nfp_bias_scratch_floats(d);
  if (need > 0 && (saved == nullptr || saved_floats < need)) return short_buffer("saved", saved_floats, "nfp_bias_saved_floats is", need);
  if ((need_s > 0 && scratch == nullptr) || scratch_floats < need_s)
    return short_buffer("scratch", scratch_floats, "nfp_bias_scratch_floats is", need_s);
  hipStream_t st = (hipStream_t)hip_stream;
  if (g.measure == NFP_ATTENTION) {
    // gradient with respect to the dots behind the scratch's coefficient and partial-sum parts, then DotProduct's backward
    const long long bno = (long long)g.B * g.N * g.O;
    KP gdot = as_dot(g);
    gdot.godtype = NFP_F32;
    float* gd = scratch + bno * bias_coef_floats(gdot) + (long long)g.B * g.C * (g.N + 1);
    if (g.B > 0)
      if (int rc = attn_softmax_backward(g, grad_out, out, gd, st)) return rc;
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
