// nfp_cpool.hip — the tail every head of models/nfp_heads.py shares behind its NFP maps (NFPHead nfp_heads.py:28-32,42-43,
// MultiRadiusNFPHead 98-102,114-115, AdaptiveFusionNFP 301-305,323-324):
//   compress = Conv2d(N, D, 1, bias=False) -> BatchNorm2d(D) -> ReLU        nfp_vec = GAP(compress(maps))    [B,N,P] -> [B,D]
// which the reference runs as four ATen ops over a [B,D,P] activation (and twice that backward).  Here [B,D,P] never
// exists.  Train-mode BatchNorm statistics of a 1x1 conv's output follow from the moments of its N-channel input,
//   mean_d = w_d . mu        var_d = w_d^T Sigma w_d        (mu [N], Sigma [N,N]: mean and biased covariance over M = B*P)
// so with c = m - mu, inv_d = 1/sqrt(var_d + eps), s_d = gamma_d inv_d:
//   a_bdp = s_d (w_d . c_bp) + beta_d          out_bd = (1/P) sum_p relu(a_bdp)
// (eval: mu = 0, inv_d from the running variance, the shift beta_d - s_d running_mean_d).  Backward, the pre-activation
// recomputed, ga_bdp = (G_bd / P) [a_bdp > 0]:
//   T_dn = sum_bp ga c_n      grad_beta_d = sum_bp ga      grad_gamma_d = inv_d sum_n w_dn T_dn   (eval: - inv_d rm_d grad_beta_d)
//   grad_w_dn = s_d (T_dn - grad_gamma_d inv_d (Sigma w_d)_n)                                     (eval: s_d T_dn)
//   k_n = sum_d w_dn s_d grad_beta_d / M      Q = sum_d s_d (grad_gamma_d inv_d / M) w_d w_d^T    (eval: both 0)
//   grad_m_bnp = sum_d w_dn s_d ga_bdp - k_n - (Q c_bp)_n
//
// Kernels (no atomics; every sum in a fixed order: two runs agree bitwise, and in eval image b's row does not depend on B):
//   cpool_moments   one workgroup per chunk of an image's pixels: the chunk's maps in LDS, its mean as a float32 anchor a_n
//                   plus the mean r_n of what is left after subtracting it, and the Gram of the maps about the anchor
//   cpool_finish    float64: mu = sum_k n_k (a_k + r_k) / M, Sigma = sum_k [Gram_k + n_k (r d' + d r' + d d')] / M with
//                   d = a_k - mu (the scatter about mu from the scatter about each anchor — within plus between, exact),
//                   slices of consecutive chunks joined in order; then w^T Sigma w, inv_d and the running statistics.  mu is
//                   kept as two floats
//   cpool_fwd       one workgroup per (image, 128 channels of D): lanes along d, two channels per lane with their scaled
//                   weight rows in registers; the image's centred maps in LDS, walked in chunks, read as broadcast
//                   ds_read_b128 along p (four pixels of one map per read, eight FMAs); the eight wavefronts split the pixels
//   cpool_bwd_part  the same walk over a slice of the batch: T and grad_beta of the slice for the workgroup's channels
//   cpool_bwd_reduce  one workgroup per 32 channels: the slices in order, the parameter gradients, this tile's share of k, Q
//   cp_bwd_maps     lanes along 64 pixels (their c_n in registers); D in blocks of 128 channels whose scaled rows are staged in
//                   LDS and dealt to the wavefronts, joined in wave order through LDS; then - k - Q c.  One template over
//                   where a channel's factor comes from (CpGrad): here G_bd / P from the block's table — launched as
//                   "cpool_bwd_maps"
//
// The same projection with the map kept — nfp_cproj_* (NFPInsert's nfp_proj, models/mobilenetv3.py:346-350; NFPBottleneck's
// bn2(conv2(.)), nfp_heads.py:270-272): out_bdp = [relu](a_bdp) stored as [B,D,P] in the maps' dtype, and a backward given
// grad_out [B,D,P], so ga_bdp = grad_out_bdp [a_bdp > 0] (without the ReLU: grad_out_bdp); every other formula above holds.
// cpool_moments / cpool_finish / cpool_bwd_reduce serve both; the backward reads grad_out twice, the maps and nothing else
// of that size — never the forward's output.
//   cproj_fwd       one workgroup per (chunk of an image's pixels, 64 channels of D): the chunk's centred maps and the
//                   channels' scaled rows in LDS; lanes along the flattened (d, p) range of the chunk, so adjacent lanes
//                   store adjacent pixels of a channel (or run on into the next channel where the chunk is the whole image)
//   cproj_bwd_part  cpool_bwd_part's lanes along d, over a slice of the batch's 64-pixel passes: the pass's maps and the
//                   [128 channels][64 pixels] tile of grad_out go to LDS with lanes along p (whole lines), and are read back
//                   as a float4 per channel; the sums into T, the join and part_w are cpool_bwd_part's (cp_part_sum,
//                   cp_part_join)
//   cp_bwd_maps     with grad_out read per (channel, pixel), lanes along p, four channels' loads in flight — launched as
//                   "cproj_bwd_maps"
// Channels-last out / grad_out, [b][p][d] (nfp_cproj_*_fmt, NFP_ACT_NHWC; the maps stay [B,N,P], the statistics kernels are
// the same launches): cproj_fwd's NHWC instantiations — the same kernel, lanes along the chunk's [p][d] range, launched as
// "cproj_fwd_nhwc" — and those of cproj_bwd_part / cp_bwd_maps ("cproj_bwd_part_nhwc", "cproj_bwd_maps_nhwc"), which bring
// their grad_out tile into LDS with d fastest: the same sums in the same order.
//
// Statistics over the batches of several ranks (nn.SyncBatchNorm) — nfp_cpsync_*: the same step in four stages around two
// gathers the caller makes.  The main forward, *_bwd_part and *_bwd_maps kernels above serve unchanged; what is added:
//   cps_record      cpool_finish's join of the rank's chunks, kept as a float64 record [count, mean, scatter about it]
//   cps_finish      cpool_finish on the records of all ranks, joined in rank order (within plus between, exact); leaves the
//                   global count and Sigma's second float behind inv for the backward
//   cpool_bwd_reduce<., SYNC>  divides by that count, and forms Sigma w from both floats
//   cps_kq_row      the workgroups' shares of k, Q summed into the rank's row; *_bwd_maps then read the ranks' rows
//   cps_zero        a rank without an image: a zero row, zero parameter gradients
//
// The kernels are in nfp_cp_kernels.h; this file is the host path of all twelve launching entries.  An entry states its call
// as a CpCall; behind the checks the call becomes a CpK (cp_fwd_k / cp_bwd_k) that a few steps fill further and launch from:
//   forward   cp_local_stats | cps_rank_record | cps_joined_stats, then cp_main_forward
//   backward  cp_sums, cps_rank_row, cp_grad_maps
// cp_forward / cp_backward (one rank) and cps_moments / cps_forward / cps_reduce / cps_maps (several) are compositions of
// those.  Which chunk, stride, passes and slices a kind launches with is decided in cp_chunks and cp_slices alone, and the
// layout of the scratch in cp_records / cp_parts alone, for the steps and the nfp_*_scratch_floats queries alike.
#include "nfp_cp_kernels.h"

namespace nfp_host {
namespace {

// What an extern "C" entry asks for.  kind: the pooled tail (nfp_cpool_*: out [B,D] float32, always with the ReLU) or the
// projection with the map kept (nfp_cproj_*: out / grad_out [B,D,P] in the maps' dtype, `relu` and `layout` the caller's).
// A forward fills rm_w .. saved_w, a backward rm .. gb; the other direction's fields stay zero.
// kCpWide: the pooled tail through the wide kernels (nfp_cpool_wide_*: up to 96 maps).
enum CpKind { kCpPool, kCpProj, kCpWide };
struct CpCall {
  const char* what;   // the entry's name, at the head of every message
  CpKind kind;
  int32_t layout, relu;
  int32_t B, N;
  int64_t P;
  int32_t D, dtype, training;
  const void* maps;
  const float *w, *gamma, *beta;
  double eps;
  int64_t saved_floats;
  float* scratch;
  int64_t scratch_floats;
  void* stream;
  float *rm_w, *rv_w;   // forward
  double momentum;
  void* out;
  float* saved_w;
  const float *rm, *rv, *saved;   // backward
  const void* go;
  void* gm;
  float *gw, *gg, *gb;
  int32_t sync;   // nfp_cpsync_*: the statistics are those of all ranks, so this rank's B * P may be 0 or 1
};
// An entry's leading arguments as a CpCall — NCHW with the ReLU, which the projection's entries overwrite; everything
// behind them zero, for the entry to fill by name
CpCall cp_call(const char* what, CpKind kind, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training,
               const void* maps, const float* w, const float* gamma, const float* beta) {
  CpCall c{};
  c.what = what, c.kind = kind, c.layout = NFP_ACT_NCHW, c.relu = 1;
  c.B = B, c.N = N, c.P = P, c.D = D, c.dtype = dtype, c.training = training;
  c.maps = maps, c.w = w, c.gamma = gamma, c.beta = beta;
  return c;
}
// ... and the buffers every entry but nfp_cpsync_moments names behind them
void cp_buffers(CpCall& c, double eps, int64_t saved_floats, float* scratch, int64_t scratch_floats, void* stream) {
  c.eps = eps, c.saved_floats = saved_floats, c.scratch = scratch, c.scratch_floats = scratch_floats, c.stream = stream;
}
hipStream_t cp_stream(const CpCall& c) { return (hipStream_t)c.stream; }

// ---- the sizes of each kind's kernels ----
int cpool_np(int N) { return (N + 7) & ~7; }
// pixels per chunk: the whole image where it fits the budget, else a multiple of 64
int cpool_chunk(int NP, long long P) {
  long long ch = std::min<long long>(P, nfp::kCpBudget / NP);
  if (ch < P) ch &= ~63LL;
  return (int)ch;
}
// floats between two rows of the chunk in LDS: a multiple of 4 (16-byte reads) and an odd number of 16-byte slots, so
// that sixteen rows at one quad (cpool_moments' Gram) fall on sixteen different slots
int cpool_stride(int ch) {
  int s = (ch + 3) & ~3;
  if (((s >> 2) & 1) == 0) s += 4;
  return s;
}
int cpool_tiles(int D) { return (D + nfp::kCpDT - 1) / nfp::kCpDT; }
int cpool_rtiles(int D) { return (D + nfp::kCpRT - 1) / nfp::kCpRT; }
int cpw_np(int N) { return (N + 15) & ~15; }
// pixels per chunk: the whole image where its maps and ga fit kWBudget floats of LDS beside the rows, else a multiple of 64
// (64 at 64 maps and more, 128 at 32 and 48, 192 at 16)
int cpw_chunk(int NP, long long P) {
  return (int)std::min<long long>(P, std::max(64, (nfp::kWBudget / (NP + nfp::kWRS)) & ~63));
}
int cpw_tiles(int D) { return (D + nfp::kWDT - 1) / nfp::kWDT; }
// pixels per workgroup of cproj_fwd: cpool_chunk, halved (down to 256) while the grid has fewer than 1024 workgroups
int cproj_fwd_chunk(int NP, long long B, long long P, int D) {
  const long long tiles = (D + nfp::kCjDT - 1) / nfp::kCjDT;
  long long ch = cpool_chunk(NP, P);
  while (ch > 256 && B * ((P + ch - 1) / ch) * tiles < 1024) ch = std::max<long long>(256, (ch / 2) & ~63LL);
  return (int)ch;
}

int cpool_args(const char* what, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int training, bool wide = false) {
  const int maxN = wide ? nfp::kWMaxN : nfp::kCpMaxN;
  if (B < 0 || N < 1 || P < 1 || D < 1)
    return fail(NFP_E_INVALID, "%s: B = %d, N = %d, P = %lld, D = %d", what, B, N, (long long)P, D);
  if (dtype != NFP_F32 && dtype != NFP_BF16) return fail(NFP_E_INVALID, "%s: unknown dtype %d", what, dtype);
  if (N > maxN) return fail(NFP_E_UNSUPPORTED, "%s: N = %d maps (more than %d) has no kernel", what, N, maxN);
  if ((long long)N * P >= (1LL << 31))
    return fail(NFP_E_UNSUPPORTED, "%s: an image of N * P = %lld map elements (2^31 and more) has no kernel", what,
                (long long)N * P);
  if (D > (1 << 22)) return fail(NFP_E_UNSUPPORTED, "%s: D = %d (more than 2^22) has no kernel", what, D);
  const long long ch = wide ? cpw_chunk(cpw_np(N), P) : cpool_chunk(cpool_np(N), P), nc = (P + ch - 1) / ch;
  if ((long long)B * std::max<long long>(nc, (P + 63) / 64) >= (1LL << 31))
    return fail(NFP_E_UNSUPPORTED, "%s: B = %d images of P = %lld pixels make 2^31 workgroups and more", what, B, (long long)P);
  if (training && B > 0 && (long long)B * P < 2)
    return fail(NFP_E_UNSUPPORTED, "%s: train-mode statistics need B * P >= 2 values per channel", what);
  return NFP_OK;
}
int cproj_args(const char* what, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int training) {
  if (int rc = cpool_args(what, B, N, P, D, dtype, training)) return rc;
  if ((long long)D * P >= (1LL << 31))
    return fail(NFP_E_UNSUPPORTED, "%s: an image of D * P = %lld output elements (2^31 and more) has no kernel", what,
                (long long)D * P);
  const long long tiles = (D + nfp::kCjDT - 1) / nfp::kCjDT, ch = cproj_fwd_chunk(cpool_np(N), std::max(B, 1), P, D);
  if ((long long)B * ((P + ch - 1) / ch) * tiles >= (1LL << 31))
    return fail(NFP_E_UNSUPPORTED, "%s: B = %d, P = %lld, D = %d make 2^31 workgroups and more", what, B, (long long)P, D);
  return NFP_OK;
}
int cproj_layout(const char* what, int32_t layout) {
  if (layout != NFP_ACT_NCHW && layout != NFP_ACT_NHWC)
    return fail(NFP_E_INVALID, "%s: unknown layout %d (NFP_ACT_NCHW = 0, NFP_ACT_NHWC = 1)", what, layout);
  return NFP_OK;
}

// ---- the launch shape of a call: decided here, once per direction ----
int cp_np(const CpCall& c) { return c.kind == kCpWide ? cpw_np(c.N) : cpool_np(c.N); }
// Forward, and every kernel that walks an image chunk by chunk: the pixels per chunk, the floats between two of its rows in
// LDS and the chunks per image.  proj_fwd: cproj_fwd's own, finer chunks (the statistics ahead of it walk the pooled kind's).
void cp_chunks(const CpCall& c, nfp::CpK& k, bool proj_fwd = false) {
  const int NP = cp_np(c);
  k.CH = c.kind == kCpWide ? cpw_chunk(NP, c.P) : proj_fwd ? cproj_fwd_chunk(NP, std::max(c.B, 1), c.P, c.D) : cpool_chunk(NP, c.P);
  k.CHs = cpool_stride(k.CH), k.nc = (int)((c.P + k.CH - 1) / k.CH);
}
// Backward: the units a workgroup of *_bwd_part takes — images; proj_part: cproj_bwd_part's passes of 64 pixels, which are
// then its chunk — and the slices of the batch that makes: about 512 workgroups (every slice is read again by the few
// workgroups of *_bwd_reduce), at most one per unit
void cp_slices(const CpCall& c, nfp::CpK& k, bool proj_part = false) {
  const long long B = std::max(c.B, 1), units = proj_part ? B * ((c.P + nfp::kCjSP - 1) / nfp::kCjSP) : B;
  const long long want = std::min<long long>(units, std::max(1, 512 / (c.kind == kCpWide ? cpw_tiles(c.D) : cpool_tiles(c.D))));
  k.ipw = (int)((units + want - 1) / want), k.S = (int)((units + k.ipw - 1) / k.ipw);
  if (proj_part) k.CH = nfp::kCjSP, k.CHs = nfp::kCjSS;
}
// The call as every kernel reads it: sizes, dtype, mode, the maps and parameters, and the shape of the kernels that walk
// whole images.  The projection's two kernels that walk otherwise get theirs from cp_chunks / cp_slices where they launch.
nfp::CpK cp_k(const CpCall& c) {
  nfp::CpK k;
  memset(&k, 0, sizeof(k));
  k.B = c.B, k.N = c.N, k.P = (int)c.P, k.D = c.D;
  k.bf16 = c.dtype == NFP_BF16, k.eval = !c.training;
  k.ntr = cpool_rtiles(c.D), k.M = (double)c.B * (double)c.P;
  k.maps = c.maps, k.w = c.w, k.gamma = c.gamma, k.beta = c.beta;
  k.eps = (float)c.eps, k.eps64 = c.eps;
  cp_chunks(c, k), cp_slices(c, k);
  return k;
}
// ... with what a forward adds: the result (the projection's in the maps' dtype), and the statistics it computes and the
// running ones it updates (training) or reads (eval)
nfp::CpK cp_fwd_k(const CpCall& c) {
  nfp::CpK k = cp_k(c);
  k.mom = c.momentum;
  if (c.kind == kCpProj)
    k.outv = c.out;
  else
    k.out = (float*)c.out;
  if (c.training)
    k.stats_w = c.saved_w, k.stats = c.saved_w, k.rm_w = c.rm_w, k.rv_w = c.rv_w;
  else
    k.rm = c.rm_w, k.rv = c.rv_w;
  return k;
}
// ... and a backward: the saved statistics (eval: the running ones), the gradients wanted and, of a rank with images,
// grad_out
nfp::CpK cp_bwd_k(const CpCall& c) {
  nfp::CpK k = cp_k(c);
  k.stats = c.saved;
  if (!c.training) k.rm = c.rm, k.rv = c.rv;
  k.gm = c.gm, k.gw = c.gw, k.gg = c.gg, k.gb = c.gb;
  if (c.B > 0) {
    if (c.kind == kCpProj)
      k.gov = c.go;
    else
      k.go = (const float*)c.go;
  }
  return k;
}

// ---- the scratch of a call, laid out once ----
// Forward (training): a record [2 N + N*N] per chunk of the batch; wide: then, from an even float on, mu [N] and Sigma [N*N]
// as doubles.  Backward: the slices' partials [S][D][N + 1], then the workgroups' shares of k, Q [ntr][N + N*N].
int64_t cp_records(const CpCall& c, const nfp::CpK& k) {
  const int64_t n = (int64_t)c.B * k.nc * (2 * c.N + c.N * c.N);
  return c.kind == kCpWide ? (n + 1) & ~(int64_t)1 : n;
}
int64_t cp_parts(const nfp::CpK& k) { return (int64_t)k.S * k.D * (k.N + 1); }
// what nfp_cpool_scratch_floats, nfp_cpool_wide_scratch_floats and nfp_cproj_scratch_floats answer for the sizes they serve
int64_t cp_scratch_floats(CpKind kind, int32_t B, int32_t N, int64_t P, int32_t D, int32_t backward) {
  const CpCall c = cp_call("", kind, B, N, P, D, NFP_F32, 1, nullptr, nullptr, nullptr, nullptr);
  nfp::CpK k = cp_k(c);
  if (!backward) return std::max<int64_t>(1, cp_records(c, k) + (kind == kCpWide ? 2 * ((int64_t)N + (int64_t)N * N) : 0));
  cp_slices(c, k, kind == kCpProj);
  return std::max<int64_t>(1, cp_parts(k) + (int64_t)k.ntr * (N + N * N));
}

// ---- the checks ----
// The refusals both directions share, in order: layout, sizes, pointers (io: the forward's out, the backward's grad_out)
int cp_check(const CpCall& c, const void* io) {
  if (c.kind == kCpProj)
    if (int rc = cproj_layout(c.what, c.layout)) return rc;
  const int own = c.training && !c.sync;   // (the statistics come from this call's maps alone)
  if (int rc = c.kind == kCpProj ? cproj_args(c.what, c.B, c.N, c.P, c.D, c.dtype, own)
                                 : cpool_args(c.what, c.B, c.N, c.P, c.D, c.dtype, own, c.kind == kCpWide))
    return rc;
  if (!c.w || !c.gamma || !c.beta || (c.B > 0 && (!c.maps || !io))) return fail(NFP_E_INVALID, "%s: null tensor pointer", c.what);
  return NFP_OK;
}
int cp_check_scratch(const CpCall& c, int backward) {
  const auto query = c.kind == kCpProj ? nfp_cproj_scratch_floats
                     : c.kind == kCpWide ? nfp_cpool_wide_scratch_floats : nfp_cpool_scratch_floats;
  const char* name = c.kind == kCpProj ? "nfp_cproj_scratch_floats"
                     : c.kind == kCpWide ? "nfp_cpool_wide_scratch_floats" : "nfp_cpool_scratch_floats";
  const int64_t need = query(c.B, c.N, c.P, c.D, backward);
  if (c.B > 0 && (c.scratch == nullptr || c.scratch_floats < need))
    return fail(NFP_E_INVALID, "%s: scratch holds %lld floats, %s is %lld", c.what, (long long)(c.scratch ? c.scratch_floats : 0),
                name, (long long)need);
  return NFP_OK;
}
void cp_variant(const CpCall& c, const char* dir) {
  const char *dt = c.dtype == NFP_BF16 ? "bf16" : "f32", *mode = c.training ? "train" : "eval";
  if (c.kind == kCpPool)
    snprintf(g_variant, sizeof(g_variant), "cpool_%s<%s,%s>", dir, dt, mode);
  else if (c.kind == kCpWide)
    snprintf(g_variant, sizeof(g_variant), "cpool_wide_%s<%s,%s,n%d>", dir, dt, mode, cpw_np(c.N));
  else
    snprintf(g_variant, sizeof(g_variant), "cproj_%s<%s,%s,%s%s>", dir, dt, mode, c.relu ? "relu" : "lin",
             c.layout == NFP_ACT_NHWC ? ",nhwc" : "");
}

// ---- call fields -> kernel template arguments (as nfp_launch.h's with_* helpers) ----
// the padded maps count of the pooled kind and the projection
template <typename F>
int with_np(const CpCall& c, F&& f) {
  switch (cpool_np(c.N)) {
    case 8: return f(Int<8>{});
    case 16: return f(Int<16>{});
    case 24: return f(Int<24>{});
    default: return f(Int<32>{});
  }
}
template <typename F>
int with_flag(bool v, F&& f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}
// the projection's f(RELU, NHWC) — NHWC: the channels-last forms (out / grad_out [b][p][d]), the same grids, LDS sizes and scratch
template <typename F>
int with_act(const CpCall& c, F&& f) {
  return with_flag(c.relu != 0, [&](auto relu) {
    return with_flag(c.layout == NFP_ACT_NHWC, [&](auto nhwc) { return f(relu, nhwc); });
  });
}

// ---- the steps of a forward ----
// cpool_moments: a record per chunk into the scratch (its caller has pointed k.part there)
int cp_launch_moments(const CpCall& c, const nfp::CpK& k) {
  const int NP = cp_np(c);
  const size_t lds = ((size_t)NP * k.CHs + NP + std::max(NP * NP, nfp::kCpMT)) * sizeof(float);
  return launch("cpool_moments", nfp::cpool_moments, dim3((unsigned)((long long)k.B * k.nc)), dim3(nfp::kCpMT), lds, cp_stream(c), k,
                NP);
}
// The train-mode statistics of this call's maps alone: cpool_moments + cpool_finish; wide: cpw_moments, cpw_mu, cpw_sigma,
// cpw_var
int cp_local_stats(const CpCall& c, nfp::CpK& k) {
  hipStream_t st = cp_stream(c);
  k.part_w = c.scratch, k.part = c.scratch;
  if (c.kind != kCpWide) {
    int rc = cp_launch_moments(c, k);
    if (rc == NFP_OK)
      rc = launch("cpool_finish", nfp::cpool_finish, dim3((unsigned)((k.D + nfp::kCpFT - 1) / nfp::kCpFT)), dim3(nfp::kCpFT), 0, st,
                  k);
    return rc;
  }
  const int NP = cp_np(c), NN = k.N * k.N;
  double* mu64 = (double*)(c.scratch + cp_records(c, k));
  double* sig64 = mu64 + k.N;
  int rc = launch("cpw_moments", nfp::cpw_moments, dim3((unsigned)((long long)k.B * k.nc)), dim3(nfp::kWT),
                  ((size_t)NP * k.CHs + NP) * sizeof(float), st, k, NP);
  if (rc == NFP_OK) rc = launch("cpw_mu", nfp::cpw_mu, dim3(1), dim3(nfp::kWMuT), 0, st, k, mu64);
  if (rc == NFP_OK)
    rc = launch("cpw_sigma", nfp::cpw_sigma, dim3((unsigned)((NN + 63) / 64)), dim3(nfp::kWT), 0, st, k, (const double*)mu64, sig64);
  if (rc == NFP_OK)
    rc = launch("cpw_var", nfp::cpw_var, dim3((unsigned)((k.D + 15) / 16)), dim3(nfp::kWT), 0, st, k, (const double*)mu64,
                (const double*)sig64);
  return rc;
}
// The rank's record for the other ranks: cpool_moments (where it has an image) + cps_record
int cps_rank_record(const CpCall& c, nfp::CpK& k, double* record) {
  k.part_w = c.scratch, k.part = c.scratch;
  int rc = c.B > 0 ? cp_launch_moments(c, k) : NFP_OK;
  if (rc == NFP_OK) rc = launch("cps_record", nfp::cps_record, dim3(1), dim3(nfp::kCpFT), 0, cp_stream(c), k, record);
  return rc;
}
// The statistics joined from every rank's record: cps_finish
int cps_joined_stats(const CpCall& c, const nfp::CpK& k, const double* records, int32_t world) {
  return launch("cps_finish", nfp::cps_finish, dim3((unsigned)((k.D + nfp::kCpFT - 1) / nfp::kCpFT)), dim3(nfp::kCpFT), 0,
                cp_stream(c), k, records, (int)world);
}
// The main forward under the statistics k names: cpool_fwd, cpw_fwd, or cproj_fwd (either layout) over chunks of its own
int cp_main_forward(const CpCall& c, nfp::CpK& k) {
  const int NP = cp_np(c);
  hipStream_t st = cp_stream(c);
  if (c.kind == kCpWide) {
    const size_t lds = ((size_t)NP * nfp::kWRS + 2 * nfp::kWDT + (size_t)NP * k.CHs + 16 * nfp::kWDT) * sizeof(float);
    return launch("cpw_fwd", nfp::cpw_fwd, dim3((unsigned)k.B, (unsigned)cpw_tiles(k.D)), dim3(nfp::kWT), lds, st, k, NP);
  }
  if (c.kind == kCpPool) {
    const size_t lds = ((size_t)NP * k.CHs + nfp::kCpW * nfp::kCpDT) * sizeof(float);
    return with_np(c, [&](auto np) {
      return launch("cpool_fwd", nfp::cpool_fwd<decltype(np)::value>, dim3((unsigned)k.B, (unsigned)cpool_tiles(k.D)),
                    dim3(nfp::kCpT), lds, st, k);
    });
  }
  cp_chunks(c, k, true);
  const int tiles = (k.D + nfp::kCjDT - 1) / nfp::kCjDT;
  const size_t lds = ((size_t)NP * k.CHs + (size_t)nfp::kCjDT * (NP + 1)) * sizeof(float);
  const dim3 grid((unsigned)((long long)k.B * k.nc * tiles));
  // two bf16 elements per lane where every pair is an aligned dword of one tile (cproj_fwd's PAIR)
  const bool pair = k.bf16 && ((uintptr_t)k.outv & 3) == 0 && (tiles == 1 || (k.D & 1) == 0);
  return with_np(c, [&](auto np) {
    return with_act(c, [&](auto relu, auto nhwc) {
      constexpr int kNP = decltype(np)::value;
      constexpr bool kRelu = decltype(relu)::value;
      if constexpr (!decltype(nhwc)::value)
        return launch("cproj_fwd", nfp::cproj_fwd<kNP, kRelu, false>, grid, dim3(nfp::kCjT), lds, st, k, tiles);
      else if (pair)
        return launch("cproj_fwd_nhwc", nfp::cproj_fwd<kNP, kRelu, true, true>, grid, dim3(nfp::kCjT), lds, st, k, tiles);
      else
        return launch("cproj_fwd_nhwc", nfp::cproj_fwd<kNP, kRelu, true, false>, grid, dim3(nfp::kCjT), lds, st, k, tiles);
    });
  });
}

// ---- the steps of a backward (k sliced by cp_slices) ----
// The batch sums: *_bwd_part writes every slice's partials, *_bwd_reduce joins them into the parameter gradients and the
// workgroups' shares of k, Q behind them (cpool_bwd_reduce: LIVE = the projection, SYNC = the call's)
int cp_sums(const CpCall& c, nfp::CpK& k) {
  const int NP = cp_np(c);
  hipStream_t st = cp_stream(c);
  k.part_w = c.scratch, k.part = c.scratch;
  k.kq_w = c.scratch + cp_parts(k), k.kq = k.kq_w;
  if (c.kind == kCpWide) {
    const size_t lds = ((size_t)NP * nfp::kWRS + 3 * nfp::kWDT + (size_t)(NP + nfp::kWRS) * k.CHs) * sizeof(float);
    const size_t lds_r = ((size_t)nfp::kCpRT * (2 * k.N + 1) + (size_t)k.N * k.N) * sizeof(float);
    int rc = launch("cpw_bwd_part", nfp::cpw_bwd_part, dim3((unsigned)k.S, (unsigned)cpw_tiles(k.D)), dim3(nfp::kWT), lds, st, k, NP);
    if (rc == NFP_OK) rc = launch("cpw_bwd_reduce", nfp::cpw_bwd_reduce, dim3((unsigned)k.ntr), dim3(nfp::kWT), lds_r, st, k);
    return rc;
  }
  const dim3 grid((unsigned)k.S, (unsigned)cpool_tiles(k.D));
  const int rc = with_np(c, [&](auto np) {
    constexpr int kNP = decltype(np)::value;
    const dim3 block(nfp::cp_part_threads<kNP>());
    if (c.kind == kCpPool) {
      const size_t lds = ((size_t)kNP * k.CHs + (size_t)nfp::kCpDT * (kNP + 1)) * sizeof(float);
      return launch("cpool_bwd_part", nfp::cpool_bwd_part<kNP>, grid, block, lds, st, k);
    }
    const size_t lds = ((size_t)kNP + nfp::kCpDT) * nfp::kCjSS * sizeof(float);
    return with_act(c, [&](auto relu, auto nhwc) {
      constexpr bool kNhwc = decltype(nhwc)::value;
      return launch(kNhwc ? "cproj_bwd_part_nhwc" : "cproj_bwd_part", nfp::cproj_bwd_part<kNP, decltype(relu)::value, kNhwc>, grid,
                    block, lds, st, k, (k.P + nfp::kCjSP - 1) / nfp::kCjSP, k.ipw);
    });
  });
  if (rc != NFP_OK) return rc;
  return with_flag(c.kind == kCpProj, [&](auto live) {
    return with_flag(c.sync != 0, [&](auto sync) {
      return launch("cpool_bwd_reduce", nfp::cpool_bwd_reduce<decltype(live)::value, decltype(sync)::value>, dim3((unsigned)k.ntr),
                    dim3(nfp::kCpMT), 0, st, k);
    });
  });
}
// The rank's row of k, Q for the other ranks: cps_kq_row sums the workgroups' shares; cps_zero for a rank without an image
// (a zero row, zero parameter gradients)
int cps_rank_row(const CpCall& c, const nfp::CpK& k, float* row) {
  if (c.B > 0) return launch("cps_kq_row", nfp::cps_kq_row, dim3(1), dim3(nfp::kCpMT), 0, cp_stream(c), k, row);
  const long long n = std::max<long long>((long long)c.D * c.N, (int64_t)c.N + (int64_t)c.N * c.N);
  return launch("cps_zero", nfp::cps_zero, dim3((unsigned)std::min<long long>(1024, (n + nfp::kCpMT - 1) / nfp::kCpMT)),
                dim3(nfp::kCpMT), 0, cp_stream(c), k, row);
}
// grad_maps, under the k, Q rows that k.kq / k.ntr name
int cp_grad_maps(const CpCall& c, const nfp::CpK& k) {
  const int NP = cp_np(c), npt = (k.P + 63) / 64;
  hipStream_t st = cp_stream(c);
  const dim3 grid((unsigned)((long long)k.B * npt));
  if (c.kind == kCpWide) {
    const size_t lds = ((size_t)2 * NP * nfp::kWRS + 3 * nfp::kWDT + (size_t)nfp::kWDT * nfp::kWRS) * sizeof(float);
    return launch("cpw_bwd_maps", nfp::cpw_bwd_maps, grid, dim3(nfp::kWT), lds, st, k, NP, npt);
  }
  return with_np(c, [&](auto np) {
    constexpr int kNP = decltype(np)::value;
    if (c.kind == kCpPool)
      return launch("cpool_bwd_maps", nfp::cp_bwd_maps<kNP, nfp::kCpGradPooled, true>, grid, dim3(nfp::kCpT), 0, st, k, npt);
    return with_act(c, [&](auto relu, auto nhwc) {
      constexpr nfp::CpGrad kSrc = decltype(nhwc)::value ? nfp::kCpGradNhwc : nfp::kCpGradNchw;
      return launch(kSrc == nfp::kCpGradNhwc ? "cproj_bwd_maps_nhwc" : "cproj_bwd_maps",
                    nfp::cp_bwd_maps<kNP, kSrc, decltype(relu)::value>, grid, dim3(nfp::kCpT), 0, st, k, npt);
    });
  });
}

// ---- a call on one rank's own statistics (nfp_cpool_*, nfp_cpool_wide_*, nfp_cproj_*) ----
int cp_forward(const CpCall& c) {
  if (int rc = cp_check(c, c.out)) return rc;
  if ((c.rm_w == nullptr) != (c.rv_w == nullptr) || (!c.training && c.rm_w == nullptr))
    return fail(NFP_E_INVALID, "%s: running_mean and running_var come together (eval needs both)", c.what);
  if (!(c.eps >= 0.0) || !(c.momentum == c.momentum))
    return fail(NFP_E_INVALID, "%s: eps = %g, momentum = %g", c.what, c.eps, c.momentum);
  if (c.training) {
    if (c.saved_w == nullptr || c.saved_floats < nfp_cpool_saved_floats(c.N, c.D))
      return fail(NFP_E_INVALID, "%s: saved holds %lld floats, nfp_cpool_saved_floats is %lld", c.what,
                  (long long)(c.saved_w ? c.saved_floats : 0), (long long)nfp_cpool_saved_floats(c.N, c.D));
    if (int rc = cp_check_scratch(c, 0)) return rc;
  }
  if (c.B == 0) return NFP_OK;
  nfp::CpK k = cp_fwd_k(c);
  cp_variant(c, "fwd");
  int rc = c.training ? cp_local_stats(c, k) : NFP_OK;
  if (rc == NFP_OK) rc = cp_main_forward(c, k);
  if (rc == NFP_OK) publish_variant();
  return rc;
}

int cp_backward(const CpCall& c) {
  if (int rc = cp_check(c, c.go)) return rc;
  if (!c.training && (c.rm == nullptr || c.rv == nullptr))
    return fail(NFP_E_INVALID, "%s: eval needs running_mean and running_var", c.what);
  if (!(c.eps >= 0.0)) return fail(NFP_E_INVALID, "%s: eps = %g", c.what, c.eps);
  if (c.training && (c.saved == nullptr || c.saved_floats < nfp_cpool_saved_floats(c.N, c.D)))
    return fail(NFP_E_INVALID, "%s: saved holds %lld floats, nfp_cpool_saved_floats is %lld", c.what,
                (long long)(c.saved ? c.saved_floats : 0), (long long)nfp_cpool_saved_floats(c.N, c.D));
  const bool params = c.gw != nullptr || c.gg != nullptr || c.gb != nullptr;
  if (!params && c.gm == nullptr) return NFP_OK;
  const bool sums = params || c.training;   // (train-mode grad_maps needs k and Q: the batch sums)
  if (sums)
    if (int rc = cp_check_scratch(c, 1)) return rc;
  if (c.B == 0) return NFP_OK;
  nfp::CpK k = cp_bwd_k(c);
  cp_slices(c, k, c.kind == kCpProj);
  cp_variant(c, "bwd");
  int rc = sums ? cp_sums(c, k) : NFP_OK;
  if (rc == NFP_OK && c.gm != nullptr) rc = cp_grad_maps(c, k);
  if (rc == NFP_OK) publish_variant();
  return rc;
}

// ... with the direction's own arguments filled in behind the entry's leading fields
int cp_forward(CpCall c, float* running_mean, float* running_var, double momentum, void* out, float* saved) {
  c.rm_w = running_mean, c.rv_w = running_var, c.momentum = momentum, c.out = out, c.saved_w = saved;
  return cp_forward(c);
}
int cp_backward(CpCall c, const float* running_mean, const float* running_var, const float* saved, const void* grad_out,
                void* grad_maps, float* grad_w, float* grad_gamma, float* grad_beta) {
  c.rm = running_mean, c.rv = running_var, c.saved = saved, c.go = grad_out;
  c.gm = grad_maps, c.gw = grad_w, c.gg = grad_gamma, c.gb = grad_beta;
  return cp_backward(c);
}

// ---- the staged calls of a step whose statistics span ranks (nfp_cpsync_*) ----
int64_t cps_record_len(int32_t N) { return 1 + (int64_t)N + (int64_t)N * N; }
int64_t cps_row_len(int32_t N) { return (int64_t)N + (int64_t)N * N; }

// What the four calls of a kind share behind cp_check: the kind itself, eps, and `saved` with its length
int cps_check(const CpCall& c, int32_t kind, const void* io, const float* saved) {
  if (kind != NFP_CP_POOL && kind != NFP_CP_PROJ)
    return fail(NFP_E_INVALID, "%s: unknown kind %d (NFP_CP_POOL = 0, NFP_CP_PROJ = 1)", c.what, kind);
  if (int rc = cp_check(c, io)) return rc;
  if (!(c.eps >= 0.0)) return fail(NFP_E_INVALID, "%s: eps = %g", c.what, c.eps);
  if (saved == nullptr || c.saved_floats < nfp_cpsync_saved_floats(c.N, c.D))
    return fail(NFP_E_INVALID, "%s: saved holds %lld floats, nfp_cpsync_saved_floats is %lld", c.what,
                (long long)(saved ? c.saved_floats : 0), (long long)nfp_cpsync_saved_floats(c.N, c.D));
  return NFP_OK;
}
// `world` gathered rows of `len` elements each, behind a pointer aligned to `align` bytes
int cps_rows(const char* what, const char* name, const void* p, int32_t world, int64_t have, int64_t len, size_t align) {
  if (world < 1) return fail(NFP_E_INVALID, "%s: world = %d ranks", what, world);
  if (p == nullptr || have < (int64_t)world * len)
    return fail(NFP_E_INVALID, "%s: %s holds %lld elements, %d ranks need %lld", what, name, (long long)(p ? have : 0), world,
                (long long)world * len);
  if ((uintptr_t)p % align != 0) return fail(NFP_E_INVALID, "%s: %s is not aligned to %zu bytes", what, name, align);
  return NFP_OK;
}
void cps_variant(const CpCall& c, const char* stage) {
  snprintf(g_variant, sizeof(g_variant), "cpsync_%s<%s,%s%s>", stage, c.kind == kCpPool ? "pool" : c.relu ? "proj,relu" : "proj,lin",
           c.dtype == NFP_BF16 ? "bf16" : "f32", c.kind == kCpProj && c.layout == NFP_ACT_NHWC ? ",nhwc" : "");
}
// The CpCall of nfp_cpsync_forward / _reduce / _maps: training mode with `sync` set; the pooled kind is always NCHW with
// the ReLU, whatever the entry was handed
CpCall cps_call(const char* what, int32_t kind, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t relu,
                int32_t layout, const void* maps, const float* w, const float* gamma, const float* beta) {
  const bool proj = kind == NFP_CP_PROJ;
  CpCall c = cp_call(what, proj ? kCpProj : kCpPool, B, N, P, D, dtype, 1, maps, w, gamma, beta);
  if (proj) c.relu = relu, c.layout = layout;
  c.sync = 1;
  return c;
}

int cps_moments(const CpCall& c, double* record, int64_t record_doubles) {
  if (int rc = cpool_args(c.what, c.B, c.N, c.P, 1, c.dtype, 0)) return rc;
  if (c.B > 0 && c.maps == nullptr) return fail(NFP_E_INVALID, "%s: null tensor pointer", c.what);
  if (int rc = cps_rows(c.what, "record", record, 1, record_doubles, cps_record_len(c.N), sizeof(double))) return rc;
  if (int rc = cp_check_scratch(c, 0)) return rc;
  nfp::CpK k = cp_fwd_k(c);
  snprintf(g_variant, sizeof(g_variant), "cpsync_moments<%s>", c.dtype == NFP_BF16 ? "bf16" : "f32");
  const int rc = cps_rank_record(c, k, record);
  if (rc == NFP_OK) publish_variant();
  return rc;
}

int cps_forward(const CpCall& c, int32_t kind, const double* records, int32_t world, int64_t records_doubles,
                int64_t global_count) {
  if (int rc = cps_check(c, kind, c.out, c.saved_w)) return rc;
  if ((c.rm_w == nullptr) != (c.rv_w == nullptr))
    return fail(NFP_E_INVALID, "%s: running_mean and running_var come together", c.what);
  if (!(c.momentum == c.momentum)) return fail(NFP_E_INVALID, "%s: momentum = %g", c.what, c.momentum);
  if (int rc = cps_rows(c.what, "records", records, world, records_doubles, cps_record_len(c.N), sizeof(double))) return rc;
  if (global_count < 0) return fail(NFP_E_INVALID, "%s: global_count = %lld", c.what, (long long)global_count);
  if (global_count == 1 || (global_count > 0 && global_count < (int64_t)c.B * c.P))
    return fail(NFP_E_UNSUPPORTED, "%s: train-mode statistics need 2 values per channel over all ranks and no fewer than this "
                "rank's %lld, got global_count = %lld", c.what, (long long)c.B * (long long)c.P, (long long)global_count);
  nfp::CpK k = cp_fwd_k(c);
  cps_variant(c, "fwd");
  int rc = cps_joined_stats(c, k, records, world);
  if (rc == NFP_OK && c.B > 0) rc = cp_main_forward(c, k);
  if (rc == NFP_OK) publish_variant();
  return rc;
}

int cps_reduce(const CpCall& c, int32_t kind, float* kq_row, int64_t kq_floats) {
  if (int rc = cps_check(c, kind, c.go, c.saved)) return rc;
  if (int rc = cps_rows(c.what, "kq_row", kq_row, 1, kq_floats, cps_row_len(c.N), sizeof(float))) return rc;
  if (int rc = cp_check_scratch(c, 1)) return rc;
  nfp::CpK k = cp_bwd_k(c);
  cps_variant(c, "bwd_reduce");
  int rc = NFP_OK;
  if (c.B > 0) {
    cp_slices(c, k, c.kind == kCpProj);
    rc = cp_sums(c, k);
  }
  if (rc == NFP_OK) rc = cps_rank_row(c, k, kq_row);
  if (rc == NFP_OK) publish_variant();
  return rc;
}

int cps_maps(const CpCall& c, int32_t kind, const float* kq_rows, int32_t world, int64_t kq_floats) {
  if (int rc = cps_check(c, kind, c.go, c.saved)) return rc;
  if (int rc = cps_rows(c.what, "kq_rows", kq_rows, world, kq_floats, cps_row_len(c.N), sizeof(float))) return rc;
  if (c.B > 0 && c.gm == nullptr) return fail(NFP_E_INVALID, "%s: null tensor pointer", c.what);
  if (c.B == 0) return NFP_OK;
  nfp::CpK k = cp_bwd_k(c);
  k.kq = kq_rows, k.ntr = world;   // (the ranks' rows, summed in rank order where the workgroups' shares are)
  cps_variant(c, "bwd_maps");
  const int rc = cp_grad_maps(c, k);
  if (rc == NFP_OK) publish_variant();
  return rc;
}

}  // namespace
}  // namespace nfp_host

using namespace nfp_host;

extern "C" {

int64_t nfp_cpool_saved_floats(int32_t N, int32_t D) {
  if (N < 1 || D < 1) return 1;
  return 2 * (int64_t)N + (int64_t)N * N + D;
}

int64_t nfp_cpool_scratch_floats(int32_t B, int32_t N, int64_t P, int32_t D, int32_t backward) {
  if (B < 1 || N < 1 || N > nfp::kCpMaxN || P < 1 || D < 1) return 1;
  return cp_scratch_floats(kCpPool, B, N, P, D, backward);
}

int64_t nfp_cpool_wide_scratch_floats(int32_t B, int32_t N, int64_t P, int32_t D, int32_t backward) {
  if (B < 1 || N < 1 || N > nfp::kWMaxN || P < 1 || D < 1) return 1;
  return cp_scratch_floats(kCpWide, B, N, P, D, backward);
}

int64_t nfp_cproj_scratch_floats(int32_t B, int32_t N, int64_t P, int32_t D, int32_t backward) {
  if (B < 1 || N < 1 || N > nfp::kCpMaxN || P < 1 || D < 1) return 1;
  return cp_scratch_floats(kCpProj, B, N, P, D, backward);
}

// The eight entries of one rank's call: cp_call of the leading arguments, cp_buffers, and cp_forward / cp_backward with the
// direction's own.

int nfp_cpool_forward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, const void* maps,
                      const float* w, const float* gamma, const float* beta, float* running_mean, float* running_var,
                      double momentum, double eps, float* out, float* saved, int64_t saved_floats, float* scratch,
                      int64_t scratch_floats, void* hip_stream) {
  CpCall c = cp_call("nfp_cpool_forward", kCpPool, B, N, P, D, dtype, training, maps, w, gamma, beta);
  cp_buffers(c, eps, saved_floats, scratch, scratch_floats, hip_stream);
  return cp_forward(c, running_mean, running_var, momentum, out, saved);
}

int nfp_cpool_backward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, const void* maps,
                       const float* w, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, double eps, const float* saved, int64_t saved_floats, const float* grad_out,
                       void* grad_maps, float* grad_w, float* grad_gamma, float* grad_beta, float* scratch,
                       int64_t scratch_floats, void* hip_stream) {
  CpCall c = cp_call("nfp_cpool_backward", kCpPool, B, N, P, D, dtype, training, maps, w, gamma, beta);
  cp_buffers(c, eps, saved_floats, scratch, scratch_floats, hip_stream);
  return cp_backward(c, running_mean, running_var, saved, grad_out, grad_maps, grad_w, grad_gamma, grad_beta);
}

int nfp_cpool_wide_forward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, const void* maps,
                           const float* w, const float* gamma, const float* beta, float* running_mean, float* running_var,
                           double momentum, double eps, float* out, float* saved, int64_t saved_floats, float* scratch,
                           int64_t scratch_floats, void* hip_stream) {
  CpCall c = cp_call("nfp_cpool_wide_forward", kCpWide, B, N, P, D, dtype, training, maps, w, gamma, beta);
  cp_buffers(c, eps, saved_floats, scratch, scratch_floats, hip_stream);
  return cp_forward(c, running_mean, running_var, momentum, out, saved);
}

int nfp_cpool_wide_backward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, const void* maps,
                            const float* w, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, double eps, const float* saved, int64_t saved_floats,
                            const float* grad_out, void* grad_maps, float* grad_w, float* grad_gamma, float* grad_beta,
                            float* scratch, int64_t scratch_floats, void* hip_stream) {
  CpCall c = cp_call("nfp_cpool_wide_backward", kCpWide, B, N, P, D, dtype, training, maps, w, gamma, beta);
  cp_buffers(c, eps, saved_floats, scratch, scratch_floats, hip_stream);
  return cp_backward(c, running_mean, running_var, saved, grad_out, grad_maps, grad_w, grad_gamma, grad_beta);
}

int nfp_cproj_forward_fmt(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, int32_t relu,
                          const void* maps, const float* w, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, double momentum, double eps, void* out, float* saved, int64_t saved_floats,
                          float* scratch, int64_t scratch_floats, void* hip_stream, int32_t out_layout) {
  CpCall c = cp_call("nfp_cproj_forward_fmt", kCpProj, B, N, P, D, dtype, training, maps, w, gamma, beta);
  c.relu = relu, c.layout = out_layout;
  cp_buffers(c, eps, saved_floats, scratch, scratch_floats, hip_stream);
  return cp_forward(c, running_mean, running_var, momentum, out, saved);
}

int nfp_cproj_backward_fmt(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, int32_t relu,
                           const void* maps, const float* w, const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, double eps, const float* saved, int64_t saved_floats, const void* grad_out,
                           void* grad_maps, float* grad_w, float* grad_gamma, float* grad_beta, float* scratch,
                           int64_t scratch_floats, void* hip_stream, int32_t grad_out_layout) {
  CpCall c = cp_call("nfp_cproj_backward_fmt", kCpProj, B, N, P, D, dtype, training, maps, w, gamma, beta);
  c.relu = relu, c.layout = grad_out_layout;
  cp_buffers(c, eps, saved_floats, scratch, scratch_floats, hip_stream);
  return cp_backward(c, running_mean, running_var, saved, grad_out, grad_maps, grad_w, grad_gamma, grad_beta);
}

// nfp_cproj_forward / nfp_cproj_backward: the NCHW call under its own name
int nfp_cproj_forward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, int32_t relu,
                      const void* maps, const float* w, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, double momentum, double eps, void* out, float* saved, int64_t saved_floats,
                      float* scratch, int64_t scratch_floats, void* hip_stream) {
  CpCall c = cp_call("nfp_cproj_forward", kCpProj, B, N, P, D, dtype, training, maps, w, gamma, beta);
  c.relu = relu;
  cp_buffers(c, eps, saved_floats, scratch, scratch_floats, hip_stream);
  return cp_forward(c, running_mean, running_var, momentum, out, saved);
}

int nfp_cproj_backward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, int32_t relu,
                       const void* maps, const float* w, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, double eps, const float* saved, int64_t saved_floats, const void* grad_out,
                       void* grad_maps, float* grad_w, float* grad_gamma, float* grad_beta, float* scratch,
                       int64_t scratch_floats, void* hip_stream) {
  CpCall c = cp_call("nfp_cproj_backward", kCpProj, B, N, P, D, dtype, training, maps, w, gamma, beta);
  c.relu = relu;
  cp_buffers(c, eps, saved_floats, scratch, scratch_floats, hip_stream);
  return cp_backward(c, running_mean, running_var, saved, grad_out, grad_maps, grad_w, grad_gamma, grad_beta);
}

// ---- nfp_cpsync_*: the four staged entries, cps_call of the leading arguments ----

int64_t nfp_cpsync_record_doubles(int32_t N) { return N < 1 ? 1 : cps_record_len(N); }
int64_t nfp_cpsync_kq_floats(int32_t N) { return N < 1 ? 1 : cps_row_len(N); }
int64_t nfp_cpsync_saved_floats(int32_t N, int32_t D) {
  if (N < 1 || D < 1) return 1;
  return nfp_cpool_saved_floats(N, D) + 1 + (int64_t)N * N;
}

int nfp_cpsync_moments(int32_t B, int32_t N, int64_t P, int32_t dtype, const void* maps, double* record, int64_t record_doubles,
                       float* scratch, int64_t scratch_floats, void* hip_stream) {
  CpCall c = cps_call("nfp_cpsync_moments", NFP_CP_POOL, B, N, P, 1, dtype, 1, NFP_ACT_NCHW, maps, nullptr, nullptr, nullptr);
  cp_buffers(c, 0.0, 0, scratch, scratch_floats, hip_stream);
  return cps_moments(c, record, record_doubles);
}

int nfp_cpsync_forward(int32_t kind, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t relu, const void* maps,
                       const float* w, const float* gamma, const float* beta, float* running_mean, float* running_var,
                       double momentum, double eps, const double* records, int32_t world, int64_t records_doubles,
                       int64_t global_count, void* out, float* saved, int64_t saved_floats, void* hip_stream,
                       int32_t out_layout) {
  CpCall c = cps_call("nfp_cpsync_forward", kind, B, N, P, D, dtype, relu, out_layout, maps, w, gamma, beta);
  cp_buffers(c, eps, saved_floats, nullptr, 0, hip_stream);
  c.rm_w = running_mean, c.rv_w = running_var, c.momentum = momentum, c.out = out, c.saved_w = saved;
  return cps_forward(c, kind, records, world, records_doubles, global_count);
}

int nfp_cpsync_reduce(int32_t kind, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t relu, const void* maps,
                      const float* w, const float* gamma, const float* beta, double eps, const float* saved,
                      int64_t saved_floats, const void* grad_out, float* grad_w, float* grad_gamma, float* grad_beta,
                      float* kq_row, int64_t kq_floats, float* scratch, int64_t scratch_floats, void* hip_stream,
                      int32_t grad_out_layout) {
  CpCall c = cps_call("nfp_cpsync_reduce", kind, B, N, P, D, dtype, relu, grad_out_layout, maps, w, gamma, beta);
  cp_buffers(c, eps, saved_floats, scratch, scratch_floats, hip_stream);
  c.saved = saved, c.go = grad_out, c.gw = grad_w, c.gg = grad_gamma, c.gb = grad_beta;
  return cps_reduce(c, kind, kq_row, kq_floats);
}

int nfp_cpsync_maps(int32_t kind, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t relu, const void* maps,
                    const float* w, const float* gamma, const float* beta, double eps, const float* saved, int64_t saved_floats,
                    const void* grad_out, const float* kq_rows, int32_t world, int64_t kq_floats, void* grad_maps,
                    void* hip_stream, int32_t grad_out_layout) {
  CpCall c = cps_call("nfp_cpsync_maps", kind, B, N, P, D, dtype, relu, grad_out_layout, maps, w, gamma, beta);
  cp_buffers(c, eps, saved_floats, nullptr, 0, hip_stream);
  c.saved = saved, c.go = grad_out, c.gm = grad_maps;
  return cps_maps(c, kind, kq_rows, world, kq_floats);
}
}  // extern "C"
