// nfp_launch.h — host-side launch machinery shared by the translation units of libnfp_hip.so (nfp_hip.hip: C ABI and
// dispatch; nfp_generic.hip: the any-geometry kernels; nfp_table_fwd.hip / nfp_table_bwd.hip: the table kernels;
// nfp_tile_fwd.hip / nfp_tile_bwd.hip: the row-band kernels (nfp_tile_r3_fwd.hip / nfp_tile_r3_bwd.hip: their radius 3); nfp_bias.hip: NFPPooling(bias=True);
// nfp_attpool.hip: SimilarityAwarePooling's softmax-pool tail; nfp_valid.hip: unpadded maps; nfp_strided.hip: stride 2-4; nfp_cpool.hip: the heads'
// compress-BN-ReLU-GAP tail; nfp_deepten.hip: the Deep-TEN baseline's encoding layer), and the interface of each unit's launchers to the dispatcher (below).  Separate
// units so that they compile in parallel; everything here is `inline` (one instance per shared library).
//
// Also the one home of "descriptor field -> kernel template argument": with_radius, with_hot, with_measure, with_storage and
// with_storage_mixed (below, with the list of combinations that have no kernel), and of the dry run: DryFlag / DryRun next
// to launch(), kStandIn for its pointers, variant_suffix for a second launch's name.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "nfp_common.h"
#include "nfp_measures.h"   // (the dispatch ids kNormP1 / kNormP2 / kSymTerm; templates only, no code of its own)

namespace nfp_host {
using namespace nfp;

inline thread_local char g_err[512] = "";
// The dispatcher names the variant it picked in a buffer of the CALLING thread (forward and autograd's backward
// thread dispatch concurrently); a finished nfp_forward / nfp_backward publishes it under a lock as the process's
// "last variant", which nfp_last_variant() copies back into the reader's own thread.
inline thread_local char g_variant[64] = "";
inline thread_local char t_variant_out[64] = "";
inline std::mutex g_variant_mu;
inline char g_variant_last[64] = "";
inline std::atomic<uint64_t> g_launches{0};
inline std::atomic<void*> g_time_start{nullptr}, g_time_stop{nullptr};  // nfp_time_next_launch (process-wide: backward launches from autograd's thread)

inline void publish_variant() {
  std::lock_guard<std::mutex> lock(g_variant_mu);
  memcpy(g_variant_last, g_variant, sizeof(g_variant_last));
}

// Test / A-B switches, read from the environment ONCE when the library is loaded (and again only when a test
// calls nfp_reload_env): the launch path itself never reads it.
struct Switches {
  std::atomic<int> fwd_scalar{0}, bwd_atomic{0}, bwd_bands{0}, force_generic{0}, mfma{1}, tile_first{0};
  std::atomic<int> tile_wgs{0}, tile_lds_kb{0}, tile_cap{0};   // A/B overrides of the row-band launchers' constants (0: built-in)
  std::atomic<int> tile_max_grid{0};                           // (tests: a smaller launch-splitting threshold)
  std::atomic<int> pool_ticket{0};   // A/B: fused pooling tail, several row bands per image combined inside ONE launch by the
                                     // band that arrives last (nfp_common.h::pool_last_band).  Measured slower than what it
                                     // replaces (profiles/r04_e_…: 8.7 vs 6.9 us at the headline shape, 103 vs 91 us at
                                     // [256,16,112,112]): off by default
  std::atomic<int> gemm3{1};         // the matrix-core backward's second form (nfp_fast.h::bwd_gemm_phase3: every row tile's densified
                                     // weights written by phase A, x in double-buffered chunks) where its LDS fits; 0 = round 3's form
  std::atomic<int> tile_dma{-1};     // the channels-last row-band forward staged by LDS-DMA into a position-major slab
                                     // (nfp_tile.h::fwd_tile, DMA): -1 = where it measured faster — bf16 maps of 64 channels and
                                     // more per pixel (8 pieces per position: [256,128,28,28] 23.9 -> 18.8 us, [256,64,56,56] 44.2 ->
                                     // 42.2) — 0 = never, 1 = wherever it applies (float32 loses: 72 -> 121 us at
                                     // [256,16,112,112]; profiles/r04_h_…)
  std::atomic<int> tile_r3{-1};      // radius-3 "same" maps (k = 7) on the row-band kernels of nfp_tile.h: -1 = the default routing
                                     // (tile_r3_wanted below), 0 = never (fwd_pairs / bwd_gather, as before those instantiations
                                     // existed: the A/B arm), 1 = wherever they can serve
  std::atomic<int> stage_blocks{0};  // A/B, tests: NCHW maps staged in 4 x 4 blocks also where bwd_fast's launcher would stage
                                     // them by pixel rows (nfp_fast.h: StagedRows) — the two forms agree bitwise
};
inline Switches g_sw;
#ifndef NFP_MFMA_DEFAULT
#define NFP_MFMA_DEFAULT 1
#endif
#ifndef NFP_GEMM3_DEFAULT
#define NFP_GEMM3_DEFAULT 1
#endif
inline void read_env() {
  auto flag = [](const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? (e[0] == '1' ? 1 : 0) : dflt;
  };
  g_sw.fwd_scalar = flag("NFP_FWD_SCALAR", 0);
  g_sw.bwd_atomic = flag("NFP_BWD_ATOMIC", 0);
  g_sw.force_generic = flag("NFP_FORCE_GENERIC", 0);
  g_sw.mfma = flag("NFP_MFMA", NFP_MFMA_DEFAULT);
  g_sw.pool_ticket = flag("NFP_POOL_TICKET", 0);
  {
    const char* e = getenv("NFP_GEMM3");   // 0 = never, 1 = where the first form needs several rounds, 2 = wherever it fits (tests)
    g_sw.gemm3 = e ? (e[0] == '2' ? 2 : (e[0] == '1' ? 1 : 0)) : NFP_GEMM3_DEFAULT;
  }
  {
    const char* e = getenv("NFP_TILE_DMA");
    g_sw.tile_dma = e ? (e[0] == '1' ? 1 : 0) : -1;
  }
  {
    const char* e = getenv("NFP_TILE_R3");
    g_sw.tile_r3 = e ? (e[0] == '1' ? 1 : 0) : -1;
  }
  g_sw.stage_blocks = flag("NFP_STAGE_BLOCKS", 0);
  g_sw.tile_first = flag("NFP_TILE_FIRST", 0);   // A/B: the row-band kernels of nfp_tile.h also for maps the table kernels serve
  auto num = [](const char* name) {
    const char* e = getenv(name);
    return e ? atoi(e) : 0;
  };
  g_sw.bwd_bands = num("NFP_BWD_BANDS");
  g_sw.tile_wgs = num("NFP_TILE_WGS");
  g_sw.tile_lds_kb = num("NFP_TILE_LDS_KB");
  g_sw.tile_cap = num("NFP_TILE_CAP");
  g_sw.tile_max_grid = num("NFP_TILE_MAX_GRID");
}

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

inline int hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return NFP_OK;
  return fail(NFP_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

constexpr int kLdsMax = 160 * 1024;
constexpr int kNotApplicable = 1;  // internal: a hot-path launcher declined, use the generic kernels

// floats per input pixel that forward hands to backward
inline int stats_of(int measure) {
  switch (measure) {
    case NFP_COSINE: case NFP_GFC: case NFP_SMITH: return 1;
    case NFP_PEARSON: return 2;
    default: return 0;
  }
}

// Kernels that want more than 64 KiB of dynamic LDS must be told so once (per kernel and size class);
// remembered here so that steady-state launches make no extra runtime call.
template <typename K>
int set_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return NFP_OK;
  // hipFuncSetAttribute applies to the kernel ON THE CURRENT DEVICE: remembered per (device, kernel)
  static std::mutex mu;
  static std::unordered_map<uintptr_t, size_t> granted;
  int dev = 0;
  if (int rc = hip_ok(hipGetDevice(&dev), "hipGetDevice")) return rc;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = granted[(uintptr_t)(const void*)kernel * 64 + (uintptr_t)(dev & 63)];
  if (have >= bytes) return NFP_OK;
  if (int rc = hip_ok(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax),
                      "hipFuncSetAttribute(max dynamic LDS)"))
    return rc;
  have = kLdsMax;
  return NFP_OK;
}

// One way to launch: host-side limits first (a launch the hardware would refuse or fault on is never
// attempted), then the LDS opt-in, the launch and its error.  In plan mode (nfp_plan) nothing touches the
// GPU: the launch is only described, so the dispatcher's decisions are testable without a device.
inline thread_local bool t_dry = false;
inline thread_local char t_plan[512] = "";
// How the launch being made stages an NCHW map (" stage=rows" / " stage=blocks"; "" for every other launch): appended to
// its record in plan mode, behind lds=, so that the form shows without a change to variant strings.  Set and put back by
// launch_staged() alone, around its one call of launch().
inline thread_local const char* t_stage = "";
// The pointer a dry run hands the launchers for every buffer: 4 KiB-aligned, so every alignment rule passes
inline void* const kStandIn = (void*)(uintptr_t)0x1000;

// Plan mode for the guard's lifetime.  nfp_plan uses this part alone: it publishes t_plan and leaves g_variant / g_err as the
// dispatcher wrote them.
struct DryFlag {
  const bool was_dry = t_dry;
  DryFlag() { t_dry = true; }
  ~DryFlag() { t_dry = was_dry; }
};
// ... and the calling thread's variant, plan and error strings put back: a question about a descriptor ("would both
// launchers launch?" — nfp_pool_supported, nfp_gap_supported, nfp_valid_supported, nfp_valid_abs_supported and their
// saved_floats) leaves no trace
struct DryRun : DryFlag {
  char variant[sizeof(g_variant)], plan[sizeof(t_plan)], err[sizeof(g_err)];
  DryRun() {
    memcpy(variant, g_variant, sizeof(variant));
    memcpy(plan, t_plan, sizeof(plan));
    memcpy(err, g_err, sizeof(err));
  }
  ~DryRun() {
    memcpy(g_variant, variant, sizeof(variant));
    memcpy(t_plan, plan, sizeof(plan));
    memcpy(g_err, err, sizeof(err));
  }
};
// "+pool_fold" / "+attn_softmax": a second launch behind the one g_variant names
inline void variant_suffix(const char* s) { strncat(g_variant, s, sizeof(g_variant) - strlen(g_variant) - 1); }

template <typename K, typename... A>
int launch(const char* name, K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  const unsigned threads = block.x * block.y * block.z;   // (the row-band kernels launch (groups, columns, rows) blocks)
  if (lds > (size_t)kLdsMax || threads < 1 || threads > 1024 || grid.x < 1 || grid.y < 1 || grid.z < 1 ||
      grid.y > 65535 || grid.z > 65535)
    return fail(NFP_E_UNSUPPORTED, "%s: launch shape grid (%u,%u,%u) block %u lds %zu outside the device limits", name,
                grid.x, grid.y, grid.z, threads, lds);
  if (t_dry) {
    const size_t n = strlen(t_plan);
    snprintf(t_plan + n, sizeof(t_plan) - n, "%s%s grid=(%u,%u,%u) block=%u lds=%zu%s", n ? "; " : "", name, grid.x, grid.y,
             grid.z, threads, lds, t_stage);
    return NFP_OK;
  }
  if (int rc = set_lds(kernel, lds)) return rc;
  // telemetry (nfp_time_next_launch): bracket this one kernel with the caller's events — recorded by the command
  // processor at the kernel's own start and end, like a profiler's kernel trace
  hipEvent_t ev0 = name[0] != '#' ? (hipEvent_t)g_time_start.exchange(nullptr) : nullptr;
  if (ev0 != nullptr) {
    hipEvent_t ev1 = (hipEvent_t)g_time_stop.exchange(nullptr);
    hipExtLaunchKernelGGL(kernel, grid, block, lds, st, ev0, ev1, 0, args...);
  } else {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  }
  if (name[0] != '#') g_launches++;  // ('#': one-time setup kernels, not part of a forward / backward)
  return hip_ok(hipGetLastError(), name);
}

// launch() of fwd_band / bwd_fast on a dense NCHW map: the record names the staging form
template <typename K, typename... A>
int launch_staged(bool rows, const char* name, K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  t_stage = rows ? " stage=rows" : " stage=blocks";
  const int rc = launch(name, kernel, grid, block, lds, st, args...);
  t_stage = "";
  return rc;
}

// The hot-path kernels (nfp_band.h / nfp_fast.h / nfp_mfma.h / nfp_tile.h) are instantiated for the product form (Cosine) and
// the squared-difference form (L2); DotProduct, GFC and RMSE ride on them through KP's run-time constants (nfp_common.h).
inline bool hot_product(const KP& g) { return g.measure == NFP_COSINE || g.measure == NFP_DOT || g.measure == NFP_GFC; }
inline bool hot_measure(const KP& g) {
  return hot_product(g) || (g.measure == NFP_NORM && g.p == 2.f) || g.measure == NFP_RMSE;
}
// Norm p = 1 (the class default, nfp.py:16) — and EMD (nfp.py:207-216), the same sum, which make_kp turns into it:
// instantiations of their own of the table kernels, the radius-(1, 2) form and the row-band kernels (sums of |a - b|; a
// gradient in sign(a - b)); plain maps only — no fused pooling tail.
inline bool hot_l1(const KP& g) { return g.measure == NFP_NORM && g.p == 1.f; }
// Geman-McClure, Canberra, Hellinger, Jeffrey, squared chord, chi-squared 1 (nfp.py:181-193, 218-227, 229-241, 295-308, 310-324,
// 243-252): sums of a symmetric per-channel term, no per-pixel statistic — one shared instantiation of the row-band and of
// the table kernels (nfp_measures.h::kSymTerm); plain maps only.  (Chi-squared 2 is not symmetric in the pair.)
inline bool hot_sym(const KP& g) {
  return g.measure == NFP_GEMAN || g.measure == NFP_CANBERRA || g.measure == NFP_SQUAREDCHORD || g.measure == NFP_CHISQUARED1 ||
         g.measure == NFP_HELLINGER || g.measure == NFP_JEFFREY;
}
inline const char* hot_name(const KP& g) {
  if (hot_l1(g)) return "l1";
  if (hot_sym(g))
    return g.measure == NFP_GEMAN ? "geman" : (g.measure == NFP_CANBERRA ? "canberra" : (g.measure == NFP_SQUAREDCHORD ? "sqchord" : (g.measure == NFP_HELLINGER ? "hellinger" : (g.measure == NFP_JEFFREY ? "jeffrey" : "chisq1"))));
  return g.measure == NFP_COSINE ? "cos" : (g.measure == NFP_DOT ? "dot" : (g.measure == NFP_GFC ? "gfc" : (g.measure == NFP_RMSE ? "rmse" : "l2")));
}
// nfp_desc.map_f32 (the torch.autocast call): bf16 x / grad_x with float32 out / grad_out.  make_kp writes it as the pair
// (dtype, odtype) — the only descriptors whose maps' type differs from the storage type on the way into the hot-path
// launchers (Attention's float32 dots never reach them with bf16 storage).
inline bool mixed_maps(const KP& g) { return g.dtype == NFP_BF16 && g.odtype == NFP_F32; }
inline bool force_generic() { return g_sw.force_generic.load(std::memory_order_relaxed) != 0; }
// the matrix-core kernels (nfp_mfma.h::fwd_gram, nfp_fast.h::bwd_gemm_phase): NFP_MFMA=0 turns them off
inline bool mfma_enabled() { return g_sw.mfma.load(std::memory_order_relaxed) != 0; }

// A "same" map: stride 1, dilation 1, pad = R, no circular padding, k = 3 or 5 — what every hot-path kernel is built for
inline bool same_geometry(const KP& g) {
  return g.stride == 1 && g.dil == 1 && g.pad == g.R && g.mode != NFP_PAD_CIRCULAR && (g.R == 1 || g.R == 2);
}
// Geometry of the table kernels: "same" maps small enough for one workgroup per image.
// These are the descriptors that have workspace tables (nfp_tables.h).
inline bool fast_geometry(const KP& g) { return same_geometry(g) && g.P <= kBwdThreads && g.P >= 4; }

// Which calls the hot-path kernels serve; everything else runs on the generic kernels.
// sym: also the five measures of nfp_measures.h::kSymTerm (plain single-radius maps only: their callers pass it)
inline bool fast_ok(const KP& g, const void* x, const void* gx, bool sym = false) {
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

// Radius 3 (k = 7) on the row-band kernels.  Both directions must serve what either serves, and the backward is the
// narrower: bwd_tile<3,...> runs workgroups of at most kTileBwdCapR3 = 512 threads (its registers: nfp_tile.h), one per padded
// position of a band of at least R + 1 = 4 rows and its 2R halo rows — (W + 6) * 10 <= 512, W <= 45 — and the bands, each at
// most rb = 512 / (W + 6) - 6 rows and at least 4, must add up to H (any H >= 4 once rb >= 7; multiples of 4 below).
// No W >= 2R + 2 rule here (it never guarded anything in these kernels), so 7 x 7 — W = 2R + 1 — is served.
inline bool tile_r3_geometry(const KP& g) {
  if (g.R != 3 || g.rs != 3 || g.stride != 1 || g.dil != 1 || g.pad != 3 || g.mode == NFP_PAD_CIRCULAR) return false;
  if (g.W < 4 || g.H < 4) return false;   // (reflect padding of 3 needs 4 rows and columns: make_kp; the others keep the same floor)
  const int rb = nfp::kTileBwdCapR3 / (g.W + 6) - 6;
  return rb >= 4 && (rb >= 7 || (g.H + rb - 1) / rb <= g.H / 4);
}
// ... and whether the routing wants them there.  Unset (the default): batches of at least 12 544 pixels — [256,C,7,7],
// [64,C,14,14], [16,C,28,28] — where they measured 1.57x to 12.4x faster than fwd_pairs + bwd_gather; below, at 7 x 7 with 512 channels, they
// lose (a workgroup walks all its channels in series behind a phase A that reads 2 x 48 maps: [64,512,7,7] 86.4 vs 72.9 us,
// [128,512,7,7] 107.7 vs 96.9, [192,512,7,7] 171.1 vs 168.9 — profiles/r13_a_r3_row_band_ab.txt) and larger
// maps are not measured there: such batches keep the kernels they had.
constexpr long long kTileR3MinPixels = 12544;
inline bool tile_r3_wanted(const KP& g) {
  const int sw = g_sw.tile_r3.load(std::memory_order_relaxed);
  return sw < 0 ? (long long)g.B * g.P >= kTileR3MinPixels : sw != 0;
}

// ... and the row-band kernels (nfp_tile.h): "same" maps of any size, no tables
inline bool tile_geometry(const KP& g) {
  if (g.R == 3) return tile_r3_geometry(g) && tile_r3_wanted(g);
  if (!same_geometry(g) || g.rs == 12) return false;
  // one thread per padded position: the smallest band (R + 1 rows and its halo) must fit a workgroup
  if (g.W < 2 * g.R + 2 || g.H < g.R + 1) return false;
  return (g.W + 2 * g.R) * (3 * g.R + 1) <= 1024;
}
inline bool tile_ok(const KP& g, const void* x, const void* gx) {
  if (force_generic() || !tile_geometry(g) || (g.C & 3)) return false;
  if (!hot_measure(g) && !hot_l1(g) && !hot_sym(g)) return false;
  if (g.R == 3 && (!hot_measure(g) || mixed_maps(g))) return false;   // (k = 7: no Norm p = 1, symmetric-term or map_f32 form)
  const bool nhwc = g.sC == 1 && g.sW == g.C && g.sH == (long long)g.W * g.C;
  if (!g.contig && !nhwc) return false;
  const int es = g.dtype == NFP_F32 ? 4 : 2;
  // 32-bit buffer offsets inside an image, and room for the "reads zero" offset (nfp_tile.h::Oob)
  if ((long long)std::max(g.C, g.N) * g.P * es >= 0x7ffffff0LL) return false;
  if (mixed_maps(g) && (long long)g.N * g.P * 4 >= 0x7ffffff0LL) return false;   // (float32 maps beside bf16 x)
  if (!g.contig) {
    const uintptr_t m = g.dtype == NFP_F32 ? 15 : 7;
    if (((uintptr_t)x & m) || ((uintptr_t)gx & m) || ((g.sB * es) & m) || ((g.gB * es) & m)) return false;
  }
  return true;
}
inline int round4(int v) { return (v + 3) & ~3; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline const char* pool_tag(int pool) { return pool == nfp::kPoolBoth ? ",pool" : (pool == nfp::kPoolGap ? ",gap" : ""); }
// fewest groups (<= gmax) that still finish ncq channel quads in ceil(ncq/gmax) rounds
inline int even_groups(int ncq, int gmax) {
  int rounds = (ncq + gmax - 1) / gmax;
  return (ncq + rounds - 1) / rounds;
}

// ---- descriptor fields -> kernel template arguments -------------------------------------------------------------------------
// Each helper calls a generic callable with the field as a std::integral_constant / std::bool_constant, so a launcher
// template is named once per call site: with_radius(g, [&](auto r) { return f<decltype(r)::value>(...); }).  A helper
// enumerates only its own field; which COMBINATIONS have a kernel is the caller's `if constexpr`, returning kNotApplicable:
//   - kNormP1 / kSymTerm: plain maps only (no pooling tail), and kSymTerm not with radius 12;
//   - radius 12: the table kernels fwd_band / bwd_fast alone (no fwd_gram, no bwd_gemm, no row-band kernel);
//   - MF (float32 maps beside bf16 x): kHasMixed below.
template <int V>
using Int = std::integral_constant<int, V>;

// the radius: 1 or 2; R12 (the caller serves both radii from one pass): 12 when g.rs == 12
template <bool R12 = false, typename F>
int with_radius(const KP& g, F&& f) {
  if constexpr (R12)
    if (g.rs == 12) return f(Int<12>{});
  return g.R == 1 ? f(Int<1>{}) : f(Int<2>{});
}

// the hot-path family: the product form or the squared-difference form (hot_measure); ALL: also the instantiations of
// Norm p = 1 and of the symmetric-term measures
template <bool ALL = false, typename F>
int with_hot(const KP& g, F&& f) {
  if constexpr (ALL) {
    if (hot_l1(g)) return f(Int<kNormP1>{});
    if (hot_sym(g)) return f(Int<kSymTerm>{});
  }
  return hot_product(g) ? f(Int<NFP_COSINE>{}) : f(Int<NFP_NORM>{});
}

// The fused tail of a launch as one value; default-constructed: plain maps, no tail.  mode: kPoolNone, kPoolBoth (nfp_pool_*:
// both pooled sums) or kPoolGap (nfp_gap_*: GAP(x) beside the maps).  The launchers unpack it at their launch(...) call.
struct FwdTail {
  int mode = nfp::kPoolNone;
  float* gap = nullptr;    // [B,C] channel means, or null
  float* nfpm = nullptr;   // [B,N] map means (kPoolBoth), or null
  float* part = nullptr;   // scratch for the bands' partial sums: rows of C + N floats (kPoolGap: C), or null (one band)
  int* nb = nullptr;       // out: rows of `part` per image
};
struct BwdTail {
  int mode = nfp::kPoolNone;
  const float* ggap = nullptr;    // grad of gap [B,C], or null
  const float* gnfpm = nullptr;   // grad of nfpm [B,N] (kPoolBoth), or null
};
// ... and its template argument
template <typename F>
int with_pool(int pool, F&& f) {
  if (pool == nfp::kPoolGap) return f(Int<nfp::kPoolGap>{});
  return pool ? f(Int<nfp::kPoolBoth>{}) : f(Int<nfp::kPoolNone>{});
}

// every measure with a Meas<> of its own, Norm by its order; Attention and SharpenedCosine (the caller's): kNotApplicable.
// EMD is a case here for the bias path, whose g.measure is the descriptor's own (nfp_hip.hip::bias_kp); make_kp has
// turned it into Norm p = 1 on the difference weights for nfp_forward / nfp_backward, which never arrive with it.
template <typename F>
int with_measure(const KP& g, F&& f) {
  switch (g.measure) {
    case NFP_NORM:
      if (g.p == 1.f) return f(Int<kNormP1>{});
      if (g.p == 2.f) return f(Int<kNormP2>{});
      return f(Int<NFP_NORM>{});
    case NFP_COSINE: return f(Int<NFP_COSINE>{});
    case NFP_DOT: return f(Int<NFP_DOT>{});
    case NFP_RMSE: return f(Int<NFP_RMSE>{});
    case NFP_GEMAN: return f(Int<NFP_GEMAN>{});
    case NFP_EMD: return f(Int<NFP_EMD>{});
    case NFP_CANBERRA: return f(Int<NFP_CANBERRA>{});
    case NFP_HELLINGER: return f(Int<NFP_HELLINGER>{});
    case NFP_CHISQUARED1: return f(Int<NFP_CHISQUARED1>{});
    case NFP_CHISQUARED2: return f(Int<NFP_CHISQUARED2>{});
    case NFP_GFC: return f(Int<NFP_GFC>{});
    case NFP_PEARSON: return f(Int<NFP_PEARSON>{});
    case NFP_JEFFREY: return f(Int<NFP_JEFFREY>{});
    case NFP_SQUAREDCHORD: return f(Int<NFP_SQUAREDCHORD>{});
    case NFP_SMITH: return f(Int<NFP_SMITH>{});
    default: return kNotApplicable;
  }
}

// storage: f(BF, NHWC) from g.dtype and the layout (dense NCHW, or channels-last: the launchers' callers have checked)
template <typename F>
int with_storage(const KP& g, F&& f) {
  constexpr std::true_type yes;
  constexpr std::false_type no;
  if (g.dtype == NFP_BF16) return g.contig ? f(yes, no) : f(yes, yes);
  return g.contig ? f(no, no) : f(no, yes);
}
// MF kernels exist only for plain maps (no pooling), one radius (1 or 2) and the COSINE / NORM instantiations (with their dot / gfc /
// rmse riders); Norm p = 1 and the symmetric-term measures with float32 maps are the any-geometry kernels'
template <int R, int M, int POOL>
constexpr bool kHasMixed = POOL == nfp::kPoolNone && R != 12 && R != 3 && (M == NFP_COSINE || M == NFP_NORM);
// ... and the launchers that serve mixed_maps descriptors: f(BF, NHWC, MF)
template <int R, int M, int POOL, typename F>
int with_storage_mixed(const KP& g, F&& f) {
  if (!mixed_maps(g)) return with_storage(g, [&](auto bf, auto nhwc) { return f(bf, nhwc, std::false_type{}); });
  constexpr std::true_type yes;
  if constexpr (kHasMixed<R, M, POOL>)
    return g.contig ? f(yes, std::false_type{}, yes) : f(yes, yes, yes);
  else
    return kNotApplicable;
}

// ---- the any-geometry kernels of nfp_gather.h / nfp_direct.h (nfp_generic.hip) -------------------------------------------
// fwd_pairs, else fwd_direct; bwd_gather, bwd_gather_banded, else bwd_direct — by with_measure: NFP_OK, an NFP_E_* code, or
// kNotApplicable for the measures with_measure leaves to the caller.  Attention arrives as its DotProduct block
// (nfp_hip.hip::as_dot); its softmax over the neighbours is the two launches below.
int generic_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st);
int generic_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st);
int attn_softmax_forward(const KP& g, const float* dots, void* out, hipStream_t st);
int attn_softmax_backward(const KP& g, const void* go, const void* out, float* gd, hipStream_t st);

// ---- the table kernels of nfp_mfma.h / nfp_band.h (nfp_table_fwd.hip) and nfp_fast.h (nfp_table_bwd.hip) ------------------
// Each returns NFP_OK, kNotApplicable or an NFP_E_* code; g_variant names the launch.  The caller has asked fast_ok; the
// radius (12: g.rs), the family (with_hot<true>) and the tail (t.mode) select the instantiation.  Those that exist:
// plain maps for every family, but not kSymTerm with radius 12; the pooled and gap tails for the cosine and L2 families
// alone, and kPoolBoth not with radius 12.  fwd_gram and the matrix-core backward: cosine / L2, one radius (its tail is
// a run-time option of fwd_gram: gap, nfpm or both null).
template <int R, int M, int POOL>
constexpr bool kHasTable = POOL == nfp::kPoolNone ? !(R == 12 && M == kSymTerm)
                                                  : (M == NFP_COSINE || M == NFP_NORM) && !(R == 12 && POOL == nfp::kPoolBoth);
int table_fwd_gram(const KP& g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t = {});
int table_fwd_band(const KP& g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t = {});
// (the matrix-core form first where it exists and applies, else the vector form)
int table_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st,
                   const BwdTail& t = {});

// ---- the row-band kernels of nfp_tile.h (nfp_tile_fwd.hip, nfp_tile_bwd.hip; shared sizing: nfp_tile_launch.h) ------------
// Each returns NFP_OK, kNotApplicable (this descriptor is not theirs / does not fit) or an NFP_E_* code; g_variant names
// the launch.  The tail: FwdTail / BwdTail above (a pooled forward always writes its sums to t.part, *t.nb rows per image).
int tile_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t = {});
int tile_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st,
                  const BwdTail& t = {});
int tile_pool_fold(const KP& g, const float* part, float* gap, float* nfpm, int nb, hipStream_t st);
// ... and their radius-3 instantiations, units of their own (tile_forward / tile_backward hand g.R == 3 on)
int tile_forward_r3(const KP& g, const void* x, void* out, float* saved, hipStream_t st, const FwdTail& t);
int tile_backward_r3(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st,
                     const BwdTail& t);

// ---- NFPPooling(bias=True) (nfp_bias.hip, ABI 7) -------------------------------------------------------------------------
// g.measure is the descriptor's own measure (Attention: its DotProduct form), g.diff = 0 and dw = the difference weights.
// bias_forward stores the maps in `out` (g.odtype) and the per-pair stats in `saved`, or — dots != null — the raw sums in
// `dots` alone.  bias_backward needs bias_coef_floats(g) * B*N*O + B*C*(N + 1) floats of `scratch`.
int bias_coef_floats(const KP& g);
int bias_forward(const KP& g, int dw, const void* x, const float* bc, const float* beta, void* out, float* saved,
                 float* dots, hipStream_t st);
int bias_backward(const KP& g, int dw, const void* x, const float* bc, const float* beta, const void* go, const void* out,
                  const float* saved, void* gx, float* gbc, float* gbeta, float* scratch, hipStream_t st);

// ---- valid maps: stride 1, dilation 1, padding 0 (nfp_valid.hip; include/nfp.h: nfp_valid_*) --------------------------------
// valid_refusal: why the descriptor lies outside the kernels' set (measure, geometry, layout), or null.  The two launchers
// return NFP_OK or an NFP_E_* code (NFP_E_UNSUPPORTED also for channels-last images off 16-byte boundaries); g_variant
// names the launch.
const char* valid_refusal(const KP& g);
int valid_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st);
int valid_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st);
// ... and their L1 family (include/nfp.h: nfp_valid_abs_*): Norm p = 1 on the difference weights (EMD arrives as it: make_kp)
// under the same geometry and layout rules; neither `out` nor a saved statistic on the way back.
const char* valid_abs_refusal(const KP& g);
int valid_abs_forward(const KP& g, const void* x, void* out, hipStream_t st);
int valid_abs_backward(const KP& g, const void* x, const void* go, void* gx, hipStream_t st);

// ---- strided maps: stride 2 to 4, dilation 1, padding 0 or R (nfp_strided.hip; include/nfp.h: nfp_strided_*) ---------------
// As the valid-map trio: strided_refusal names what lies outside the kernels' set, or null; the launchers return NFP_OK or
// an NFP_E_* code (NFP_E_UNSUPPORTED also for a band that does not fit a workgroup); g_variant names the launch.
const char* strided_refusal(const KP& g);
int strided_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st);
int strided_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st);

}  // namespace nfp_host
