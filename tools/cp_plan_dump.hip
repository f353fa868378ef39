// cp_plan_dump.hip — what the twelve launching entries of the compress-BN family (nfp_cpool_*, nfp_cpool_wide_*, nfp_cproj_*
// and their _fmt forms, nfp_cpsync_*) would launch over a sweep of sizes and options, and what they refuse: no GPU needed.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I neighbour_feature_pooling_amd/csrc tools/cp_plan_dump.hip \
//         -L neighbour_feature_pooling_amd -lnfp_hip -Wl,-rpath,$PWD/neighbour_feature_pooling_amd -o cp_plan_dump
//   ./cp_plan_dump > plan.txt          (one line per call; the last line counts them)
//
// launch() in plan mode (nfp_launch.h: t_dry) records each launch's name, grid, block and LDS bytes in t_plan instead of
// making it, and every pointer handed in is kStandIn, which is never dereferenced.  Those three names are all the tool takes
// from the library's headers beside the C ABI of include/nfp.h, so the same source builds against any tree that has these
// entries: two trees whose host paths decide alike print the same bytes (`cmp`).  A line is
//   entry sizes options -> return code | nfp_last_variant() | t_plan | nfp_last_error()
// with the variant shown for a served call and the error for a refused one.
//
// The sweep crosses every branch of the size functions: B in {0, 1, 4, 64, 256}; N in {1, 8, 9, 24, 32} and {33, 48, 96} for
// the wide entries; P in {1, 49, 196, 784, 3025, 12100} (both sides of the chunk budget at 8 and 32 maps and of the wide
// chunk); D in {1, 24, 33, 128, 129, 512, 2048} (the 32-, 64- and 128-channel tiles, 512 / tiles, odd and even D for the
// bf16 channels-last pairs); float32 and bf16, train and eval, the projection with and without the ReLU in both layouts,
// a backward with all / maps only / parameters only / no gradients wanted, the staged entries for 1 and 3 ranks (B = 0: an
// empty rank).  Then one refusal of each kind per entry.
#include <cmath>
#include <cstdio>

#include "nfp_launch.h"

namespace {

enum Entry { kPoolF, kPoolB, kWideF, kWideB, kProjF, kProjB, kProjFmtF, kProjFmtB, kSyncMoments, kSyncF, kSyncReduce, kSyncMaps };
const char* const kNames[] = {"nfp_cpool_forward", "nfp_cpool_backward", "nfp_cpool_wide_forward", "nfp_cpool_wide_backward",
                              "nfp_cproj_forward", "nfp_cproj_backward", "nfp_cproj_forward_fmt", "nfp_cproj_backward_fmt",
                              "nfp_cpsync_moments", "nfp_cpsync_forward", "nfp_cpsync_reduce", "nfp_cpsync_maps"};

struct Call {
  int B = 4, N = 8;
  long long P = 49;
  int D = 32, dtype = NFP_F32, training = 1, relu = 1, layout = NFP_ACT_NCHW;
  int want = 15;   // bit 0: grad_maps, 1: grad_w, 2: grad_gamma, 3: grad_beta
  int kind = NFP_CP_POOL, world = 1;
  long long global_count = 0;
  double eps = 1e-5, momentum = 0.1;
  // what a refusal case takes away
  bool null_w = false, null_rv = false, odd_rows = false;
  int short_saved = 0, short_scratch = 0, short_rows = 0;
};

long long g_calls = 0;

int call(Entry e, const Call& c) {
  void* const X = nfp_host::kStandIn;
  float* const F = (float*)X;
  const float* w = c.null_w ? nullptr : F;
  float* rv = c.null_rv ? nullptr : F;
  const bool sync = e >= kSyncMoments, proj = e >= kProjF && e <= kProjFmtB, wide = e == kWideF || e == kWideB;
  const bool backward = e == kPoolB || e == kWideB || e == kProjB || e == kProjFmtB || e == kSyncReduce;
  const int64_t saved = (sync ? nfp_cpsync_saved_floats(c.N, c.D) : nfp_cpool_saved_floats(c.N, c.D)) - c.short_saved;
  int64_t scratch;
  if (e == kSyncMoments)
    scratch = nfp_cpool_scratch_floats(c.B, c.N, c.P, 1, 0);
  else if (proj || (sync && c.kind == NFP_CP_PROJ))
    scratch = nfp_cproj_scratch_floats(c.B, c.N, c.P, c.D, backward);
  else
    scratch = wide ? nfp_cpool_wide_scratch_floats(c.B, c.N, c.P, c.D, backward) : nfp_cpool_scratch_floats(c.B, c.N, c.P, c.D, backward);
  scratch -= c.short_scratch;
  void* gm = c.want & 1 ? X : nullptr;
  float *gw = c.want & 2 ? F : nullptr, *gg = c.want & 4 ? F : nullptr, *gb = c.want & 8 ? F : nullptr;
  void* rows = c.odd_rows ? (void*)((char*)X + 4) : X;     // (records are doubles: 4 bytes off is misaligned)
  const int64_t records = (int64_t)c.world * nfp_cpsync_record_doubles(c.N) - c.short_rows;
  const int64_t kq = nfp_cpsync_kq_floats(c.N);
  switch (e) {
    case kPoolF:
      return nfp_cpool_forward(c.B, c.N, c.P, c.D, c.dtype, c.training, X, w, F, F, F, rv, c.momentum, c.eps, F, F, saved, F, scratch,
                               nullptr);
    case kWideF:
      return nfp_cpool_wide_forward(c.B, c.N, c.P, c.D, c.dtype, c.training, X, w, F, F, F, rv, c.momentum, c.eps, F, F, saved, F,
                                    scratch, nullptr);
    case kPoolB:
      return nfp_cpool_backward(c.B, c.N, c.P, c.D, c.dtype, c.training, X, w, F, F, F, rv, c.eps, F, saved, F, gm, gw, gg, gb, F,
                                scratch, nullptr);
    case kWideB:
      return nfp_cpool_wide_backward(c.B, c.N, c.P, c.D, c.dtype, c.training, X, w, F, F, F, rv, c.eps, F, saved, F, gm, gw, gg, gb, F,
                                     scratch, nullptr);
    case kProjF:
      return nfp_cproj_forward(c.B, c.N, c.P, c.D, c.dtype, c.training, c.relu, X, w, F, F, F, rv, c.momentum, c.eps, X, F, saved, F,
                               scratch, nullptr);
    case kProjFmtF:
      return nfp_cproj_forward_fmt(c.B, c.N, c.P, c.D, c.dtype, c.training, c.relu, X, w, F, F, F, rv, c.momentum, c.eps, X, F, saved,
                                   F, scratch, nullptr, c.layout);
    case kProjB:
      return nfp_cproj_backward(c.B, c.N, c.P, c.D, c.dtype, c.training, c.relu, X, w, F, F, F, rv, c.eps, F, saved, X, gm, gw, gg, gb,
                                F, scratch, nullptr);
    case kProjFmtB:
      return nfp_cproj_backward_fmt(c.B, c.N, c.P, c.D, c.dtype, c.training, c.relu, X, w, F, F, F, rv, c.eps, F, saved, X, gm, gw, gg,
                                    gb, F, scratch, nullptr, c.layout);
    case kSyncMoments:
      return nfp_cpsync_moments(c.B, c.N, c.P, c.dtype, X, (double*)rows, nfp_cpsync_record_doubles(c.N) - c.short_rows, F, scratch,
                                nullptr);
    case kSyncF:
      return nfp_cpsync_forward(c.kind, c.B, c.N, c.P, c.D, c.dtype, c.relu, X, w, F, F, F, rv, c.momentum, c.eps,
                                (const double*)rows, c.world, records, c.global_count, X, F, saved, nullptr, c.layout);
    case kSyncReduce:
      return nfp_cpsync_reduce(c.kind, c.B, c.N, c.P, c.D, c.dtype, c.relu, X, w, F, F, c.eps, F, saved, X, gw, gg, gb, (float*)rows,
                               kq - c.short_rows, F, scratch, nullptr, c.layout);
    default:
      return nfp_cpsync_maps(c.kind, c.B, c.N, c.P, c.D, c.dtype, c.relu, X, w, F, F, c.eps, F, saved, X, (const float*)rows, c.world,
                             (int64_t)c.world * kq - c.short_rows, gm, nullptr, c.layout);
  }
}

void run(Entry e, const Call& c, const char* label = "") {
  nfp_host::t_plan[0] = 0;
  const int rc = call(e, c);
  printf("%s B=%d N=%d P=%lld D=%d dtype=%d training=%d relu=%d layout=%d want=%d kind=%d world=%d %s-> %d | %s | %s | %s\n",
         kNames[e], c.B, c.N, c.P, c.D, c.dtype, c.training, c.relu, c.layout, c.want, c.kind, c.world, label, rc,
         rc == NFP_OK ? nfp_last_variant() : "", nfp_host::t_plan, rc == NFP_OK ? "" : nfp_last_error());
  ++g_calls;
}

// every option of every entry at one size
void sweep(Call c) {
  const int wants[] = {15, 1, 14, 0};
  for (int dtype : {NFP_F32, NFP_BF16}) {
    c.dtype = dtype;
    for (int training : {1, 0}) {
      c.training = training;
      for (Entry f : {kPoolF, kWideF}) {
        if (f == kPoolF && c.N > 32) continue;
        run(f, c);
        for (int want : wants) {
          c.want = want;
          run(f == kPoolF ? kPoolB : kWideB, c);
        }
      }
      if (c.N > 32) continue;
      for (int relu : {1, 0}) {
        c.relu = relu;
        for (int layout : {NFP_ACT_NCHW, NFP_ACT_NHWC}) {
          c.layout = layout;
          for (Entry f : {kProjF, kProjFmtF}) {
            if (f == kProjF && layout != NFP_ACT_NCHW) continue;
            run(f, c);
            for (int want : wants) {
              c.want = want;
              run(f == kProjF ? kProjB : kProjFmtB, c);
            }
          }
        }
      }
      c.relu = 1, c.layout = NFP_ACT_NCHW;
    }
    if (c.N > 32) continue;
    c.training = 1;
    run(kSyncMoments, c);
    for (int kind : {NFP_CP_POOL, NFP_CP_PROJ}) {
      c.kind = kind;
      for (int relu : {1, 0}) {
        c.relu = relu;
        for (int layout : {NFP_ACT_NCHW, NFP_ACT_NHWC}) {
          c.layout = layout;
          for (int world : {1, 3}) {
            c.world = world;
            c.want = 15;
            run(kSyncF, c);
            run(kSyncMaps, c);
          }
          c.world = 1;
          for (int want : wants) {
            c.want = want;
            run(kSyncReduce, c);
          }
        }
      }
    }
    c.kind = NFP_CP_POOL, c.relu = 1, c.layout = NFP_ACT_NCHW, c.want = 15;
  }
}

// one refusal of each kind per entry, at a size every entry otherwise serves
void refusals() {
  for (int i = kPoolF; i <= kSyncMaps; ++i) {
    const Entry e = (Entry)i;
    const bool sync = e >= kSyncMoments, wide = e == kWideF || e == kWideB, proj = e >= kProjF && e <= kProjFmtB;
    const bool forward = e == kPoolF || e == kWideF || e == kProjF || e == kProjFmtF || e == kSyncF;
    Call base;
    if (sync) base.kind = NFP_CP_PROJ;
    auto refuse = [&](const char* label, auto&& change) {
      Call c = base;
      change(c);
      run(e, c, label);
    };
    refuse("[N = 0] ", [](Call& c) { c.N = 0; });
    refuse("[P = 0] ", [](Call& c) { c.P = 0; });
    refuse("[D = 0] ", [](Call& c) { c.D = 0; });
    refuse("[B = -1] ", [](Call& c) { c.B = -1; });
    refuse("[dtype = 2] ", [](Call& c) { c.dtype = 2; });
    refuse("[too many maps] ", [&](Call& c) { c.N = wide ? 97 : 33; });
    refuse("[N * P = 2^31] ", [](Call& c) { c.B = 1, c.N = 32, c.P = 1LL << 26; });
    refuse("[D > 2^22] ", [](Call& c) { c.D = (1 << 22) + 1; });
    refuse("[2^31 workgroups] ", [](Call& c) { c.B = 1 << 30, c.N = 1, c.P = 128; });
    refuse("[one value per channel] ", [](Call& c) { c.B = 1, c.P = 1; });
    refuse("[D * P = 2^31] ", [](Call& c) { c.B = 1, c.N = 1, c.P = 1LL << 20, c.D = 1 << 11; });
    refuse("[2^31 workgroups of D tiles] ", [](Call& c) { c.B = 1 << 20, c.N = 1, c.P = 64, c.D = 1 << 17; });
    refuse("[NULL w] ", [](Call& c) { c.null_w = true; });
    refuse("[one running statistic] ", [](Call& c) { c.null_rv = true; });
    refuse("[eval, one running statistic] ", [](Call& c) { c.training = 0, c.null_rv = true; });
    refuse("[eps < 0] ", [](Call& c) { c.eps = -1.0; });
    refuse("[momentum NaN] ", [](Call& c) { c.momentum = NAN; });
    refuse("[short saved] ", [](Call& c) { c.short_saved = 1; });
    refuse("[short scratch] ", [](Call& c) { c.short_scratch = 1; });
    refuse("[short scratch, 196 pixels] ", [](Call& c) { c.P = 196, c.short_scratch = 1; });
    if (proj || sync) refuse("[layout = 2] ", [](Call& c) { c.layout = 2; });
    if (!sync) continue;
    refuse("[kind = 2] ", [](Call& c) { c.kind = 2; });
    refuse("[world = 0] ", [](Call& c) { c.world = 0; });
    refuse("[short rows] ", [](Call& c) { c.world = 3, c.short_rows = 1; });
    refuse("[misaligned rows] ", [](Call& c) { c.odd_rows = true; });
    refuse("[NULL grad_maps] ", [](Call& c) { c.want = 0; });
    if (forward) {
      refuse("[global_count = -1] ", [](Call& c) { c.global_count = -1; });
      refuse("[global_count = 1] ", [](Call& c) { c.global_count = 1; });
      refuse("[global_count below the rank's] ", [](Call& c) { c.global_count = 100; });
    }
  }
}

}  // namespace

int main() {
  nfp_host::t_dry = true;
  for (int B : {0, 1, 4, 64, 256})
    for (int N : {1, 8, 9, 24, 32, 33, 48, 96})
      for (long long P : {1LL, 49LL, 196LL, 784LL, 3025LL, 12100LL})
        for (int D : {1, 24, 33, 128, 129, 512, 2048}) {
          Call c;
          c.B = B, c.N = N, c.P = P, c.D = D;
          sweep(c);
        }
  refusals();
  printf("%lld calls\n", g_calls);
  return 0;
}
