// nfp_attpool.hip — the tail of models/nfp_heads.py::SimilarityAwarePooling (nfp_heads.py:224-232): the NFP maps m [B,N,P]
// of a layer, a trainable 1x1 conv att_proj (w [N], b [1]), a softmax over the P pixels and the attention-weighted sum
//   l_p = b + sum_n w_n m_np      a = softmax_p(l)      pooled_n = sum_p a_p m_np
// which the reference runs as six ATen ops (conv, flatten, softmax, view, mul, sum) and twice that backward.  Here: one
// kernel each way and a tiny batch reduce for the gradients of att_proj.  Backward, given g [N]:
//   t_p = sum_n g_n m_np    s = sum_p a_p t_p    dl_p = a_p (t_p - s)
//   grad_m_np = a_p g_n + dl_p w_n      gw_n = sum_b sum_p dl_p m_np      gb = sum_b sum_p dl_p
// (gb is zero in exact arithmetic — softmax is shift-invariant — and comes out as the rounding noise of that sum.)
//
// One workgroup per image.  The image's maps are walked in chunks of CH pixels, every chunk staged in LDS as float32
// (one chunk — the whole image — where (N + 1) * P floats fit the budget below, which is every head-sized map):
//   lanes along p   thread p loads m[0..N) of its pixel (neighbouring lanes, neighbouring addresses; N independent loads in
//                   flight), keeps them in LDS and forms l_p (backward: t_p)
//   workgroup       max and sums through wave butterflies / the DPP sums of nfp_common.h, then LDS
//   rows            one wavefront per map row n: sum_p e_p m_np from LDS, lanes along p
// The forward takes the max of the logits in a first pass and the exps and sums in a second; the backward s in a first pass
// and everything else in a second.  An image of one chunk stays in LDS between the passes; with several chunks the second
// pass reads the maps again, which the L2 serves.
// Float32 arithmetic whose error does not grow with the logits (tests: l spanning +-80 inside the 1e-5 bar):
//   * exp(l_p - M) turns an ABSOLUTE error of l_p into a relative one of a_p, and a float32 sum of N products near 80 is off
//     by several 1e-6: the second pass forms l_p as a two-float sum (error-free products and sums, att_logit2);
//   * t_p - s cancels where one pixel holds nearly all the attention (s is then t of that pixel, up to rounding — and it is
//     this difference times a_p ~ 1 that the gradients of att_proj are made of).  softmax' is shift-invariant in t, so both
//     are taken about c = t of the pixel of largest attention: t_p - c is exactly 0 there and s - c a sum of small terms.
// Every sum in a fixed order, no atomics: two runs agree bitwise, and image b's results do not depend on the batch around it.
#include "nfp_launch.h"

#include <cmath>

namespace nfp {
namespace {

constexpr int kAttMaxT = 1024;            // threads per workgroup: 256 ... 1024 by the chunk's width (attpool_threads)
constexpr int kAttBudgetFloats = 18432;   // 72 KiB for the chunk's maps and its row of exps: with the row sums and the
                                          // reduction words a workgroup stays under 80 KiB — two per CU out of 160 KiB
constexpr int kAttMaxN = 1024;            // (a chunk is then at least 17 pixels wide)
constexpr int kAttRed = 32;               // reduction words behind the row sums: 16 values, 16 indices

__device__ __forceinline__ float att_ldm(const void* m, long long i, int bf16) {
  return bf16 ? bf16_to_f32(((const uint16_t*)m)[i]) : ((const float*)m)[i];
}

// sum over the 64 lanes, the same value in every lane: the DPP row sums of nfp_common.h, then the two halves
__device__ __forceinline__ float att_wave_sum(float v) {
  v = group_sum(v, 32);   // lane 31: lanes 0..31, lane 63: lanes 32..63
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31)) +
         __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// over the workgroup, the same value in every thread; red: 16 floats nobody else uses between the two barriers
__device__ __forceinline__ float att_block_sum(float v, float* red) {
  v = att_wave_sum(v);
  const int nw = blockDim.x >> 6;
  __syncthreads();   // (the previous reduction's words are read)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
  for (int i = 1; i < nw; ++i) s += red[i];
  return s;
}
// max over the workgroup (fmaxf: a NaN logit does not hide the others — it reaches the result through the sum of exps)
__device__ __forceinline__ float att_block_max(float v, float* red) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  const int nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
  for (int i = 1; i < nw; ++i) s = fmaxf(s, red[i]);
  return s;
}
// (a, p) beats (b, q): the larger value, of equal values the lower index — a total order, so the winner does not depend on
// the order of the comparisons.  A NaN never wins.
__device__ __forceinline__ bool att_beats(float a, int p, float b, int q) { return a > b || (a == b && p < q); }
// index of the largest value over the workgroup, the same in every thread; red: 16 floats and 16 ints
__device__ __forceinline__ int att_block_argmax(float v, int p, float* red) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const float ov = __shfl_xor(v, m, 64);
    const int op = __shfl_xor(p, m, 64);
    if (att_beats(ov, op, v, p)) {
      v = ov;
      p = op;
    }
  }
  int* redp = (int*)(red + 16);
  const int nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = v;
    redp[threadIdx.x >> 6] = p;
  }
  __syncthreads();
  v = red[0];
  p = redp[0];
  for (int i = 1; i < nw; ++i)
    if (att_beats(red[i], redp[i], v, p)) {
      v = red[i];
      p = redp[i];
    }
  return p;
}

// b + sum_n w_n col[n * CH] as the unevaluated sum hi + lo of two floats: every product with its rounding error (one fma),
// every sum with its rounding error (Knuth's two-sum).  Contraction off: an fma formed from p and the sum would break both.
__device__ __forceinline__ void att_logit2(const float* col, int CH, int N, const float* __restrict__ w, float b0, float& hi,
                                           float& lo) {
#pragma clang fp contract(off)
  hi = b0;
  lo = 0.f;
  for (int n = 0; n < N; ++n) {
    const float wn = w[n], v = col[n * CH];
    const float p = wn * v;
    const float pe = __builtin_fmaf(wn, v, -p);
    const float s = hi + p;
    const float bb = s - hi;
    const float se = (hi - (s - bb)) + (p - bb);
    hi = s;
    lo += se + pe;
  }
}

// Dynamic LDS (floats): sm[N * CH] the chunk's maps, row n at n * CH; lg[CH] its exps; acc[N] the row sums; red[kAttRed].
// grid = B, block = 256 ... 1024.
template <int BF16>
__global__ void __launch_bounds__(kAttMaxT) attpool_fwd(int N, int P, int CH, const void* __restrict__ maps,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ pooled, float* att) {
  extern __shared__ __attribute__((aligned(16))) float att_lds[];
  float* sm = att_lds;
  float* lg = sm + (size_t)N * CH;
  float* acc = lg + CH;
  float* red = acc + N;
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = T >> 6;
  const long long base = (long long)blockIdx.x * N * P;
  float* att_b = att != nullptr ? att + (long long)blockIdx.x * P : nullptr;
  const bool several = CH < P;
  const float b0 = bias[0];
  for (int n = tid; n < N; n += T) acc[n] = 0.f;
  // pass 1: the largest logit (one chunk: its maps stay in LDS)
  float lmax = -INFINITY;
  for (long long p0 = 0; p0 < P; p0 += CH) {
    const int ch = (int)min((long long)CH, P - p0);
    for (int pl = tid; pl < ch; pl += T) {
      float l = b0;
#pragma unroll 8
      for (int n = 0; n < N; ++n) {
        const float v = att_ldm(maps, base + (long long)n * P + p0 + pl, BF16);
        if (!several) sm[n * CH + pl] = v;
        l = fmaf(w[n], v, l);
      }
      lmax = fmaxf(lmax, l);
    }
  }
  const float M = att_block_max(lmax, red);
  const float Mu = M == -INFINITY ? 0.f : M;   // (every logit -inf: exp(-inf - 0) = 0 and 0 / 0 below, not exp(NaN))
  // pass 2: the exps, their sum, the rows' weighted sums
  float es = 0.f;
  for (long long p0 = 0; p0 < P; p0 += CH) {
    const int ch = (int)min((long long)CH, P - p0);
    if (several) {
      __syncthreads();   // (the previous chunk's row sums have read sm and lg)
      for (int pl = tid; pl < ch; pl += T) {
#pragma unroll 8
        for (int n = 0; n < N; ++n) sm[n * CH + pl] = att_ldm(maps, base + (long long)n * P + p0 + pl, BF16);
      }
    }
    for (int pl = tid; pl < ch; pl += T) {   // (every thread reads the column it wrote)
      float hi, lo;
      att_logit2(sm + pl, CH, N, w, b0, hi, lo);
      const float e = expf((hi - Mu) + lo);
      lg[pl] = e;
      es += e;
      if (several && att_b != nullptr) att_b[p0 + pl] = e;   // (divided by the sum by this thread, behind the loop)
    }
    __syncthreads();   // (sm and lg are complete)
    for (int n = wv; n < N; n += nw) {
      const float* row = sm + n * CH;
      float s = 0.f;
      for (int pl = lane; pl < ch; pl += 64) s = fmaf(lg[pl], row[pl], s);
      s = att_wave_sum(s);
      if (lane == 0) acc[n] += s;
    }
  }
  const float inv = 1.f / att_block_sum(es, red);   // (its barriers publish acc)
  for (int n = tid; n < N; n += T) pooled[(long long)blockIdx.x * N + n] = acc[n] * inv;
  if (att_b == nullptr) return;
  if (!several) {
    for (int pl = tid; pl < P; pl += T) att_b[pl] = lg[pl] * inv;
  } else {
    for (long long p0 = 0; p0 < P; p0 += CH) {
      const int ch = (int)min((long long)CH, P - p0);
      for (int pl = tid; pl < ch; pl += T) att_b[p0 + pl] *= inv;   // (this thread's own store)
    }
  }
}

// Dynamic LDS as attpool_fwd: sm, lg (dl_p), acc (the gw row sums), red.  part: row b of [B, N + 1] floats — gw's share
// of this image, then gb's — or null (att_proj frozen); gm null: the maps take no gradient.
template <int BF16>
__global__ void __launch_bounds__(kAttMaxT) attpool_bwd(int N, int P, int CH, const void* __restrict__ maps,
                                                        const float* __restrict__ w, const float* __restrict__ att,
                                                        const float* __restrict__ gp, void* __restrict__ gm,
                                                        float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float att_lds[];
  float* sm = att_lds;
  float* lg = sm + (size_t)N * CH;
  float* acc = lg + CH;
  float* red = acc + N;
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = T >> 6;
  const long long base = (long long)blockIdx.x * N * P;
  const float* att_b = att + (long long)blockIdx.x * P;
  const float* g = gp + (long long)blockIdx.x * N;
  const bool several = CH < P;
  for (int n = tid; n < N; n += T) acc[n] = 0.f;
  // the pixel of largest attention and its t: the point about which t and s are taken (file comment)
  float best = -INFINITY;
  int pbest = 0;
  for (int p = tid; p < P; p += T) {
    const float a = att_b[p];
    if (a > best) {
      best = a;
      pbest = p;
    }
  }
  pbest = att_block_argmax(best, pbest, red);
  float c = 0.f;
#pragma unroll 8
  for (int n = 0; n < N; ++n) c = fmaf(g[n], att_ldm(maps, base + (long long)n * P + pbest, BF16), c);   // (as t below: bitwise)
  // pass 1: s - c = sum_p a_p (t_p - c) (one chunk: its maps stay in LDS)
  float st = 0.f;
  for (long long p0 = 0; p0 < P; p0 += CH) {
    const int ch = (int)min((long long)CH, P - p0);
    for (int pl = tid; pl < ch; pl += T) {
      float t = 0.f;
#pragma unroll 8
      for (int n = 0; n < N; ++n) {
        const float v = att_ldm(maps, base + (long long)n * P + p0 + pl, BF16);
        if (!several) sm[n * CH + pl] = v;
        t = fmaf(g[n], v, t);
      }
      st = fmaf(att_b[p0 + pl], t - c, st);
    }
  }
  const float s = att_block_sum(st, red);
  // pass 2: dl_p, the maps' gradient, the sums of gw and gb
  float sb = 0.f;
  for (long long p0 = 0; p0 < P; p0 += CH) {
    const int ch = (int)min((long long)CH, P - p0);
    if (several) {
      __syncthreads();   // (the previous chunk's row sums have read sm and lg)
      for (int pl = tid; pl < ch; pl += T) {
#pragma unroll 8
        for (int n = 0; n < N; ++n) sm[n * CH + pl] = att_ldm(maps, base + (long long)n * P + p0 + pl, BF16);
      }
    }
    for (int pl = tid; pl < ch; pl += T) {   // (every thread reads the column it wrote)
      float t = 0.f;
      for (int n = 0; n < N; ++n) t = fmaf(g[n], sm[n * CH + pl], t);
      const float a = att_b[p0 + pl];
      const float dl = a * ((t - c) - s);
      lg[pl] = dl;
      sb += dl;
      if (gm != nullptr) {
#pragma unroll 8
        for (int n = 0; n < N; ++n) {
          const float v = fmaf(dl, w[n], a * g[n]);
          const long long i = base + (long long)n * P + p0 + pl;
          if (BF16)
            ((uint16_t*)gm)[i] = f32_to_bf16(v);
          else
            ((float*)gm)[i] = v;
        }
      }
    }
    if (part != nullptr) {
      __syncthreads();   // (sm and lg are complete)
      for (int n = wv; n < N; n += nw) {
        const float* row = sm + n * CH;
        float r = 0.f;
        for (int pl = lane; pl < ch; pl += 64) r = fmaf(lg[pl], row[pl], r);
        r = att_wave_sum(r);
        if (lane == 0) acc[n] += r;
      }
    }
  }
  if (part == nullptr) return;
  const float gb = att_block_sum(sb, red);   // (its barriers publish acc)
  float* pb = part + (long long)blockIdx.x * (N + 1);
  for (int n = tid; n < N; n += T) pb[n] = acc[n];
  if (tid == 0) pb[N] = gb;
}

// gw[j] = sum_b part[b][j], gb = sum_b part[b][N]: image order, one thread per column
__global__ void __launch_bounds__(256) attpool_reduce(int B, int N, const float* __restrict__ part, float* __restrict__ gw,
                                                      float* __restrict__ gb) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > N || (j < N ? gw == nullptr : gb == nullptr)) return;
  float s = 0.f;
#pragma unroll 8
  for (int b = 0; b < B; ++b) s += part[(long long)b * (N + 1) + j];
  if (j < N)
    gw[j] = s;
  else
    gb[0] = s;
}

}  // namespace
}  // namespace nfp

namespace nfp_host {
namespace {

// pixels per chunk: the whole image where it fits the budget, else a multiple of 64 (full wavefronts along p)
int attpool_chunk(int N, long long P) {
  long long ch = std::min<long long>(P, kAttBudgetFloats / (N + 1));
  if (ch < P && ch >= 64) ch &= ~63LL;
  return (int)ch;
}
int attpool_threads(int ch) { return std::min(kAttMaxT, std::max(256, (ch + 63) & ~63)); }
size_t attpool_lds(int N, int ch) { return ((size_t)(N + 1) * ch + N + nfp::kAttRed) * sizeof(float); }

// the checks both calls share; everything here runs before any HIP call
int attpool_args(const char* what, int32_t B, int32_t N, int64_t P, int32_t dtype) {
  if (B < 0 || N < 1 || P < 1) return fail(NFP_E_INVALID, "%s: B = %d, N = %d, P = %lld", what, B, N, (long long)P);
  if (dtype != NFP_F32 && dtype != NFP_BF16) return fail(NFP_E_INVALID, "%s: unknown dtype %d", what, dtype);
  if ((long long)N * P >= (1LL << 31))
    return fail(NFP_E_UNSUPPORTED, "%s: an image of N * P = %lld map elements (2^31 and more) has no kernel", what,
                (long long)N * P);
  if (N > kAttMaxN) return fail(NFP_E_UNSUPPORTED, "%s: N = %d maps (more than %d) has no kernel", what, N, kAttMaxN);
  return NFP_OK;
}

}  // namespace
}  // namespace nfp_host

using namespace nfp_host;

extern "C" {

int64_t nfp_attpool_scratch_floats(int32_t B, int32_t N) {
  return std::max<int64_t>(1, (int64_t)std::max(B, 0) * ((int64_t)std::max(N, 0) + 1));
}

int nfp_attpool_forward(int32_t B, int32_t N, int64_t P, int32_t dtype, const void* maps, const float* w, const float* b,
                        float* pooled, float* att, void* hip_stream) {
  if (int rc = attpool_args("nfp_attpool_forward", B, N, P, dtype)) return rc;
  // (an empty batch: maps and pooled hold no element, and torch hands such tensors over as NULL)
  if (!w || !b || (B > 0 && (!maps || !pooled))) return fail(NFP_E_INVALID, "nfp_attpool_forward: null tensor pointer");
  if (B == 0) return NFP_OK;
  const int ch = attpool_chunk(N, P), T = attpool_threads(ch);
  const bool bf = dtype == NFP_BF16;
  snprintf(g_variant, sizeof(g_variant), "attpool_fwd<%s>", bf ? "bf16" : "f32");
  hipStream_t st = (hipStream_t)hip_stream;
  const int rc = bf ? launch("attpool_fwd", nfp::attpool_fwd<1>, dim3((unsigned)B), dim3(T), attpool_lds(N, ch), st, (int)N,
                             (int)P, ch, maps, w, b, pooled, att)
                    : launch("attpool_fwd", nfp::attpool_fwd<0>, dim3((unsigned)B), dim3(T), attpool_lds(N, ch), st, (int)N,
                             (int)P, ch, maps, w, b, pooled, att);
  if (rc == NFP_OK) publish_variant();
  return rc;
}

int nfp_attpool_backward(int32_t B, int32_t N, int64_t P, int32_t dtype, const void* maps, const float* w, const float* att,
                         const float* grad_pooled, void* grad_maps, float* grad_w, float* grad_b, float* scratch,
                         int64_t scratch_floats, void* hip_stream) {
  if (int rc = attpool_args("nfp_attpool_backward", B, N, P, dtype)) return rc;
  if (!w || (B > 0 && (!maps || !att || !grad_pooled)))
    return fail(NFP_E_INVALID, "nfp_attpool_backward: null tensor pointer");
  const bool params = grad_w != nullptr || grad_b != nullptr;
  if (params && (scratch == nullptr || scratch_floats < nfp_attpool_scratch_floats(B, N)))
    return fail(NFP_E_INVALID, "nfp_attpool_backward: scratch holds %lld floats, nfp_attpool_scratch_floats is %lld",
                (long long)(scratch ? scratch_floats : 0), (long long)nfp_attpool_scratch_floats(B, N));
  if (B == 0 || (!params && grad_maps == nullptr)) return NFP_OK;
  const int ch = attpool_chunk(N, P), T = attpool_threads(ch);
  const bool bf = dtype == NFP_BF16;
  snprintf(g_variant, sizeof(g_variant), "attpool_bwd<%s>", bf ? "bf16" : "f32");
  hipStream_t st = (hipStream_t)hip_stream;
  float* part = params ? scratch : nullptr;
  int rc = bf ? launch("attpool_bwd", nfp::attpool_bwd<1>, dim3((unsigned)B), dim3(T), attpool_lds(N, ch), st, (int)N, (int)P,
                       ch, maps, w, att, grad_pooled, grad_maps, part)
              : launch("attpool_bwd", nfp::attpool_bwd<0>, dim3((unsigned)B), dim3(T), attpool_lds(N, ch), st, (int)N, (int)P,
                       ch, maps, w, att, grad_pooled, grad_maps, part);
  if (rc == NFP_OK && params)
    rc = launch("attpool_reduce", nfp::attpool_reduce, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, st, (int)B, (int)N,
                (const float*)part, grad_w, grad_b);
  if (rc == NFP_OK) publish_variant();
  return rc;
}

}  // extern "C"
