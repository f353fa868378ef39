// nfp_deepten.hip — the encoding layer of the Deep-TEN baseline (models/deepten.py::DeepTENEncoding): x [B,D,H,W] as pixels
// X [B,N,D] (N = H*W), codewords C [K,D], scale s [K]:
//   r[b,n,k,d]  = X[b,n,d] - C[k,d]                (never stored)
//   dist[b,n,k] = sum_d r^2                        (the direct form: |x|^2 - 2x.c + |c|^2 cancels)
//   A           = softmax_k(-s[k] * dist)
//   E[b,k,d]    = sum_n A[b,n,k] * r
// The reference forms r — B*N*K*D elements — twice forward and keeps it for autograd; here nothing larger than x, E, the
// assignments A / dist / w [B,N,K] and one [B,K,D] scratch of per-image partials ever reaches memory.  Backward, given G [B,K,D]:
//   dA[b,n,k] = sum_d G[b,k,d] * r       dl = A * (dA - sum_k' A dA)       w = -2 s[k] * dl
//   grad_X[b,n,d] = sum_k ( A[b,n,k] G[b,k,d] + w[b,n,k] * r )
//   grad_C[k,d]   = sum_b ( -G[b,k,d] * sum_n A[b,n,k]  -  sum_n w[b,n,k] * r )
//   grad_s[k]     = -sum_{b,n} dl * dist
//
// Two shapes of workgroup, 256 threads each:
//   dten_assign / dten_bwd_assign   a tile of pixels of one image x all K codewords: thread = (codeword k, two pixels), lanes
//       along k (KP = K rounded up to a power of two, at least 8, lanes side by side), x and the codewords (backward: G too)
//       staged in LDS by chunks of 64 channels; every thread walks d = 0 .. D-1 in order.  Then the softmax (backward: its
//       adjoint) across the KP lanes by butterflies.  Forward writes A and dist; backward w and — for grad_s — the tile's
//       sums of dl * dist, pixels in order.
//   dten_aggregate / dten_bwd_x     64 channels of one image x all K codewords x all pixels: lanes along d, the four
//       wavefronts share the codewords (k = wavefront + 4 j, j < KK), the image's x chunk and its A (backward: w too) in LDS
//       by chunks of 64 pixels; every thread walks n = 0 .. N-1 in order.  dten_bwd_x forms the image's partial of grad_C
//       first, then grad_x over the staged x tile in place, and stores the tile through the map it was loaded by.
//   dten_reduce                     both partials summed over the batch in image (and tile) order.
// A dense NCHW chunk of 64 channels is one contiguous run of 64 * N elements (read flat when the tile holds every pixel);
// a channels-last one is rows of 64 elements.  Either way neighbouring lanes take neighbouring addresses and the tile is
// transposed by where it lands in LDS (rows of 65 floats: both directions free of bank conflicts).
// Float32 arithmetic.  The softmax' adjoint is taken about the codeword of largest assignment (dA - c: exactly 0 there, a
// sum of small terms elsewhere — softmax' is shift-invariant), so a saturated assignment does not cancel.
// Every sum in a fixed order, no atomics: two runs agree bitwise, and image b's E and grad_x do not depend on the batch.
#include "nfp_launch.h"
#include "nfp_tile.h"   // (lds_poison)

#include <cmath>

namespace nfp {
namespace {

constexpr int kDtT = 256;          // threads per workgroup
constexpr int kDtDC = 64;          // channels per chunk
constexpr int kDtXS = kDtDC + 1;   // floats between two rows of a staged tile
constexpr int kDtNCH = 64;         // pixels per chunk of the channel-chunk kernels
constexpr int kDtMaxK = 64;

struct DG {            // by value in kernarg
  int N, K, D;
  int nhwc;            // 0: element (n, d) of an image at d * N + n; 1: at n * D + d
  long long sxB;       // elements between two images of x
  int KP, kshift;      // assign kernels: lanes per pixel pair (a power of two >= max(K, 8)) and its log2
  int TP, T;           // ... pixels per tile, tiles per image
  int DCH;             // channel-chunk kernels: chunks per image
  int ldsw;            // 32-bit words of dynamic LDS (lds_poison)
};

__device__ __forceinline__ long long dt_at(const DG& g, int n, int d) {
  return g.nhwc ? (long long)n * g.D + d : (long long)d * g.N + n;
}
template <int BF16>
__device__ __forceinline__ float dt_ld(const void* x, long long i) {
  return BF16 ? bf16_to_f32(((const uint16_t*)x)[i]) : ((const float*)x)[i];
}
template <int BF16>
__device__ __forceinline__ void dt_st(void* x, long long i, float v) {
  if (BF16)
    ((uint16_t*)x)[i] = f32_to_bf16(v);
  else
    ((float*)x)[i] = v;
}

// pixels [n0, n0 + tp) x channels [d0, d0 + dc) of the image at `base`: element i of the tile in the order of its addresses
template <int BF16, bool STORE>
__device__ __forceinline__ void dt_tile(const DG& g, void* x, long long base, float* xs, int n0, int tp, int d0, int dc) {
  const int tot = tp * dc;
  for (int i = threadIdx.x; i < tot; i += kDtT) {
    int p, dd;
    if (g.nhwc) {
      p = i / dc;
      dd = i - p * dc;
    } else {
      dd = i / tp;
      p = i - dd * tp;
    }
    const long long at = base + dt_at(g, n0 + p, d0 + dd);
    if (STORE)
      dt_st<BF16>(x, at, xs[p * kDtXS + dd]);
    else
      xs[p * kDtXS + dd] = dt_ld<BF16>(x, at);
  }
}

// sum / max over the KP lanes of a pixel pair's group (KP a power of two, groups aligned), the same value in each
__device__ __forceinline__ float dt_group_sum(float v, int KP) {
  for (int m = KP >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float dt_group_max(float v, int KP) {
  for (int m = KP >> 1; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
// the value `v` of the lane holding the largest `a` (of equal ones the lowest k; a NaN never wins)
__device__ __forceinline__ float dt_group_at_max(float a, int k, float v, int KP) {
  for (int m = KP >> 1; m > 0; m >>= 1) {
    const float oa = __shfl_xor(a, m, 64), ov = __shfl_xor(v, m, 64);
    const int ok = __shfl_xor(k, m, 64);
    if (oa > a || (oa == a && ok < k) || (a != a && oa == oa)) {
      a = oa;
      k = ok;
      v = ov;
    }
  }
  return v;
}

// Dynamic LDS (floats): cs[64][65] the codewords' chunk, xs[64][65] the pixels' (later the tile's dl * dist, [TP][64]),
// BWD: gs[64][65] the chunk of G.  grid = B * T, block = 256.
// Forward: writes A, dist [B,N,K].  BWD: reads them, writes w [B,N,K] and — spart not null — the tile's K sums of dl * dist,
// negated, at spart[(b * T + tile) * K].
template <int BF16, int BWD>
__global__ void __launch_bounds__(kDtT) dten_assign(DG g, const void* __restrict__ x, const float* __restrict__ cw,
                                                    const float* __restrict__ scale, float* A, float* dist,
                                                    const float* __restrict__ go, float* __restrict__ w,
                                                    float* __restrict__ spart) {
  extern __shared__ __attribute__((aligned(16))) float dt_lds[];
  lds_poison(dt_lds, g.ldsw);
  float* cs = dt_lds;
  float* xs = cs + kDtMaxK * kDtXS;
  float* gs = xs + kDtMaxK * kDtXS;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / g.T, tile = blockIdx.x - b * g.T;
  const int n0 = tile * g.TP, tp = min(g.TP, g.N - n0);
  const int k = tid & (g.KP - 1), pq = tid >> g.kshift;
  const bool live = k < g.K;
  const int kc = min(k, g.K - 1);                       // (a lane past K walks the last codeword; nothing of it is used)
  const int p0 = 2 * pq, p1 = p0 + 1;
  const bool in0 = p0 < tp, in1 = p1 < tp;
  const int r0 = min(p0, tp - 1), r1 = min(p1, tp - 1);   // (a slot past the tile walks its last pixel, likewise)
  const long long xbase = (long long)b * g.sxB;
  // The sums over d feed an exp (dist) and a difference of near-equal values (dA): a chunk is summed in eight interleaved
  // partial sums and a tree, the chunks with a compensated (Kahan) sum — a few roundings in all, where one running sum of
  // D terms collects D of them.
  float a0 = 0.f, a1 = 0.f, k0 = 0.f, k1 = 0.f;
  for (int d0 = 0; d0 < g.D; d0 += kDtDC) {
    const int dc = min(kDtDC, g.D - d0);
    if (d0) __syncthreads();   // (the previous chunk has been read)
    dt_tile<BF16, false>(g, (void*)x, xbase, xs, n0, tp, d0, dc);
    for (int i = tid; i < g.K * dc; i += kDtT) {
      const int kk = i / dc, dd = i - kk * dc;
      cs[kk * kDtXS + dd] = cw[(long long)kk * g.D + d0 + dd];
      if (BWD) gs[kk * kDtXS + dd] = go[((long long)b * g.K + kk) * g.D + d0 + dd];
    }
    __syncthreads();
    const float* cr = cs + kc * kDtXS;
    const float* gr = gs + kc * kDtXS;
    const float* x0 = xs + r0 * kDtXS;
    const float* x1 = xs + r1 * kDtXS;
    float q0[8], q1[8], t0 = 0.f, t1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) q0[j] = q1[j] = 0.f;
    int dd = 0;
    for (; dd + 8 <= dc; dd += 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c = cr[dd + j];
        const float e0 = x0[dd + j] - c, e1 = x1[dd + j] - c;
        const float m = BWD ? gr[dd + j] : 0.f;
        q0[j] = fmaf(BWD ? m : e0, e0, q0[j]);
        q1[j] = fmaf(BWD ? m : e1, e1, q1[j]);
      }
    }
    for (; dd < dc; ++dd) {   // (the last chunk's tail: at most seven terms)
      const float c = cr[dd];
      const float e0 = x0[dd] - c, e1 = x1[dd] - c;
      const float m = BWD ? gr[dd] : 0.f;
      t0 = fmaf(BWD ? m : e0, e0, t0);
      t1 = fmaf(BWD ? m : e1, e1, t1);
    }
    const float s0 = (((q0[0] + q0[1]) + (q0[2] + q0[3])) + ((q0[4] + q0[5]) + (q0[6] + q0[7]))) + t0;
    const float s1 = (((q1[0] + q1[1]) + (q1[2] + q1[3])) + ((q1[4] + q1[5]) + (q1[6] + q1[7]))) + t1;
    const float y0 = s0 - k0, y1 = s1 - k1;
    const float u0 = a0 + y0, u1 = a1 + y1;
    k0 = (u0 - a0) - y0;
    k1 = (u1 - a1) - y1;
    a0 = u0;
    a1 = u1;
  }
  const float s = scale[kc];
  const long long i0 = ((long long)b * g.N + n0 + r0) * g.K + kc, i1 = ((long long)b * g.N + n0 + r1) * g.K + kc;
  if (!BWD) {
    // softmax over k of l = -s * dist; the lanes past K hold -inf and 0
    const float l0 = live ? -s * a0 : -INFINITY, l1 = live ? -s * a1 : -INFINITY;
    const float m0 = dt_group_max(l0, g.KP), m1 = dt_group_max(l1, g.KP);
    const float e0 = live ? expf(l0 - m0) : 0.f, e1 = live ? expf(l1 - m1) : 0.f;
    const float z0 = dt_group_sum(e0, g.KP), z1 = dt_group_sum(e1, g.KP);
    if (live && in0) {
      A[i0] = e0 / z0;
      dist[i0] = a0;
    }
    if (live && in1) {
      A[i1] = e1 / z1;
      dist[i1] = a1;
    }
    return;
  }
  // a0, a1: dA.  dl = A (dA - sum_k A dA), about the codeword of largest A (file comment)
  const float A0 = live ? A[i0] : 0.f, A1 = live ? A[i1] : 0.f;
  const float c0 = dt_group_at_max(live ? A0 : -INFINITY, k, a0, g.KP);
  const float c1 = dt_group_at_max(live ? A1 : -INFINITY, k, a1, g.KP);
  const float t0 = a0 - c0, t1 = a1 - c1;
  const float S0 = dt_group_sum(live ? A0 * t0 : 0.f, g.KP), S1 = dt_group_sum(live ? A1 * t1 : 0.f, g.KP);
  const float dl0 = A0 * (t0 - S0), dl1 = A1 * (t1 - S1);
  if (live && in0) w[i0] = -2.f * s * dl0;
  if (live && in1) w[i1] = -2.f * s * dl1;
  if (spart == nullptr) return;
  __syncthreads();   // (every thread has left the chunk loop: xs is free)
  if (live && in0) xs[p0 * kDtMaxK + k] = dl0 * dist[i0];
  if (live && in1) xs[p1 * kDtMaxK + k] = dl1 * dist[i1];
  __syncthreads();
  if (tid < g.K) {
    float q = 0.f;
    for (int p = 0; p < tp; ++p) q += xs[p * kDtMaxK + tid];
    spart[((long long)b * g.T + tile) * g.K + tid] = -q;
  }
}

// the codewords of wavefront wv: k = wv + 4 j, j < KK (past K: the last codeword again; nothing of it is stored)
template <int KK>
__device__ __forceinline__ void dt_ks(int K, int wv, int (&kk)[KK]) {
#pragma unroll
  for (int j = 0; j < KK; ++j) kk[j] = min(wv + 4 * j, K - 1);
}

// Dynamic LDS (floats): xs[nchmax][65] the x tile, As[nchmax * K] the assignments of its pixels.  grid = B * DCH, block = 256.
template <int BF16, int KK>
__global__ void __launch_bounds__(kDtT) dten_aggregate(DG g, const void* __restrict__ x, const float* __restrict__ cw,
                                                       const float* __restrict__ A, void* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float dt_lds[];
  lds_poison(dt_lds, g.ldsw);
  const int nchmax = min(g.N, kDtNCH);
  float* xs = dt_lds;
  float* As = xs + nchmax * kDtXS;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x / g.DCH, ch = blockIdx.x - b * g.DCH;
  const int d0 = ch * kDtDC, dc = min(kDtDC, g.D - d0);
  const int d = d0 + min(lane, dc - 1), ld = min(lane, dc - 1);   // (a lane past the chunk walks its last channel)
  const long long xbase = (long long)b * g.sxB;
  int kk[KK];
  dt_ks<KK>(g.K, wv, kk);
  float c[KK], acc[KK];
#pragma unroll
  for (int j = 0; j < KK; ++j) {
    c[j] = cw[(long long)kk[j] * g.D + d];
    acc[j] = 0.f;
  }
  for (int n0 = 0; n0 < g.N; n0 += kDtNCH) {
    const int nch = min(kDtNCH, g.N - n0);
    if (n0) __syncthreads();   // (the previous chunk has been read)
    dt_tile<BF16, false>(g, (void*)x, xbase, xs, n0, nch, d0, dc);
    const float* Ab = A + ((long long)b * g.N + n0) * g.K;
    for (int i = tid; i < nch * g.K; i += kDtT) As[i] = Ab[i];
    __syncthreads();
    for (int n = 0; n < nch; ++n) {
      const float xv = xs[n * kDtXS + ld];
      const float* an = As + n * g.K;
#pragma unroll
      for (int j = 0; j < KK; ++j) acc[j] = fmaf(an[kk[j]], xv - c[j], acc[j]);
    }
  }
  if (lane >= dc) return;
#pragma unroll
  for (int j = 0; j < KK; ++j)
    if (wv + 4 * j < g.K) dt_st<BF16>(out, ((long long)b * g.K + wv + 4 * j) * g.D + d, acc[j]);
}

// Dynamic LDS (floats): xs[nchmax][65], As[nchmax * K], ws[nchmax * K], and — gx not null — gs[K][64], cs[K][64] the chunks
// of G and of the codewords.  grid = B * DCH, block = 256.  gx: the dense grad_x in x's layout, or null; cpart: the image's
// partial of grad_C at cpart[b * K * D], or null.
template <int BF16, int KK>
__global__ void __launch_bounds__(kDtT) dten_bwd_x(DG g, const void* __restrict__ x, const float* __restrict__ cw,
                                                   const float* __restrict__ A, const float* __restrict__ w,
                                                   const float* __restrict__ go, void* __restrict__ gx,
                                                   float* __restrict__ cpart) {
  extern __shared__ __attribute__((aligned(16))) float dt_lds[];
  lds_poison(dt_lds, g.ldsw);
  const int nchmax = min(g.N, kDtNCH);
  float* xs = dt_lds;
  float* As = xs + nchmax * kDtXS;
  float* ws = As + nchmax * g.K;
  float* gs = ws + nchmax * g.K;
  float* cs = gs + g.K * kDtDC;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x / g.DCH, ch = blockIdx.x - b * g.DCH;
  const int d0 = ch * kDtDC, dc = min(kDtDC, g.D - d0);
  const int ld = min(lane, dc - 1), d = d0 + ld;
  const long long xbase = (long long)b * g.sxB, gxbase = (long long)b * g.N * g.D;
  const float* gob = go + (long long)b * g.K * g.D;
  int kk[KK];
  dt_ks<KK>(g.K, wv, kk);
  float c[KK], gv[KK], acc[KK], sa[KK];
#pragma unroll
  for (int j = 0; j < KK; ++j) {
    c[j] = cw[(long long)kk[j] * g.D + d];
    gv[j] = gob[(long long)kk[j] * g.D + d];
    acc[j] = 0.f;
    sa[j] = 0.f;
  }
  if (gx != nullptr) {
    for (int i = tid; i < g.K * kDtDC; i += kDtT) {
      const int k = i >> 6, dd = d0 + min(i & 63, dc - 1);
      gs[i] = gob[(long long)k * g.D + dd];
      cs[i] = cw[(long long)k * g.D + dd];
    }
  }
  for (int n0 = 0; n0 < g.N; n0 += kDtNCH) {
    const int nch = min(kDtNCH, g.N - n0);
    if (n0) __syncthreads();   // (the previous chunk has been read and stored)
    dt_tile<BF16, false>(g, (void*)x, xbase, xs, n0, nch, d0, dc);
    const long long ab = ((long long)b * g.N + n0) * g.K;
    for (int i = tid; i < nch * g.K; i += kDtT) {
      As[i] = A[ab + i];
      ws[i] = w[ab + i];
    }
    __syncthreads();   // (also: gs and cs are complete)
    if (cpart != nullptr) {
      for (int n = 0; n < nch; ++n) {
        const float xv = xs[n * kDtXS + ld];
        const float* an = As + n * g.K;
        const float* wn = ws + n * g.K;
#pragma unroll
        for (int j = 0; j < KK; ++j) {
          acc[j] = fmaf(wn[kk[j]], xv - c[j], acc[j]);
          sa[j] += an[kk[j]];
        }
      }
    }
    if (gx == nullptr) continue;
    if (cpart != nullptr) __syncthreads();   // (every wavefront has read the x tile: grad_x takes its place)
    for (int n = wv; n < nch; n += 4) {
      const float xv = xs[n * kDtXS + ld];
      const float* an = As + n * g.K;
      const float* wn = ws + n * g.K;
      float ta[2] = {0.f, 0.f}, tw[2] = {0.f, 0.f};   // (the two families apart, even and odd k apart: four short sums)
      int k = 0;
      for (; k + 2 <= g.K; k += 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          ta[j] = fmaf(an[k + j], gs[(k + j) * kDtDC + lane], ta[j]);
          tw[j] = fmaf(wn[k + j], xv - cs[(k + j) * kDtDC + lane], tw[j]);
        }
      }
      if (k < g.K) {
        ta[0] = fmaf(an[k], gs[k * kDtDC + lane], ta[0]);
        tw[0] = fmaf(wn[k], xv - cs[k * kDtDC + lane], tw[0]);
      }
      const float t = (ta[0] + ta[1]) + (tw[0] + tw[1]);
      if (lane < dc) xs[n * kDtXS + lane] = t;
    }
    __syncthreads();
    dt_tile<BF16, true>(g, gx, gxbase, xs, n0, nch, d0, dc);
  }
  if (cpart == nullptr || lane >= dc) return;
#pragma unroll
  for (int j = 0; j < KK; ++j)
    if (wv + 4 * j < g.K) cpart[((long long)b * g.K + wv + 4 * j) * g.D + d] = -fmaf(gv[j], sa[j], acc[j]);
}

// grad_C[j] = sum_b cpart[b][j] (one thread per element, image order); grad_s[k] = sum_i spart[i][k], i over the BT tiles
// of the batch (one workgroup per k: thread t takes i = t, t + 256, ..., then the 256 sums in a fixed tree).
// grid = cblocks + (gs ? K : 0), block = 256.
__global__ void __launch_bounds__(kDtT) dten_reduce(int B, long long KD, int K, long long BT, unsigned cblocks,
                                                    const float* __restrict__ cpart, const float* __restrict__ spart,
                                                    float* __restrict__ gc, float* __restrict__ gsc) {
  __shared__ float red[kDtT / 64];
  if (blockIdx.x < cblocks) {
    const long long j = (long long)blockIdx.x * kDtT + threadIdx.x;
    if (j >= KD) return;
    float s = 0.f;
#pragma unroll 8
    for (int b = 0; b < B; ++b) s += cpart[(long long)b * KD + j];
    gc[j] = s;
    return;
  }
  const int k = blockIdx.x - cblocks;
  float s = 0.f;
  for (long long i = threadIdx.x; i < BT; i += kDtT) s += spart[i * K + k];
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) gsc[k] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace
}  // namespace nfp

namespace nfp_host {
namespace {

// the sizes both calls share; everything here runs before any HIP call
int deepten_geometry(const char* what, int32_t B, int64_t N, int32_t K, int32_t D, int32_t dtype, int32_t layout, int64_t sxB,
                     nfp::DG& g) {
  if (B < 0 || N < 1 || K < 1 || D < 1)
    return fail(NFP_E_INVALID, "%s: B = %d, N = %lld, K = %d, D = %d", what, B, (long long)N, K, D);
  if (dtype != NFP_F32 && dtype != NFP_BF16) return fail(NFP_E_INVALID, "%s: unknown dtype %d", what, dtype);
  if (layout != NFP_ACT_NCHW && layout != NFP_ACT_NHWC) return fail(NFP_E_INVALID, "%s: unknown layout %d", what, layout);
  if (sxB < 0) return fail(NFP_E_INVALID, "%s: batch stride %lld", what, (long long)sxB);
  if (K > kDtMaxK) return fail(NFP_E_UNSUPPORTED, "%s: K = %d codewords (more than %d) has no kernel", what, K, kDtMaxK);
  const long long lim = 1LL << 31;
  if (N >= lim || N * D >= lim || N * K >= lim || (long long)K * D >= lim)
    return fail(NFP_E_UNSUPPORTED, "%s: an image of N = %lld, N * D = %lld (2^31 and more) has no kernel", what, (long long)N,
                (long long)N * D);
  g.N = (int)N;
  g.K = K;
  g.D = D;
  g.nhwc = layout == NFP_ACT_NHWC;
  g.sxB = sxB;
  g.KP = 8;
  g.kshift = 3;
  while (g.KP < K) {
    g.KP <<= 1;
    g.kshift++;
  }
  g.TP = 2 * (kDtT / g.KP);
  g.T = (int)((N + g.TP - 1) / g.TP);
  g.DCH = (D + kDtDC - 1) / kDtDC;
  g.ldsw = 0;
  if ((long long)B * g.T >= lim || (long long)B * g.DCH >= lim)
    return fail(NFP_E_UNSUPPORTED, "%s: B = %d images of %d pixel tiles / %d channel chunks: more workgroups than a launch holds",
                what, B, g.T, g.DCH);
  return NFP_OK;
}
int deepten_tiles(int64_t N, int32_t K) {   // g.T of deepten_geometry
  int kp = 8;
  while (kp < K) kp <<= 1;
  const int tp = 2 * (kDtT / kp);
  return (int)((N + tp - 1) / tp);
}
size_t deepten_assign_lds(bool bwd) { return (size_t)(bwd ? 3 : 2) * kDtMaxK * kDtXS * sizeof(float); }
size_t deepten_chunk_lds(const nfp::DG& g, bool bwd, bool gx) {
  const size_t nch = std::min(g.N, kDtNCH);
  return (nch * kDtXS + (bwd ? 2 : 1) * nch * g.K + (gx ? 2 : 0) * (size_t)g.K * kDtDC) * sizeof(float);
}
// K -> the codewords per wavefront the channel-chunk kernels are instantiated for
template <typename F>
int with_kk(int K, F&& f) {
  if (K <= 8) return f(Int<2>{});
  if (K <= 16) return f(Int<4>{});
  if (K <= 32) return f(Int<8>{});
  return f(Int<16>{});
}
const char* deepten_tag(bool bf, const nfp::DG& g) {
  return bf ? (g.nhwc ? "bf16,nhwc" : "bf16,nchw") : (g.nhwc ? "f32,nhwc" : "f32,nchw");
}

}  // namespace
}  // namespace nfp_host

using namespace nfp_host;

extern "C" {

int64_t nfp_deepten_saved_floats(int32_t B, int64_t N, int32_t K) {
  return std::max<int64_t>(1, 2 * (int64_t)std::max(B, 0) * std::max<int64_t>(N, 0) * std::max(K, 0));
}

int64_t nfp_deepten_scratch_floats(int32_t B, int64_t N, int32_t K, int32_t D, int32_t want_params) {
  const int64_t b = std::max(B, 0), n = std::max<int64_t>(N, 0), k = std::max(K, 0), d = std::max(D, 0);
  int64_t f = b * n * k;                                                   // w
  if (want_params && n > 0 && k > 0) f += b * k * d + b * deepten_tiles(n, K) * k;   // the partials of grad_C and of grad_s
  return std::max<int64_t>(1, f);
}

int nfp_deepten_forward(int32_t B, int64_t N, int32_t K, int32_t D, int32_t dtype, int32_t layout, int64_t sxB, const void* x,
                        const float* codewords, const float* scale, void* out, float* saved, int64_t saved_floats,
                        void* hip_stream) {
  nfp::DG g;
  if (int rc = deepten_geometry("nfp_deepten_forward", B, N, K, D, dtype, layout, sxB, g)) return rc;
  // (an empty batch: x, out and saved hold no element, and torch hands such tensors over as NULL)
  if (!codewords || !scale || (B > 0 && (!x || !out || !saved)))
    return fail(NFP_E_INVALID, "nfp_deepten_forward: null tensor pointer");
  if (B > 0 && saved_floats < nfp_deepten_saved_floats(B, N, K))
    return fail(NFP_E_INVALID, "nfp_deepten_forward: saved holds %lld floats, nfp_deepten_saved_floats is %lld",
                (long long)saved_floats, (long long)nfp_deepten_saved_floats(B, N, K));
  if (B == 0) return NFP_OK;
  const bool bf = dtype == NFP_BF16;
  snprintf(g_variant, sizeof(g_variant), "dten_fwd<%s>", deepten_tag(bf, g));
  hipStream_t st = (hipStream_t)hip_stream;
  float* A = saved;
  float* dist = saved + (long long)B * N * K;
  size_t lds = deepten_assign_lds(false);
  g.ldsw = (int)(lds / 4);
  const dim3 grid_a((unsigned)((long long)B * g.T)), block(kDtT);
  int rc = bf ? launch("dten_assign", nfp::dten_assign<1, 0>, grid_a, block, lds, st, g, x, codewords, scale, A, dist,
                       (const float*)nullptr, (float*)nullptr, (float*)nullptr)
              : launch("dten_assign", nfp::dten_assign<0, 0>, grid_a, block, lds, st, g, x, codewords, scale, A, dist,
                       (const float*)nullptr, (float*)nullptr, (float*)nullptr);
  if (rc != NFP_OK) return rc;
  lds = deepten_chunk_lds(g, false, false);
  g.ldsw = (int)(lds / 4);
  const dim3 grid_c((unsigned)((long long)B * g.DCH));
  rc = with_kk(K, [&](auto kk) {
    constexpr int KK = decltype(kk)::value;
    return bf ? launch("dten_aggregate", nfp::dten_aggregate<1, KK>, grid_c, block, lds, st, g, x, codewords, (const float*)A, out)
              : launch("dten_aggregate", nfp::dten_aggregate<0, KK>, grid_c, block, lds, st, g, x, codewords, (const float*)A, out);
  });
  if (rc == NFP_OK) publish_variant();
  return rc;
}

int nfp_deepten_backward(int32_t B, int64_t N, int32_t K, int32_t D, int32_t dtype, int32_t layout, int64_t sxB, const void* x,
                         const float* codewords, const float* scale, const float* saved, int64_t saved_floats,
                         const float* grad_out, void* grad_x, float* grad_codewords, float* grad_scale, float* scratch,
                         int64_t scratch_floats, void* hip_stream) {
  nfp::DG g;
  if (int rc = deepten_geometry("nfp_deepten_backward", B, N, K, D, dtype, layout, sxB, g)) return rc;
  if (!codewords || !scale || (B > 0 && (!x || !saved || !grad_out)))
    return fail(NFP_E_INVALID, "nfp_deepten_backward: null tensor pointer");
  if (B > 0 && saved_floats < nfp_deepten_saved_floats(B, N, K))
    return fail(NFP_E_INVALID, "nfp_deepten_backward: saved holds %lld floats, nfp_deepten_saved_floats is %lld",
                (long long)saved_floats, (long long)nfp_deepten_saved_floats(B, N, K));
  const bool params = grad_codewords != nullptr || grad_scale != nullptr;
  const bool any = params || grad_x != nullptr;
  const int64_t need = nfp_deepten_scratch_floats(B, N, K, D, params);
  if (B > 0 && any && (scratch == nullptr || scratch_floats < need))
    return fail(NFP_E_INVALID, "nfp_deepten_backward: scratch holds %lld floats, nfp_deepten_scratch_floats is %lld",
                (long long)(scratch ? scratch_floats : 0), (long long)need);
  if (B == 0 || !any) return NFP_OK;
  const bool bf = dtype == NFP_BF16;
  snprintf(g_variant, sizeof(g_variant), "dten_bwd<%s>", deepten_tag(bf, g));
  hipStream_t st = (hipStream_t)hip_stream;
  const long long bnk = (long long)B * N * K, bkd = (long long)B * K * D;
  const float* A = saved;
  const float* dist = saved + bnk;
  float* w = scratch;
  float* cpart = grad_codewords != nullptr ? scratch + bnk : nullptr;
  float* spart = grad_scale != nullptr ? scratch + bnk + bkd : nullptr;
  size_t lds = deepten_assign_lds(true);
  g.ldsw = (int)(lds / 4);
  const dim3 grid_a((unsigned)((long long)B * g.T)), block(kDtT);
  int rc = bf ? launch("dten_bwd_assign", nfp::dten_assign<1, 1>, grid_a, block, lds, st, g, x, codewords, scale, (float*)A,
                       (float*)dist, grad_out, w, spart)
              : launch("dten_bwd_assign", nfp::dten_assign<0, 1>, grid_a, block, lds, st, g, x, codewords, scale, (float*)A,
                       (float*)dist, grad_out, w, spart);
  if (rc != NFP_OK) return rc;
  if (grad_x != nullptr || cpart != nullptr) {
    lds = deepten_chunk_lds(g, true, grad_x != nullptr);
    g.ldsw = (int)(lds / 4);
    const dim3 grid_c((unsigned)((long long)B * g.DCH));
    rc = with_kk(K, [&](auto kk) {
      constexpr int KK = decltype(kk)::value;
      return bf ? launch("dten_bwd_x", nfp::dten_bwd_x<1, KK>, grid_c, block, lds, st, g, x, codewords, A, (const float*)w,
                         grad_out, grad_x, cpart)
                : launch("dten_bwd_x", nfp::dten_bwd_x<0, KK>, grid_c, block, lds, st, g, x, codewords, A, (const float*)w,
                         grad_out, grad_x, cpart);
    });
    if (rc != NFP_OK) return rc;
  }
  if (params) {
    const long long KD = (long long)K * D;
    const unsigned cblocks = cpart != nullptr ? (unsigned)((KD + kDtT - 1) / kDtT) : 0u;
    rc = launch("dten_reduce", nfp::dten_reduce, dim3(cblocks + (spart != nullptr ? (unsigned)K : 0u)), block, 0, st, (int)B, KD,
                (int)K, (long long)B * g.T, cblocks, (const float*)cpart, (const float*)spart, grad_codewords, grad_scale);
    if (rc != NFP_OK) return rc;
  }
  publish_variant();
  return NFP_OK;
}

}  // extern "C"
