// nfp_cp_kernels.h — the kernels of the compress-BN family (nfp_cpool_*, nfp_cpool_wide_*, nfp_cproj_*, nfp_cpsync_*): CpK, the
// one argument block they all take, and every __global__ function with its __device__ helpers.  The formulas, the list of
// kernels and the host path that launches them are nfp_cpool.hip's, which alone includes this file.
#pragma once
#include "nfp_launch.h"

#include <cmath>

namespace nfp {
namespace {

constexpr int kCpT = 512;         // threads of cpool_fwd / cpool_bwd_part / cp_bwd_maps: 8 wavefronts
constexpr int kCpW = kCpT / 64;
constexpr int kCpDT = 128;        // channels of D per workgroup: 64 lanes x 2
constexpr int kCpBudget = 8192;   // floats of maps per chunk (32 KiB): with the join buffers a workgroup stays near 50 KiB
constexpr int kCpMaxN = 32;
constexpr int kCpRT = 32;         // channels of D per workgroup of cpool_bwd_reduce
constexpr int kCpMT = 256;        // threads of cpool_moments / cpool_bwd_reduce
constexpr int kCpFT = 1024;       // threads of cpool_finish
constexpr int kCpMB = 128;        // channels of D per LDS block of cp_bwd_maps

struct CpK {
  int B, N, P, CH, CHs, D, bf16, eval, S, ipw, nc, ntr;
  float eps;
  double eps64, mom, M;
  const void* maps;
  const float *w, *gamma, *beta, *rm, *rv, *stats, *go, *part, *kq;
  float *out, *stats_w, *part_w, *kq_w, *rm_w, *rv_w, *gw, *gg, *gb;
  void* gm;
  const void* gov;   // cproj: grad_out [B,D,P] and out [B,D,P] in the maps' dtype
  void* outv;
};
// stats (the forward's saved state, training): mu_hi [N], mu_lo [N], Sigma [N*N], inv [D]
__device__ __forceinline__ const float* cp_inv(const CpK& k) { return k.stats + 2 * k.N + k.N * k.N; }

__device__ __forceinline__ float cp_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// s_d = gamma_d inv_d and the shift of channel d (file comment)
__device__ __forceinline__ void cp_coef(const CpK& k, int d, float& scale, float& shift) {
  const float inv = k.eval ? 1.f / sqrtf(k.rv[d] + k.eps) : cp_inv(k)[d];
  scale = k.gamma[d] * inv;
  shift = k.eval ? k.beta[d] - scale * k.rm[d] : k.beta[d];
}

// element j of a tensor of the maps' dtype (the maps, or cproj's grad_out) as float32
__device__ __forceinline__ float cj_load(const CpK& k, const void* p, long long j) {
  return k.bf16 ? bf16_to_f32(((const uint16_t*)p)[j]) : ((const float*)p)[j];
}

// ... and v stored there
__device__ __forceinline__ void cj_store(const CpK& k, void* p, long long j, float v) {
  if (k.bf16)
    ((uint16_t*)p)[j] = f32_to_bf16(v);
  else
    ((float*)p)[j] = v;
}

// element j of the maps, of map n: centred about mu, which the statistics hold as two floats
__device__ __forceinline__ float cp_map(const CpK& k, int n, long long j, bool centre) {
  float v = cj_load(k, k.maps, j);
  if (centre) v = (v - k.stats[n]) - k.stats[k.N + n];
  return v;
}

// The chunk [p0, p0 + ch) of image b into sm[NP][CHs] as centred float32; rows n >= N and pixels >= ch are zero.
__device__ __forceinline__ void cp_stage(const CpK& k, int NP, float* sm, int b, int p0, int ch, bool centre) {
  const long long base = (long long)b * k.N * k.P + p0;
  const int total = NP * k.CHs;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int n = i / k.CHs, pl = i - n * k.CHs;
    sm[i] = (n < k.N && pl < ch) ? cp_map(k, n, base + (long long)n * k.P + pl, centre) : 0.f;
  }
}

// dst[i] = the sum over the k.ntr rows [k (N), Q (N * N)] that k.kq names, in row order: the workgroups' shares of
// cpool_bwd_reduce, or the ranks' rows.  T: the threads of the workgroup.
template <int T>
__device__ __forceinline__ void cp_kq_sum(const CpK& k, float* dst) {
  const int L = k.N + k.N * k.N;
  for (int i = threadIdx.x; i < L; i += T) {
    float s = 0.f;
#pragma unroll 8
    for (int t = 0; t < k.ntr; ++t) s += k.kq[(long long)t * L + i];
    dst[i] = s;
  }
}

// ---- moments ---------------------------------------------------------------------------------------------------------------
// The first passes over a staged chunk sm[.][CHs] of ch pixels, by 256 threads: the mean of map n as a float32 anchor
// a_n, then the map centred about it in place and the mean r_n of what is left; outp takes [a (N), r (N)].  Rows n >= N
// and pixels >= ch stay zero.  Ends behind a barrier.
__device__ __forceinline__ void cp_anchor_centre(const CpK& k, float* sm, float* anchor, int ch, float* outp) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = kCpMT >> 6, N = k.N;
  for (int n = wv; n < N; n += nw) {
    float s = 0.f;
    for (int pl = lane; pl < ch; pl += 64) s += sm[n * k.CHs + pl];
    s = cp_wave_sum(s);
    if (lane == 0) anchor[n] = s / (float)ch;
  }
  __syncthreads();
  for (int n = wv; n < N; n += nw) {
    const float an = anchor[n];
    float s = 0.f;
    for (int pl = lane; pl < ch; pl += 64) {
      const float c = sm[n * k.CHs + pl] - an;
      sm[n * k.CHs + pl] = c;
      s += c;
    }
    s = cp_wave_sum(s);
    if (lane == 0) {
      outp[n] = an;
      outp[N + n] = s / (float)ch;
    }
  }
  __syncthreads();
}

// grid = B * nc chunks, block = 256.  LDS: sm[NP * CHs], anchor[NP], red[max(NP * NP, 256)].
// part_w: per chunk [a (N), r (N), Gram (N * N)].
__global__ void __launch_bounds__(kCpMT) cpool_moments(CpK k, int NP) {
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  float* sm = cp_lds;
  float* anchor = sm + NP * k.CHs;
  float* red = anchor + NP;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / k.nc, j = blockIdx.x - b * k.nc;
  const int p0 = j * k.CH, ch = min(k.CH, k.P - p0);
  const int N = k.N, NN = NP * NP;
  float* outp = k.part_w + (long long)blockIdx.x * (2 * N + N * N);
  cp_stage(k, NP, sm, b, p0, ch, false);
  __syncthreads();
  cp_anchor_centre(k, sm, anchor, ch, outp);
  // Gram about the anchor: pair (n, n2) per thread, the pixels in quads; with fewer pairs than threads the quads are dealt
  // to T / NN slices and joined in slice order
  const int nq = (ch + 3) >> 2;
  const int nsl = NN >= kCpMT ? 1 : kCpMT / NN;
  for (int pr0 = 0; pr0 < NN; pr0 += kCpMT) {
    const int pr = nsl > 1 ? tid % NN : pr0 + tid;
    const int sl = nsl > 1 ? tid / NN : 0;
    if (pr < NN && sl < nsl) {
      const int n = pr / NP, n2 = pr - n * NP;
      const float4* ra = (const float4*)(sm + n * k.CHs);
      const float4* rb = (const float4*)(sm + n2 * k.CHs);
      float g = 0.f;
      for (int q = sl; q < nq; q += nsl) {
        const float4 x = ra[q], y = rb[q];
        g = fmaf(x.x, y.x, g);
        g = fmaf(x.y, y.y, g);
        g = fmaf(x.z, y.z, g);
        g = fmaf(x.w, y.w, g);
      }
      if (nsl > 1) {
        red[sl * NN + pr] = g;
      } else if (n < N && n2 < N) {
        outp[2 * N + n * N + n2] = g;
      }
    }
  }
  if (nsl > 1) {
    __syncthreads();
    if (tid < NN) {
      const int n = tid / NP, n2 = tid - n * NP;
      float g = red[tid];
      for (int s = 1; s < nsl; ++s) g += red[s * NN + tid];
      if (n < N && n2 < N) outp[2 * N + n * N + n2] = g;
    }
  }
}

// The join of a rank's B * nc chunk records, by the 1024 threads of a workgroup (red[1024], mu[32], sig[32][32], zero beyond
// N).  The chunks are dealt to slices of consecutive chunks — 32 slices for mu, 1024 / N^2 for Sigma — whose sums are joined
// in slice order: one thread walking all B * nc chunks is a chain of dependent global loads (measured: 100 us at 64 chunks).
// RECORD (cps_record): sig keeps the scatter about mu undivided, and a rank without a chunk has mu = 0.
template <bool RECORD>
__device__ __forceinline__ void cp_join_chunks(const CpK& k, double* mu, double* sig, double* red) {
  const int tid = threadIdx.x, N = k.N, NN = N * N, K = k.B * k.nc, rec = 2 * N + NN;
  const int last = k.P - (k.nc - 1) * k.CH;   // pixels of an image's last chunk
  {
    const int n = tid & 31, sl = tid >> 5, Kc = (K + 31) / 32;
    const int c0 = min(K, sl * Kc), c1 = min(K, c0 + Kc);
    double s = 0.0;
    if (n < N) {
      int j = c0 % k.nc;
#pragma unroll 4
      for (int c = c0; c < c1; ++c) {
        const float* r = k.part + (long long)c * rec;
        const double cnt = j == k.nc - 1 ? last : k.CH;
        s += cnt * ((double)r[n] + (double)r[N + n]);
        if (++j == k.nc) j = 0;
      }
    }
    red[tid] = s;
    sig[tid] = 0.0;
    __syncthreads();
    if (tid < N) {
      double t = red[tid];
      for (int i = 1; i < 32; ++i) t += red[i * 32 + tid];
      mu[tid] = RECORD && K == 0 ? 0.0 : t / k.M;
    }
    __syncthreads();
  }
  {
    const int nsl = kCpFT / NN, pr = tid % NN, sl = tid / NN, Kc = (K + nsl - 1) / nsl;
    const int n = pr / N, n2 = pr - n * N;
    if (sl < nsl) {
      const int c0 = min(K, sl * Kc), c1 = min(K, c0 + Kc);
      const double m1 = mu[n], m2 = mu[n2];
      double s = 0.0;
      int j = c0 % k.nc;
#pragma unroll 4
      for (int c = c0; c < c1; ++c) {
        const float* r = k.part + (long long)c * rec;
        const double cnt = j == k.nc - 1 ? last : k.CH;
        const double d1 = (double)r[n] - m1, d2 = (double)r[n2] - m2, r1 = r[N + n], r2 = r[N + n2];
        s += (double)r[2 * N + pr] + cnt * (r1 * d2 + d1 * r2 + d1 * d2);
        if (++j == k.nc) j = 0;
      }
      red[sl * NN + pr] = s;
    }
    __syncthreads();
    if (tid < NN) {
      double t = red[tid];
      for (int i = 1; i < nsl; ++i) t += red[i * NN + tid];
      sig[n * kCpMaxN + n2] = RECORD ? t : t / k.M;
    }
    __syncthreads();
  }
}

// What follows mu and Sigma over M values per channel: they go to stats_w (workgroup 0), and channel d = blockIdx.x * 1024 +
// tid gets w_d' Sigma w_d, inv_d and its running statistics.
__device__ __forceinline__ void cp_finish_channels(const CpK& k, const double* mu, const double* sig, double M) {
  const int tid = threadIdx.x, N = k.N, NN = N * N;
  if (blockIdx.x == 0) {
    if (tid < N) {
      const float hi = (float)mu[tid];
      k.stats_w[tid] = hi;
      k.stats_w[N + tid] = (float)(mu[tid] - (double)hi);
    }
    if (tid < NN) k.stats_w[2 * N + tid] = (float)sig[(tid / N) * kCpMaxN + tid % N];
  }
  const int d = blockIdx.x * kCpFT + tid;
  if (d >= k.D) return;
  const float* wd = k.w + (long long)d * N;
  double wr[kCpMaxN];   // (every index a constant below: registers)
#pragma unroll
  for (int n = 0; n < kCpMaxN; ++n) wr[n] = n < N ? (double)wd[n] : 0.0;
  double var = 0.0, mean = 0.0;
#pragma unroll
  for (int n = 0; n < kCpMaxN; ++n) {
    if (n < N) {   // (the same in every thread)
      double v = 0.0;
#pragma unroll
      for (int n2 = 0; n2 < kCpMaxN; ++n2) v += sig[n * kCpMaxN + n2] * wr[n2];
      var += wr[n] * v;
      mean += wr[n] * mu[n];
    }
  }
  var = var > 0.0 ? var : 0.0;
  k.stats_w[2 * N + NN + d] = (float)(1.0 / sqrt(var + k.eps64));
  if (k.rm_w != nullptr) {
    k.rm_w[d] = (float)((1.0 - k.mom) * (double)k.rm_w[d] + k.mom * mean);
    k.rv_w[d] = (float)((1.0 - k.mom) * (double)k.rv_w[d] + k.mom * var * (M / (M - 1.0)));
  }
}

// grid = ceil(D / 1024), block = 1024; every workgroup joins the chunks itself (the same sums in the same order).
__global__ void __launch_bounds__(kCpFT) cpool_finish(CpK k) {
  __shared__ double mu[kCpMaxN];
  __shared__ double sig[kCpMaxN * kCpMaxN];   // [32][32], zero beyond N
  __shared__ double red[kCpFT];
  cp_join_chunks<false>(k, mu, sig, red);
  cp_finish_channels(k, mu, sig, k.M);
}

// ---- the statistics across ranks (nfp_cpsync_*) ----------------------------------------------------------------------------
// A rank's record, float64: [n, mu (N), S (N * N)] — its count of values per map, their mean, and their scatter about that
// mean, not divided.  grid = 1, block = 1024: cpool_finish's join of the rank's chunk records; a rank without an image
// (B = 0: no chunk) writes n = 0, mu = 0, S = 0.
__global__ void __launch_bounds__(kCpFT) cps_record(CpK k, double* rec) {
  __shared__ double mu[kCpMaxN];
  __shared__ double sig[kCpMaxN * kCpMaxN];
  __shared__ double red[kCpFT];
  cp_join_chunks<true>(k, mu, sig, red);
  const int tid = threadIdx.x, N = k.N, NN = N * N;
  if (tid == 0) rec[0] = k.M;
  if (tid < N) rec[1 + tid] = mu[tid];
  if (tid < NN) rec[1 + N + tid] = sig[(tid / N) * kCpMaxN + tid % N];
}

// grid = ceil(D / 1024), block = 1024: cpool_finish over the records of `world` ranks instead of one rank's chunks, joined
// in rank order by every workgroup (the same sums in the same order on every rank that holds the same records):
//   M = sum n_r      mu = sum n_r mu_r / M      Sigma = sum_r (S_r + n_r d_r d_r') / M,  d_r = mu_r - mu
// stats_w takes more than cpool_finish writes, behind inv [D]: (float)M, the count the backward divides by, and what
// Sigma [N * N] loses as a float.  Ranks whose means lie far apart put the variance into the between-rank term — every
// entry of Sigma large, the differences between them small — and grad_w, a difference of T and Sigma w, needs both floats
// (means of +-100 at unit spread: 1.1e-4 of max|grad_w| with one, measured).
__global__ void __launch_bounds__(kCpFT) cps_finish(CpK k, const double* recs, int world) {
  __shared__ double mu[kCpMaxN];
  __shared__ double sig[kCpMaxN * kCpMaxN];
  const int tid = threadIdx.x, N = k.N, NN = N * N, rec = 1 + N + NN;
  double M = 0.0;   // (every thread: the same loads, the same order)
  for (int r = 0; r < world; ++r) M += recs[(long long)r * rec];
  sig[tid] = 0.0;
  if (tid < N) {
    double s = 0.0;
    for (int r = 0; r < world; ++r) s += recs[(long long)r * rec] * recs[(long long)r * rec + 1 + tid];
    mu[tid] = s / M;
  }
  __syncthreads();
  if (tid < NN) {
    const int n = tid / N, n2 = tid - n * N;
    const double m1 = mu[n], m2 = mu[n2];
    double s = 0.0;
    for (int r = 0; r < world; ++r) {
      const double* R = recs + (long long)r * rec;
      const double d1 = R[1 + n] - m1, d2 = R[1 + n2] - m2;
      s += R[1 + N + tid] + R[0] * (d1 * d2);
    }
    sig[n * kCpMaxN + n2] = s / M;
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    float* tail = k.stats_w + 2 * N + NN + k.D;
    if (tid == 0) tail[0] = (float)M;
    if (tid < NN) {
      const double s = sig[(tid / N) * kCpMaxN + tid % N];
      tail[1 + tid] = (float)(s - (double)(float)s);
    }
  }
  cp_finish_channels(k, mu, sig, M);
}

// A rank's row [k (N), Q (N * N)]: the shares of cpool_bwd_reduce's workgroups, summed in workgroup order as the *_bwd_maps
// kernels sum them.  Those kernels then read the ranks' rows where they read the workgroups' shares.  grid = 1, block = 256.
__global__ void __launch_bounds__(kCpMT) cps_kq_row(CpK k, float* row) { cp_kq_sum<kCpMT>(k, row); }

// What a rank without an image contributes backward: a zero row and zero parameter gradients (those that are asked for).
// grid-stride, block = 256.
__global__ void __launch_bounds__(kCpMT) cps_zero(CpK k, float* row) {
  const long long L = k.N + k.N * k.N, DN = (long long)k.D * k.N, end = L > DN ? L : DN;
  for (long long i = (long long)blockIdx.x * kCpMT + threadIdx.x; i < end; i += (long long)gridDim.x * kCpMT) {
    if (i < L) row[i] = 0.f;
    if (i < DN && k.gw != nullptr) k.gw[i] = 0.f;
    if (i < k.D && k.gg != nullptr) k.gg[i] = 0.f;
    if (i < k.D && k.gb != nullptr) k.gb[i] = 0.f;
  }
}

// ---- lanes along d -----------------------------------------------------------------------------------------------------------
// The two channels of a lane: d0 = tile * 128 + lane and d0 + 64.  ws = s_d w_d (zero beyond D and N), sh the shift.
template <int NP>
__device__ __forceinline__ void cp_rows(const CpK& k, int tile, int lane, float (&ws)[2][NP], float (&sh)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int d = tile * kCpDT + lane + 64 * j;
    float scale = 0.f;
    sh[j] = 0.f;
    if (d < k.D) cp_coef(k, d, scale, sh[j]);
#pragma unroll
    for (int n = 0; n < NP; ++n) ws[j][n] = (d < k.D && n < k.N) ? k.w[(long long)d * k.N + n] * scale : 0.f;
  }
}
// a of the lane's two channels at the four pixels of quad q: the shift first, then the maps in order (cp_bwd_maps forms
// the same chain: the same bits, the same mask)
template <int NP>
__device__ __forceinline__ void cp_preact(const float* sm, int CHs, int q, const float (&ws)[2][NP], const float (&sh)[2],
                                          float (&a)[2][4]) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) a[j][i] = sh[j];
#pragma unroll
  for (int n = 0; n < NP; ++n) {
    const float4 c = ((const float4*)(sm + n * CHs))[q];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      a[j][0] = fmaf(ws[j][n], c.x, a[j][0]);
      a[j][1] = fmaf(ws[j][n], c.y, a[j][1]);
      a[j][2] = fmaf(ws[j][n], c.z, a[j][2]);
      a[j][3] = fmaf(ws[j][n], c.w, a[j][3]);
    }
  }
}

// grid = (B, ceil(D / 128)), block = 512.  LDS: sm[NP * CHs], red[8 * 128].
template <int NP>
__global__ void __launch_bounds__(kCpT) cpool_fwd(CpK k) {
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  float* sm = cp_lds;
  float* red = sm + NP * k.CHs;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x, tile = blockIdx.y;
  float ws[2][NP], sh[2], s[2] = {0.f, 0.f};
  cp_rows<NP>(k, tile, lane, ws, sh);
  for (int p0 = 0; p0 < k.P; p0 += k.CH) {
    const int ch = min(k.CH, k.P - p0), nq = (ch + 3) >> 2;
    if (p0 > 0) __syncthreads();   // (the previous chunk has been read)
    cp_stage(k, NP, sm, b, p0, ch, !k.eval);
    __syncthreads();
    for (int q = wv; q < nq; q += kCpW) {
      float a[2][4];
      cp_preact<NP>(sm, k.CHs, q, ws, sh, a);
      const int nv = min(4, ch - 4 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < nv) {
          s[0] += fmaxf(a[0][i], 0.f);
          s[1] += fmaxf(a[1][i], 0.f);
        }
    }
  }
  red[wv * kCpDT + lane] = s[0];
  red[wv * kCpDT + lane + 64] = s[1];
  __syncthreads();
  const int d = tile * kCpDT + tid;
  if (tid < kCpDT && d < k.D) {
    float t = red[tid];
#pragma unroll
    for (int w = 1; w < kCpW; ++w) t += red[w * kCpDT + tid];
    k.out[(long long)b * k.D + d] = t / (float)k.P;
  }
}

// The threads of the *_bwd_part kernels.  A lane keeps 2 * NP scaled weights and 2 * NP sums: above 24 maps that passes the
// 256 registers two wavefronts per SIMD leave each (92 spilled at 512 threads), so those run four wavefronts, one per
// SIMD, with the whole file.
template <int NP>
constexpr int cp_part_threads() { return NP > 24 ? 256 : kCpT; }

// What cpool_bwd_part and cproj_bwd_part share behind their ga.
// T_dn += ga c_n of the lane's two channels over the four pixels of quad q, the pixels in order
template <int NP>
__device__ __forceinline__ void cp_part_sum(const float* sm, int CHs, int q, const float (&ga)[2][4], float (&T)[2][NP]) {
#pragma unroll
  for (int n = 0; n < NP; ++n) {
    const float4 c = ((const float4*)(sm + n * CHs))[q];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float t = T[j][n];
      t = fmaf(ga[j][0], c.x, t);
      t = fmaf(ga[j][1], c.y, t);
      t = fmaf(ga[j][2], c.z, t);
      t = fmaf(ga[j][3], c.w, t);
      T[j][n] = t;
    }
  }
}
// The wavefronts' sums joined in wavefront order into red[dl][NP + 1] (every lane its own words), then slice sl's rows of
// part_w.  The caller has a barrier behind the last read of what red overlays.
template <int NP>
__device__ __forceinline__ void cp_part_join(const CpK& k, float* red, int sl, int tile, const float (&T)[2][NP],
                                             const float (&gbs)[2]) {
  constexpr int kT = cp_part_threads<NP>(), kW = kT / 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int w = 0; w < kW; ++w) {
    if (wv == w) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float* r = red + (lane + 64 * j) * (NP + 1);
#pragma unroll
        for (int n = 0; n < NP; ++n) r[n] = w == 0 ? T[j][n] : r[n] + T[j][n];
        r[NP] = w == 0 ? gbs[j] : r[NP] + gbs[j];
      }
    }
    __syncthreads();
  }
  const int N1 = k.N + 1;
  for (int i = tid; i < kCpDT * N1; i += kT) {
    const int dl = i / N1, j = i - dl * N1, d = tile * kCpDT + dl;
    if (d < k.D) k.part_w[((long long)sl * k.D + d) * N1 + j] = red[dl * (NP + 1) + (j < k.N ? j : NP)];
  }
}

// grid = (S, ceil(D / 128)), block = cp_part_threads: images [s * ipw, (s + 1) * ipw) of the batch.  LDS: sm[NP * CHs],
// red[128 * (NP + 1)].  part_w: [S][D][N + 1] — T_dn of the slice, then grad_beta_d.
template <int NP>
__global__ void __launch_bounds__(cp_part_threads<NP>()) cpool_bwd_part(CpK k) {
  constexpr int kW = cp_part_threads<NP>() / 64;
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  float* sm = cp_lds;
  float* red = sm + NP * k.CHs;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sl = blockIdx.x, tile = blockIdx.y;
  float ws[2][NP], sh[2], T[2][NP], gbs[2] = {0.f, 0.f};
  cp_rows<NP>(k, tile, lane, ws, sh);
#pragma unroll
  for (int n = 0; n < NP; ++n) T[0][n] = T[1][n] = 0.f;
  const int b1 = min(k.B, (sl + 1) * k.ipw);
  bool first = true;
  for (int b = sl * k.ipw; b < b1; ++b) {
    float gs[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int d = tile * kCpDT + lane + 64 * j;
      gs[j] = d < k.D ? k.go[(long long)b * k.D + d] / (float)k.P : 0.f;
    }
    for (int p0 = 0; p0 < k.P; p0 += k.CH) {
      const int ch = min(k.CH, k.P - p0), nq = (ch + 3) >> 2;
      if (!first) __syncthreads();
      first = false;
      cp_stage(k, NP, sm, b, p0, ch, !k.eval);
      __syncthreads();
      for (int q = wv; q < nq; q += kW) {
        float a[2][4];
        cp_preact<NP>(sm, k.CHs, q, ws, sh, a);
        const int nv = min(4, ch - 4 * q);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            a[j][i] = (i < nv && a[j][i] > 0.f) ? gs[j] : 0.f;   // ga
            gbs[j] += a[j][i];
          }
        cp_part_sum<NP>(sm, k.CHs, q, a, T);
      }
    }
  }
  cp_part_join<NP>(k, red, sl, tile, T, gbs);
}

// What both reduce kernels do once the slices are joined, by 256 threads behind a barrier: Tl[dl * ts + n] holds T_dn of
// the workgroup's 32 channels from d0 = 32 blockIdx.x, with grad_beta_d at n = ts - 1; wl[dl * ws + n] their weights
// (zero beyond D); sg[N * N] Sigma (training).  Per channel inv, s_d, grad_gamma and e, f; then grad_w; then this
// workgroup's share [k (N), Q (N * N)] of kq_w (training).
// SYNC (nfp_cpsync_reduce): e and f divide by the count over all ranks, which cps_finish left behind inv in stats, and
// Sigma w comes from both of Sigma's floats.
template <bool SYNC>
__device__ __forceinline__ void cp_reduce_tail(const CpK& k, const float* Tl, int ts, const float* wl, int ws, const float* sg) {
  __shared__ float el[kCpRT], fl[kCpRT], ggl[kCpRT], c1l[kCpRT], invl[kCpRT];
  const int tid = threadIdx.x, N = k.N, NN = N * N, d0 = blockIdx.x * kCpRT;
  if (tid < kCpRT) {
    const int d = d0 + tid;
    float e = 0.f, f = 0.f, gg = 0.f, c1 = 0.f, inv = 0.f;
    if (d < k.D) {
      inv = k.eval ? 1.f / sqrtf(k.rv[d] + k.eps) : cp_inv(k)[d];
      c1 = k.gamma[d] * inv;
      const float gb = Tl[tid * ts + ts - 1];
      float dot = 0.f;
      for (int n = 0; n < N; ++n) dot = fmaf(wl[tid * ws + n], Tl[tid * ts + n], dot);
      gg = k.eval ? inv * (dot - k.rm[d] * gb) : inv * dot;
      if (!k.eval) {
        const float M = SYNC ? cp_inv(k)[k.D] : (float)k.M;
        e = c1 * (gb / M);
        f = c1 * (gg * inv / M);
      }
      if (k.gg != nullptr) k.gg[d] = gg;
      if (k.gb != nullptr) k.gb[d] = gb;
    }
    el[tid] = e;
    fl[tid] = f;
    ggl[tid] = gg;
    c1l[tid] = c1;
    invl[tid] = inv;
  }
  __syncthreads();
  if (k.gw != nullptr)
    for (int i = tid; i < kCpRT * N; i += kCpMT) {
      const int dl = i / N, n = i - dl * N, d = d0 + dl;
      if (d >= k.D) continue;
      float t = Tl[dl * ts + n];
      if (!k.eval) {
        float sw = 0.f;
        if constexpr (SYNC) {   // Sigma as cps_finish left it, two floats an entry, summed in float64
          const float* lo = cp_inv(k) + k.D + 1;
          double s64 = 0.0;
          for (int n2 = 0; n2 < N; ++n2) s64 += ((double)sg[n * N + n2] + (double)lo[n * N + n2]) * (double)wl[dl * ws + n2];
          sw = (float)s64;
        } else {
          for (int n2 = 0; n2 < N; ++n2) sw = fmaf(sg[n * N + n2], wl[dl * ws + n2], sw);
        }
        t -= ggl[dl] * invl[dl] * sw;
      }
      k.gw[(long long)d * N + n] = c1l[dl] * t;
    }
  if (k.eval || k.kq_w == nullptr) return;
  float* kq = k.kq_w + (long long)blockIdx.x * (N + NN);
  for (int i = tid; i < N + NN; i += kCpMT) {
    float s = 0.f;
    if (i < N) {
      for (int dl = 0; dl < kCpRT; ++dl) s = fmaf(wl[dl * ws + i], el[dl], s);
    } else {
      const int n = (i - N) / N, n2 = (i - N) - n * N;
      for (int dl = 0; dl < kCpRT; ++dl) s = fmaf(fl[dl] * wl[dl * ws + n], wl[dl * ws + n2], s);
    }
    kq[i] = s;
  }
}

// grid = ceil(D / 32), block = 256.  kq_w: per workgroup [k (N), Q (N * N)] of its 32 channels (training).
// LIVE (the cproj backward, whose S reaches 512): loads are issued only from the element rounds and lanes that hold an
// element; the sums and their order are the same in both forms.
// SYNC: the slices are one rank's (cp_reduce_tail).
template <bool LIVE, bool SYNC = false>
__global__ void __launch_bounds__(kCpMT) cpool_bwd_reduce(CpK k) {
  __shared__ float Tl[kCpRT * (kCpMaxN + 1)];
  __shared__ float wl[kCpRT * kCpMaxN];
  __shared__ float sg[kCpMaxN * kCpMaxN];
  const int tid = threadIdx.x, N = k.N, N1 = N + 1, NN = N * N, d0 = blockIdx.x * kCpRT;
  {
    // a thread's elements (at most 5 of the 32 * (N + 1)) side by side, the slices in order: their loads are independent, so
    // several are in flight — one element after the other is a chain of S dependent loads
    constexpr int kE = (kCpRT * (kCpMaxN + 1) + kCpMT - 1) / kCpMT;
    float acc[kE];
    long long off[kE];
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      const int i = tid + e * kCpMT, dl = i / N1, j = i - dl * N1, d = d0 + dl;
      acc[e] = 0.f;
      off[e] = (i < kCpRT * N1 && d < k.D) ? (long long)d * N1 + j : -1;
    }
    const long long stride = (long long)k.D * N1;
    if (!LIVE) {
      for (int sl0 = 0; sl0 < k.S; sl0 += 8) {   // eight slices' loads issued together, added in slice order
        float v[kE][8];
#pragma unroll
        for (int e = 0; e < kE; ++e)
#pragma unroll
          for (int u = 0; u < 8; ++u) v[e][u] = k.part[min(sl0 + u, k.S - 1) * stride + max(off[e], 0LL)];
#pragma unroll
        for (int e = 0; e < kE; ++e)
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (sl0 + u < k.S && off[e] >= 0) acc[e] += v[e][u];
      }
    } else {
      // the same, but only the ne element rounds that hold an element at all (2 of the 5 at N = 8) and only the lanes that
      // hold one issue loads: with hundreds of slices the walk is bound by the loads one CU can issue (measured: 90 us over
      // the 704 slices of cproj_bwd_part at [64,8,26,26] -> 40 with every lane of every round loading)
      const int ne = (kCpRT * N1 + kCpMT - 1) / kCpMT;
      for (int sl0 = 0; sl0 < k.S; sl0 += 8) {
        float v[kE][8];
#pragma unroll
        for (int e = 0; e < kE; ++e)
          if (e < ne) {   // (the same in every thread)
#pragma unroll
            for (int u = 0; u < 8; ++u) v[e][u] = off[e] >= 0 ? k.part[min(sl0 + u, k.S - 1) * stride + off[e]] : 0.f;
          }
#pragma unroll
        for (int e = 0; e < kE; ++e)
          if (e < ne) {
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if (sl0 + u < k.S && off[e] >= 0) acc[e] += v[e][u];
          }
      }
    }
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      const int i = tid + e * kCpMT, dl = i / N1, j = i - dl * N1;
      if (i < kCpRT * N1) Tl[dl * (kCpMaxN + 1) + (j < N ? j : kCpMaxN)] = acc[e];
    }
  }
  for (int i = tid; i < kCpRT * N; i += kCpMT) {
    const int dl = i / N, n = i - dl * N, d = d0 + dl;
    wl[dl * kCpMaxN + n] = d < k.D ? k.w[(long long)d * N + n] : 0.f;
  }
  if (!k.eval)
    for (int i = tid; i < NN; i += kCpMT) sg[i] = k.stats[2 * N + i];
  __syncthreads();
  cp_reduce_tail<SYNC>(k, Tl, kCpMaxN + 1, wl, kCpMaxN, sg);
}

// ---- lanes along p -----------------------------------------------------------------------------------------------------------
// Where the factor t_bdp of channel d at a lane's pixel comes from, in grad_m_bnp = sum_d s_d w_dn t_bdp [a_bdp > 0]:
//   kCpGradPooled  G_bd / P of the pooled tail: divided once per channel when the block's table is filled, and kept in
//                  the channel's row of it
//   kCpGradNchw    the projection's grad_out [b][d][p]: a lane's own loads, four channels' in flight
//   kCpGradNhwc    the projection's grad_out [b][p][d], where a lane's own loads would be D elements apart: the block's
//                  [64 pixels][<= 128 d] tile comes through LDS instead — gt[pl * 129 + dl], written with d fastest across
//                  the lanes (whole segments of global memory, consecutive banks) and read by every lane from its own
//                  pixel's row (an odd stride: 32 banks)
enum CpGrad { kCpGradPooled, kCpGradNchw, kCpGradNhwc };

// grid = B * ceil(P / 64), block = 512: the 64 pixels from pt * 64 of image b.  LDS: red[NP * 64], kql[N + N * N], the table
// of a block of channels tb[128][NP + 4] — a channel's scaled row, then its shift (pooled: then G_bd / P) in 16-byte rows;
// gt for kCpGradNhwc alone.  RELU: the pooled tail always has it.  The sums and their order are the same for every source.
template <int NP, CpGrad SRC, bool RELU>
__global__ void __launch_bounds__(kCpT) cp_bwd_maps(CpK k, int npt) {
  static_assert(RELU || SRC != kCpGradPooled, "the pooled tail has the ReLU");
  constexpr int kTS = NP + 4;
  constexpr int kCS = SRC == kCpGradPooled ? 4 : 1;   // floats between two channels' scales in cf
  constexpr int kU = SRC == kCpGradPooled ? 1 : 4;    // channels of a wavefront whose t is fetched together
  constexpr int kGS = kCpMB + 1;
  __shared__ float red[NP * 64];
  __shared__ float kql[kCpMaxN + kCpMaxN * kCpMaxN];
  __shared__ __attribute__((aligned(16))) float tb[kCpMB * kTS];
  __shared__ float cf[kCpMB * kCS];
  __shared__ float gt[SRC == kCpGradNhwc ? 64 * kGS : 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / npt, pt = blockIdx.x - b * npt, p = pt * 64 + lane, N = k.N;
  const bool live = p < k.P;
  if (!k.eval) cp_kq_sum<kCpT>(k, kql);
  float c[NP], g[NP];
  const long long base = (long long)b * N * k.P + p;
#pragma unroll
  for (int n = 0; n < NP; ++n) {
    c[n] = (n < N && live) ? cp_map(k, n, base + (long long)n * k.P, !k.eval) : 0.f;
    g[n] = 0.f;
  }
  const long long gbase = (long long)b * k.D * k.P + p;
  // D in blocks of 128 channels: the block's rows s_d w_d and shifts go to LDS with coalesced, independent loads first
  // (fetched per channel inside the loop they were a chain of dependent global loads: 0.6 us per channel, measured), then
  // every wavefront walks its channels of the block, dl = wv, wv + 8, ..., reading them as broadcasts
  for (int dB = 0; dB < k.D; dB += kCpMB) {
    const int nd = min(kCpMB, k.D - dB);
    if (dB > 0) __syncthreads();   // (the previous block has been read)
    if constexpr (SRC == kCpGradNhwc) {
      const int lg = nd <= 1 ? 0 : 32 - __clz(nd - 1);   // lanes cover nd rounded up to a power of two
      for (int i = tid; i < 64 << lg; i += kCpT) {
        const int dl = i & ((1 << lg) - 1), pl = i >> lg, pp = pt * 64 + pl;
        if (dl < nd) gt[pl * kGS + dl] = pp < k.P ? cj_load(k, k.gov, ((long long)b * k.P + pp) * k.D + dB + dl) : 0.f;
      }
    }
    if (tid < nd) {
      float scale, shift;
      cp_coef(k, dB + tid, scale, shift);
      cf[tid * kCS] = scale;
      tb[tid * kTS + NP] = shift;
      if constexpr (SRC == kCpGradPooled) tb[tid * kTS + NP + 1] = k.go[(long long)b * k.D + dB + tid] / (float)k.P;
    }
    __syncthreads();
    for (int i = tid; i < nd * NP; i += kCpT) {
      const int dl = i / NP, n = i - dl * NP;
      tb[dl * kTS + n] = n < N ? k.w[(long long)(dB + dl) * N + n] * cf[dl * kCS] : 0.f;
    }
    __syncthreads();
    for (int dl0 = wv; dl0 < nd; dl0 += kU * kCpW) {   // kU channels' t together, used in channel order
      float t[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int dl = dl0 + u * kCpW;
        if constexpr (SRC == kCpGradPooled)
          t[u] = tb[dl * kTS + NP + 1];
        else if constexpr (SRC == kCpGradNhwc)
          t[u] = dl < nd ? gt[lane * kGS + dl] : 0.f;   // (zero beyond P)
        else
          t[u] = (dl < nd && live) ? cj_load(k, k.gov, gbase + (long long)(dB + dl) * k.P) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int dl = dl0 + u * kCpW;
        if (dl >= nd) break;   // (the same in every lane)
        const float* row = tb + dl * kTS;
        float wsn[NP];
#pragma unroll
        for (int n = 0; n < NP; ++n) wsn[n] = row[n];
        float tu = t[u];
        if (RELU) {
          float a = row[NP];   // the shift first, then the maps in order: cp_preact's chain, the same bits, the same mask
#pragma unroll
          for (int n = 0; n < NP; ++n) a = fmaf(wsn[n], c[n], a);
          tu = a > 0.f ? tu : 0.f;
        }
#pragma unroll
        for (int n = 0; n < NP; ++n) g[n] = fmaf(wsn[n], tu, g[n]);
      }
    }
  }
  for (int w = 0; w < kCpW; ++w) {   // the eight wavefronts in order
    if (wv == w) {
#pragma unroll
      for (int n = 0; n < NP; ++n) red[n * 64 + lane] = w == 0 ? g[n] : red[n * 64 + lane] + g[n];
    }
    __syncthreads();
  }
  if (!live) return;
  for (int n = wv; n < N; n += kCpW) {
    float v = red[n * 64 + lane];
    if (!k.eval) {
      float qc = kql[n];
#pragma unroll
      for (int n2 = 0; n2 < NP; ++n2)
        if (n2 < N) qc = fmaf(kql[N + n * N + n2], c[n2], qc);
      v -= qc;
    }
    cj_store(k, k.gm, base + (long long)n * k.P, v);
  }
}

// ---- cproj: the projection with the map kept ------------------------------------------------------------------------------
constexpr int kCjT = 256;    // threads of cproj_fwd
constexpr int kCjDT = 64;    // channels of D per workgroup of cproj_fwd
constexpr int kCjSP = 64;    // pixels per pass of cproj_bwd_part
constexpr int kCjSS = 68;    // floats between two rows of a pass in LDS: 16-byte rows, an odd number of 16-byte slots

// out of one channel at pixel pl of the staged maps sm (rows CHs apart): row = the channel's scaled weights, then its shift.
// The shift first, then the maps in order: cp_preact's chain.
template <int NP, bool RELU>
__device__ __forceinline__ float cj_act(const float* row, const float* sm, int CHs, int pl) {
  float a = row[NP];
#pragma unroll
  for (int n = 0; n < NP; ++n) a = fmaf(row[n], sm[n * CHs + pl], a);
  if (RELU) a = a < 0.f ? 0.f : a;
  return a;
}

// grid = B * nc * tiles (the tile fastest), block = 256; k.CH / k.CHs / k.nc are this kernel's own chunks (cproj_fwd_chunk).
// LDS: sm[NP * CHs], tb[64][NP + 1] — the scaled row of a channel, then its shift.
// The tile's share of the chunk is a [slow][fast] range that lanes walk flat, element e = slow * fast-extent + fast, a
// thread's next one 256 further on.  NCHW out, [b][d][p]: [nd][ch], the pixel fastest, at obase + dl * P + pl.
// NHWC out, [b][p][d]: [ch][nd], the channel fastest, at obase + pl * D + dl — so where the tile is all of D the chunk is
// one span of ch * D elements, and otherwise ch segments of nd channels; a wavefront's store covers whole segments
// (several pixels where D is small), the rows of tb are read at an odd stride and the maps as broadcasts.
// Prologue, chain (cj_act) and store are shared; each layout keeps its own walk, and hands cj_act the maps the way its
// loop always has (NCHW: the pixel's column; NHWC: the maps and the pixel).  As one walk over a fast extent of ch or nd
// the NCHW eval forward measured 0.2 us (1 %) over its time at [64,8,54,54] -> 24 and [64,8,5,5] -> 160.
// PAIR (NHWC only: bf16, out 4-byte aligned, and a single tile or an even D): a lane holds the two elements of an aligned
// dword and stores them together.  With a single tile the pairs are laid over the span from its even address down (s: the
// span starts on an odd element), so they may straddle two pixels' rows and the span's first and last element may stand
// alone; with an even D every segment starts and ends on a pair.
template <int NP, bool RELU, bool NHWC, bool PAIR = false>
__global__ void __launch_bounds__(kCjT) cproj_fwd(CpK k, int tiles) {
  static_assert(NHWC || !PAIR, "pairs are laid along d");
  constexpr int kTS = NP + 1;
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  float* sm = cp_lds;
  float* tb = sm + NP * k.CHs;
  const int tid = threadIdx.x;
  const int bj = blockIdx.x / tiles, tile = blockIdx.x - bj * tiles;
  const int b = bj / k.nc, j = bj - b * k.nc;
  const int p0 = j * k.CH, ch = min(k.CH, k.P - p0);
  const int d0 = tile * kCjDT, nd = min(kCjDT, k.D - d0);
  cp_stage(k, NP, sm, b, p0, ch, !k.eval);
  for (int i = tid; i < nd * kTS; i += kCjT) {
    const int dl = i / kTS, n = i - dl * kTS;
    float scale, shift;
    cp_coef(k, d0 + dl, scale, shift);
    tb[i] = n == NP ? shift : (n < k.N ? k.w[(long long)(d0 + dl) * k.N + n] * scale : 0.f);
  }
  __syncthreads();
  const int CHs = k.CHs;
  auto act = [&](int pl, int dl) { return cj_act<NP, RELU>(tb + dl * kTS, sm, CHs, pl); };
  const int total = nd * ch;
  if constexpr (!NHWC) {
    const int qT = kCjT / ch, rT = kCjT - qT * ch;
    int dl = tid / ch, pl = tid - dl * ch;
    const long long obase = ((long long)b * k.D + d0) * k.P + p0;
    for (int e = tid; e < total; e += kCjT) {
      const float a = cj_act<NP, RELU>(tb + dl * kTS, sm + pl, k.CHs, 0);
      cj_store(k, k.outv, obase + (long long)dl * k.P + pl, a);
      pl += rT, dl += qT;
      if (pl >= ch) pl -= ch, ++dl;
    }
    return;
  }
  const long long obase = ((long long)b * k.P + p0) * k.D + d0;
  if (!PAIR) {
    const int qT = kCjT / nd, rT = kCjT - qT * nd;
    int pl = tid / nd, dl = tid - pl * nd;
    for (int e = tid; e < total; e += kCjT) {
      const float a = act(pl, dl);
      cj_store(k, k.outv, obase + (long long)pl * k.D + dl, a);
      dl += rT, pl += qT;
      if (dl >= nd) dl -= nd, ++pl;
    }
  } else {
    const int s = tiles == 1 ? (int)(obase & 1) : 0;
    const int qT = 2 * kCjT / nd, rT = 2 * kCjT - qT * nd;   // a thread's next pair is 512 elements further on
    int e0 = 2 * tid - s, pl = -1, dl = nd - 1;              // (e0 = -1: the element before the span)
    if (e0 >= 0) pl = e0 / nd, dl = e0 - pl * nd;
    for (; e0 < total; e0 += 2 * kCjT) {
      int pl1 = pl, dl1 = dl + 1;
      if (dl1 == nd) dl1 = 0, ++pl1;
      const bool v0 = e0 >= 0, v1 = e0 + 1 < total;
      const float a0 = v0 ? act(pl, dl) : 0.f, a1 = v1 ? act(pl1, dl1) : 0.f;
      uint16_t* o = (uint16_t*)k.outv + (obase + (long long)pl * k.D + dl);
      if (v0 && v1)
        *(uint32_t*)o = f32_to_bf16x2(a0, a1);
      else if (v0)
        o[0] = f32_to_bf16(a0);
      else
        o[1] = f32_to_bf16(a1);
      dl += rT, pl += qT;
      if (dl >= nd) dl -= nd, ++pl;
    }
  }
}

// grid = (S, ceil(D / 128)), block = cp_part_threads: passes [s * upw, (s + 1) * upw) of the batch's B * nsub passes of 64
// pixels.  LDS: sm[NP * 68], gl[128 * 68] (grad_out of the pass; at the end the join buffer red[128 * (NP + 1)]).
// part_w: [S][D][N + 1], as cpool_bwd_part.
// NHWC: grad_out is [b][p][d].  The tile goes into the same gl[dl * 68 + pl], read from global memory with d fastest: a
// lane takes one channel at four neighbouring pixels — four loads that each run along d across the wavefront — and
// stores them as one 16-byte row piece.  ds_write_b128 is served eight lanes at a time; eight neighbouring channels are
// 8 * 68 floats apart, banks 4 * dl + {0..3} (mod 32): all 32 different.  (One pixel per lane, a dword each, puts the 32
// lanes of a half on eight banks.)  Lanes cover the nd channels of the tile rounded up to a power of two, 8 at the
// least; the rows beyond that are zeroed once.  Everything behind the staging is the same code for both layouts.
template <int NP, bool RELU, bool NHWC = false>
__global__ void __launch_bounds__(cp_part_threads<NP>()) cproj_bwd_part(CpK k, int nsub, int upw) {
  constexpr int kT = cp_part_threads<NP>(), kW = kT / 64;
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  float* sm = cp_lds;
  float* gl = sm + NP * kCjSS;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sl = blockIdx.x, tile = blockIdx.y;
  float ws[2][NP], sh[2], T[2][NP], gbs[2] = {0.f, 0.f};
  if (RELU) cp_rows<NP>(k, tile, lane, ws, sh);
#pragma unroll
  for (int n = 0; n < NP; ++n) T[0][n] = T[1][n] = 0.f;
  const int units = k.B * nsub, u0 = sl * upw, u1 = min(units, u0 + upw);
  for (int u = u0; u < u1; ++u) {
    const int b = u / nsub, ps = (u - b * nsub) * kCjSP, npx = min(kCjSP, k.P - ps);
    if (u > u0) __syncthreads();   // (the previous pass has been read)
    cp_stage(k, NP, sm, b, ps, npx, !k.eval);
    if constexpr (NHWC) {
      const int nd = min(kCpDT, k.D - tile * kCpDT), lg = nd <= 8 ? 3 : 32 - __clz(nd - 1);
      if (u == u0)
        for (int i = (kCjSS << lg) + tid; i < kCpDT * kCjSS; i += kT) gl[i] = 0.f;
      for (int i = tid; i < (kCjSP / 4) << lg; i += kT) {
        const int dl = i & ((1 << lg) - 1), q = i >> lg, d = tile * kCpDT + dl;
        const long long g0 = ((long long)b * k.P + ps + 4 * q) * k.D + d;
        float4 v;
        v.x = (d < k.D && 4 * q < npx) ? cj_load(k, k.gov, g0) : 0.f;
        v.y = (d < k.D && 4 * q + 1 < npx) ? cj_load(k, k.gov, g0 + k.D) : 0.f;
        v.z = (d < k.D && 4 * q + 2 < npx) ? cj_load(k, k.gov, g0 + 2LL * k.D) : 0.f;
        v.w = (d < k.D && 4 * q + 3 < npx) ? cj_load(k, k.gov, g0 + 3LL * k.D) : 0.f;
        *(float4*)(gl + dl * kCjSS + 4 * q) = v;
      }
    } else {
      for (int i = tid; i < kCpDT * kCjSP; i += kT) {
        const int dl = i >> 6, pl = i & 63, d = tile * kCpDT + dl;
        float v = 0.f;
        if (d < k.D && pl < npx) v = cj_load(k, k.gov, ((long long)b * k.D + d) * k.P + ps + pl);
        gl[dl * kCjSS + pl] = v;
      }
    }
    __syncthreads();
    const int nq = (npx + 3) >> 2;
    for (int q = wv; q < nq; q += kW) {
      float ga[2][4];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float4 g4 = ((const float4*)(gl + (lane + 64 * j) * kCjSS))[q];   // (zero beyond npx and D)
        ga[j][0] = g4.x, ga[j][1] = g4.y, ga[j][2] = g4.z, ga[j][3] = g4.w;
      }
      if (RELU) {
        float a[2][4];
        cp_preact<NP>(sm, kCjSS, q, ws, sh, a);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) ga[j][i] = a[j][i] > 0.f ? ga[j][i] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) gbs[j] += ga[j][i];
      cp_part_sum<NP>(sm, kCjSS, q, ga, T);
    }
  }
  __syncthreads();   // (gl has been read: red takes its place)
  cp_part_join<NP>(k, gl, sl, tile, T, gbs);
}

// ---- the wide form: 1 <= N <= 96 maps (nfp_cpool_wide_*) --------------------------------------------------------------------
// The kernels above keep a lane's weight rows, its T sums or a pixel's c_n in registers: a cost that grows with N and ends at
// 32 maps.  Here the rows of a block of 64 channels and the chunk's centred maps both sit in LDS, and a lane owns a small
// tile of outputs: nothing in registers grows with N beyond N' / 16 <= 6 accumulators per owned row (N' = N rounded up to 16).
// The formulas, the saved state (2N + N^2 + D floats) and the layouts of the partial sums are the ones above.
//   cpw_moments     cpool_moments' anchor and centring passes (cp_anchor_centre), then the Gram as 4 x 4 register tiles of
//                   (n, n2) pairs, each pair's sum in pixel order
//   cpw_mu          one workgroup: mu in float64 from the chunks' anchors (eight slices of consecutive chunks, in order)
//   cpw_sigma       one workgroup per 64 (n, n2) pairs: cpool_finish's join of the chunks in float64, four slices in order
//   cpw_var         one workgroup per 16 channels: w_d^T Sigma w_d in float64, the rows of Sigma dealt to sixteen slices
//                   joined in order; inv_d and the running statistics
//   cpw_fwd         one workgroup per (image, 64 channels): a lane owns 4 channels x 4 pixels of pre-activations, summed
//                   over n from two ds_read_b128 (the rows transposed, tb[n][d]; the maps sm[n][p]); the sixteen pixel
//                   slots joined in order
//   cpw_bwd_part    the same pre-activations over a slice of the batch, ga written to LDS as [p][d]; then T_dn as a second
//                   product, a lane owning 4 channels x N'/16 maps, summed over the pixels in order (no join)
//   cpw_bwd_reduce  the slices joined into tables sized by N, then cpool_bwd_reduce's tail (cp_reduce_tail)
//   cpw_bwd_maps    one workgroup per 64 pixels of an image: per block of 64 channels the pre-activations as in cpw_fwd, the
//                   masked G_bd / P to LDS as [d][p]; then sum_d s_d w_dn ga_dp, a lane owning 4 pixels x N'/16 maps, summed
//                   over d in order; then - k - Q c from LDS
// Every a_bdp is one chain — the shift, then the maps in order (cw_preact) — in all three kernels: the same bits, the same mask.
constexpr int kWT = 256;          // threads of every wide kernel but cpw_mu
constexpr int kWDT = 64;          // channels of D per workgroup / per LDS block
constexpr int kWRS = kWDT + 4;    // floats between two maps' rows of the transposed table: 16-byte rows, an odd number of slots
constexpr int kWMaxN = 96;
constexpr int kWJ = kWMaxN / 16;  // maps per lane of the second products
constexpr int kWBudget = 16384;   // floats of LDS the chunk's maps and ga may take together (cpw_chunk)
constexpr int kWMuT = 1024;       // threads of cpw_mu

// tb[n * 68 + dl] = s_d w_dn and sh[dl] of the 64 channels from d0 (zero beyond D and N); cf: 64 floats of scratch.
// The caller has a barrier before (tb is free) and after.
__device__ __forceinline__ void cw_rows(const CpK& k, int NP, int d0, float* tb, float* sh, float* cf) {
  const int tid = threadIdx.x;
  if (tid < kWDT) {
    float scale = 0.f, shift = 0.f;
    if (d0 + tid < k.D) cp_coef(k, d0 + tid, scale, shift);
    cf[tid] = scale;
    sh[tid] = shift;
  }
  __syncthreads();
  for (int i = tid; i < kWDT * NP; i += kWT) {
    const int dl = i / NP, n = i - dl * NP, d = d0 + dl;
    tb[n * kWRS + dl] = (d < k.D && n < k.N) ? k.w[(long long)d * k.N + n] * cf[dl] : 0.f;
  }
}

// a of channels 4 dg .. 4 dg + 3 at the pixels 4 q .. 4 q + 3 of sm (rows rs floats apart): the shift first, then the maps
// in order
__device__ __forceinline__ void cw_preact(const float* tb, const float* sh, const float* sm, int rs, int NP, int dg, int q,
                                          float (&a)[4][4]) {
  const float4 s4 = *(const float4*)(sh + 4 * dg);
#pragma unroll
  for (int j = 0; j < 4; ++j) a[0][j] = s4.x, a[1][j] = s4.y, a[2][j] = s4.z, a[3][j] = s4.w;
  const float* tp = tb + 4 * dg;
  const float* cp = sm + 4 * q;
#pragma unroll 4
  for (int n = 0; n < NP; ++n) {
    const float4 w = *(const float4*)(tp + n * kWRS);
    const float4 c = *(const float4*)(cp + n * rs);
    const float wv[4] = {w.x, w.y, w.z, w.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[i][j] = fmaf(wv[i], cv[j], a[i][j]);
  }
}

// grid = B * nc chunks, block = 256.  LDS: sm[NP * CHs], anchor[NP].  part_w: per chunk [a (N), r (N), Gram (N * N)].
__global__ void __launch_bounds__(kWT) cpw_moments(CpK k, int NP) {
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  float* sm = cp_lds;
  float* anchor = sm + NP * k.CHs;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / k.nc, j = blockIdx.x - b * k.nc;
  const int p0 = j * k.CH, ch = min(k.CH, k.P - p0);
  const int N = k.N;
  float* outp = k.part_w + (long long)blockIdx.x * (2 * N + N * N);
  cp_stage(k, NP, sm, b, p0, ch, false);
  __syncthreads();
  cp_anchor_centre(k, sm, anchor, ch, outp);
  const int nq = (ch + 3) >> 2, NT = NP >> 2;
  for (int t = tid; t < NT * NT; t += kWT) {
    const int tn = t / NT, tm = t - tn * NT;
    const float4* ra = (const float4*)(sm + 4 * tn * k.CHs);
    const float4* rb = (const float4*)(sm + 4 * tm * k.CHs);
    const int qs = k.CHs >> 2;
    float g[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) g[i][jj] = 0.f;
    for (int q = 0; q < nq; ++q) {
      float4 x[4], y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = ra[i * qs + q], y[i] = rb[i * qs + q];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          float v = g[i][jj];
          v = fmaf(x[i].x, y[jj].x, v);
          v = fmaf(x[i].y, y[jj].y, v);
          v = fmaf(x[i].z, y[jj].z, v);
          v = fmaf(x[i].w, y[jj].w, v);
          g[i][jj] = v;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int n = 4 * tn + i, n2 = 4 * tm + jj;
        if (n < N && n2 < N) outp[2 * N + n * N + n2] = g[i][jj];
      }
  }
}

// pixels of chunk c (chunk j of its image)
__device__ __forceinline__ double cw_count(const CpK& k, int j) {
  return j == k.nc - 1 ? (double)(k.P - (k.nc - 1) * k.CH) : (double)k.CH;
}

// grid = 1, block = 1024: thread (n = tid % 128, slice = tid / 128).  mu64: N doubles.
__global__ void __launch_bounds__(kWMuT) cpw_mu(CpK k, double* mu64) {
  __shared__ double red[kWMuT];
  const int tid = threadIdx.x, N = k.N, K = k.B * k.nc, rec = 2 * N + N * N;
  const int n = tid & 127, sl = tid >> 7, Kc = (K + 7) / 8;
  const int c0 = min(K, sl * Kc), c1 = min(K, c0 + Kc);
  double s = 0.0;
  if (n < N) {
    int j = c0 % k.nc;
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
      const float* r = k.part + (long long)c * rec;
      s += cw_count(k, j) * ((double)r[n] + (double)r[N + n]);
      if (++j == k.nc) j = 0;
    }
  }
  red[tid] = s;
  __syncthreads();
  if (tid < N) {
    double t = red[tid];
    for (int i = 1; i < 8; ++i) t += red[i * 128 + tid];
    t /= k.M;
    mu64[tid] = t;
    const float hi = (float)t;
    k.stats_w[tid] = hi;
    k.stats_w[N + tid] = (float)(t - (double)hi);
  }
}

// grid = ceil(N^2 / 64), block = 256: thread (pair = 64 blockIdx + tid % 64, slice = tid / 64).  sig64: N * N doubles.
__global__ void __launch_bounds__(kWT) cpw_sigma(CpK k, const double* mu64, double* sig64) {
  __shared__ double red[kWT];
  const int tid = threadIdx.x, N = k.N, NN = N * N, K = k.B * k.nc, rec = 2 * N + NN;
  const int pl = tid & 63, sl = tid >> 6, pr = blockIdx.x * 64 + pl, Kc = (K + 3) / 4;
  double s = 0.0;
  if (pr < NN) {
    const int n = pr / N, n2 = pr - n * N;
    const int c0 = min(K, sl * Kc), c1 = min(K, c0 + Kc);
    const double m1 = mu64[n], m2 = mu64[n2];
    int j = c0 % k.nc;
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
      const float* r = k.part + (long long)c * rec;
      const double d1 = (double)r[n] - m1, d2 = (double)r[n2] - m2, r1 = r[N + n], r2 = r[N + n2];
      s += (double)r[2 * N + pr] + cw_count(k, j) * (r1 * d2 + d1 * r2 + d1 * d2);
      if (++j == k.nc) j = 0;
    }
  }
  red[tid] = s;
  __syncthreads();
  if (tid < 64 && pr < NN) {
    const double t = (((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid]) / k.M;
    sig64[pr] = t;
    k.stats_w[2 * N + pr] = (float)t;
  }
}

// grid = ceil(D / 16), block = 256: thread (channel = 16 blockIdx + tid % 16, slice = tid / 16) takes the rows
// n = slice, slice + 16, ... of Sigma.
__global__ void __launch_bounds__(kWT) cpw_var(CpK k, const double* mu64, const double* sig64) {
  __shared__ double wl[kWMaxN * 16];   // [n][dl]
  __shared__ double red[kWT];
  const int tid = threadIdx.x, N = k.N, dl = tid & 15, sl = tid >> 4, d0 = blockIdx.x * 16;
  for (int i = tid; i < 16 * N; i += kWT) {
    const int dd = i / N, n = i - dd * N;
    wl[n * 16 + dd] = d0 + dd < k.D ? (double)k.w[(long long)(d0 + dd) * N + n] : 0.0;
  }
  __syncthreads();
  double acc = 0.0;
  for (int n = sl; n < N; n += 16) {
    const double* row = sig64 + n * N;
    double v = 0.0;
#pragma unroll 4
    for (int n2 = 0; n2 < N; ++n2) v += row[n2] * wl[n2 * 16 + dl];
    acc += wl[n * 16 + dl] * v;
  }
  red[tid] = acc;
  __syncthreads();
  const int d = d0 + tid;
  if (tid >= 16 || d >= k.D) return;
  double var = red[tid], mean = 0.0;
  for (int i = 1; i < 16; ++i) var += red[i * 16 + tid];
  for (int n = 0; n < N; ++n) mean += wl[n * 16 + tid] * mu64[n];
  var = var > 0.0 ? var : 0.0;
  k.stats_w[2 * N + N * N + d] = (float)(1.0 / sqrt(var + k.eps64));
  if (k.rm_w != nullptr) {
    k.rm_w[d] = (float)((1.0 - k.mom) * (double)k.rm_w[d] + k.mom * mean);
    k.rv_w[d] = (float)((1.0 - k.mom) * (double)k.rv_w[d] + k.mom * var * (k.M / (k.M - 1.0)));
  }
}

// grid = (B, ceil(D / 64)), block = 256: thread (dg = tid % 16: four channels, qs = tid / 16: a slot of pixel quads).
// LDS: tb[NP * 68], sh[64], cf[64], sm[NP * CHs], red[16 * 64].
__global__ void __launch_bounds__(kWT) cpw_fwd(CpK k, int NP) {
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  float* tb = cp_lds;
  float* sh = tb + NP * kWRS;
  float* cf = sh + kWDT;
  float* sm = cf + kWDT;
  float* red = sm + NP * k.CHs;
  const int tid = threadIdx.x, dg = tid & 15, qs = tid >> 4;
  const int b = blockIdx.x, d0 = blockIdx.y * kWDT;
  cw_rows(k, NP, d0, tb, sh, cf);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int p0 = 0; p0 < k.P; p0 += k.CH) {
    const int ch = min(k.CH, k.P - p0), nq = (ch + 3) >> 2;
    if (p0 > 0) __syncthreads();   // (the previous chunk has been read)
    cp_stage(k, NP, sm, b, p0, ch, !k.eval);
    __syncthreads();
    for (int q = qs; q < nq; q += 16) {
      float a[4][4];
      cw_preact(tb, sh, sm, k.CHs, NP, dg, q, a);
      const int nv = min(4, ch - 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) {
#pragma unroll
          for (int i = 0; i < 4; ++i) s[i] += fmaxf(a[i][j], 0.f);
        }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[qs * kWDT + 4 * dg + i] = s[i];
  __syncthreads();
  const int d = d0 + tid;
  if (tid < kWDT && d < k.D) {
    float t = red[tid];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += red[w * kWDT + tid];
    k.out[(long long)b * k.D + d] = t / (float)k.P;
  }
}

// grid = (S, ceil(D / 64)), block = 256: images [s * ipw, (s + 1) * ipw) of the batch.  Thread (dg, qs) as in cpw_fwd for
// the pre-activations; (dg: four channels, ns = tid / 16: the maps ns, ns + 16, ...) for T.
// LDS: tb[NP * 68], sh[64], cf[64], gp[64] (G_bd / P of the image), sm[NP * CHs], ga[CHs * 68] ([p][d]).
// part_w: [S][D][N + 1] — T_dn of the slice, then grad_beta_d.
__global__ void __launch_bounds__(kWT) cpw_bwd_part(CpK k, int NP) {
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  float* tb = cp_lds;
  float* sh = tb + NP * kWRS;
  float* cf = sh + kWDT;
  float* gp = cf + kWDT;
  float* sm = gp + kWDT;
  float* ga = sm + NP * k.CHs;
  const int tid = threadIdx.x, dg = tid & 15, qs = tid >> 4, ns = qs, nj = NP >> 4;
  const int sl = blockIdx.x, d0 = blockIdx.y * kWDT;
  cw_rows(k, NP, d0, tb, sh, cf);
  float T[4][kWJ], gbs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < kWJ; ++j) T[i][j] = 0.f;
  const int b1 = min(k.B, (sl + 1) * k.ipw);
  for (int b = sl * k.ipw; b < b1; ++b) {
    // (every thread is behind the barrier that follows the last read of gp)
    if (tid < kWDT) gp[tid] = d0 + tid < k.D ? k.go[(long long)b * k.D + d0 + tid] / (float)k.P : 0.f;
    for (int p0 = 0; p0 < k.P; p0 += k.CH) {
      const int ch = min(k.CH, k.P - p0), nq = (ch + 3) >> 2;
      __syncthreads();   // (the previous chunk's sm and ga have been read; the first time: tb is written)
      cp_stage(k, NP, sm, b, p0, ch, !k.eval);
      __syncthreads();
      const float4 g4 = *(const float4*)(gp + 4 * dg);
      for (int q = qs; q < nq; q += 16) {
        float a[4][4];
        cw_preact(tb, sh, sm, k.CHs, NP, dg, q, a);
        const int nv = min(4, ch - 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float4 v;
          v.x = (j < nv && a[0][j] > 0.f) ? g4.x : 0.f;
          v.y = (j < nv && a[1][j] > 0.f) ? g4.y : 0.f;
          v.z = (j < nv && a[2][j] > 0.f) ? g4.z : 0.f;
          v.w = (j < nv && a[3][j] > 0.f) ? g4.w : 0.f;
          *(float4*)(ga + (4 * q + j) * kWRS + 4 * dg) = v;
        }
      }
      __syncthreads();
      for (int q = 0; q < nq; ++q) {
        float4 gv[4], cv[kWJ];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) gv[jj] = *(const float4*)(ga + (4 * q + jj) * kWRS + 4 * dg);
#pragma unroll
        for (int j = 0; j < kWJ; ++j)
          if (j < nj) cv[j] = *(const float4*)(sm + (ns + 16 * j) * k.CHs + 4 * q);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float g[4] = {gv[jj].x, gv[jj].y, gv[jj].z, gv[jj].w};
          if (ns == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) gbs[i] += g[i];
          }
#pragma unroll
          for (int j = 0; j < kWJ; ++j)
            if (j < nj) {
              const float c = jj == 0 ? cv[j].x : jj == 1 ? cv[j].y : jj == 2 ? cv[j].z : cv[j].w;
#pragma unroll
              for (int i = 0; i < 4; ++i) T[i][j] = fmaf(g[i], c, T[i][j]);
            }
        }
      }
    }
  }
  const int N1 = k.N + 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = d0 + 4 * dg + i;
    if (d >= k.D) continue;
    float* row = k.part_w + ((long long)sl * k.D + d) * N1;
#pragma unroll
    for (int j = 0; j < kWJ; ++j)
      if (j < nj && ns + 16 * j < k.N) row[ns + 16 * j] = T[i][j];
    if (ns == 0) row[k.N] = gbs[i];
  }
}

// grid = ceil(D / 32), block = 256.  LDS: Tl[32 * (N + 1)], wl[32 * N], sg[N * N].
// kq_w: per workgroup [k (N), Q (N * N)] of its 32 channels (training).
static_assert(kWT == kCpMT, "cp_reduce_tail and cp_anchor_centre walk with 256 threads");
__global__ void __launch_bounds__(kWT) cpw_bwd_reduce(CpK k) {
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  const int tid = threadIdx.x, N = k.N, N1 = N + 1, NN = N * N, d0 = blockIdx.x * kCpRT;
  float* Tl = cp_lds;
  float* wl = Tl + kCpRT * N1;
  float* sg = wl + kCpRT * N;
  const long long stride = (long long)k.D * N1;
  for (int i = tid; i < kCpRT * N1; i += kWT) {
    const int dl = i / N1;
    float acc = 0.f;
    if (d0 + dl < k.D) {
      const float* src = k.part + (long long)d0 * N1 + i;
      for (int sl0 = 0; sl0 < k.S; sl0 += 8) {   // eight slices' loads issued together, added in slice order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[min(sl0 + u, k.S - 1) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (sl0 + u < k.S) acc += v[u];
      }
    }
    Tl[i] = acc;
  }
  for (int i = tid; i < kCpRT * N; i += kWT) {
    const int dl = i / N;
    wl[i] = d0 + dl < k.D ? k.w[(long long)d0 * N + i] : 0.f;
  }
  if (!k.eval)
    for (int i = tid; i < NN; i += kWT) sg[i] = k.stats[2 * N + i];
  __syncthreads();
  cp_reduce_tail<false>(k, Tl, N1, wl, N, sg);
}

// grid = B * ceil(P / 64), block = 256: the 64 pixels from pt * 64 of image b.  Thread (dg = tid % 16, q = tid / 16) for
// the pre-activations of a block of 64 channels; (pq = tid % 16: four pixels, ns = tid / 16: the maps ns, ns + 16, ...) for
// the sums over d.
// LDS: cl[NP * 68] (c_n of the pixels), sh[64], cf[64], gp[64], tb[NP * 68], tt[64 * 68] (the masked G_bd / P, [d][p]);
// after the last block tb and tt together hold k and Q (N + N * N <= 68 N' + 4352 up to 107 maps).
__global__ void __launch_bounds__(kWT) cpw_bwd_maps(CpK k, int NP, int npt) {
  extern __shared__ __attribute__((aligned(16))) float cp_lds[];
  float* cl = cp_lds;
  float* sh = cl + NP * kWRS;
  float* cf = sh + kWDT;
  float* gp = cf + kWDT;
  float* tb = gp + kWDT;
  float* tt = tb + NP * kWRS;
  float* kql = tb;
  const int tid = threadIdx.x, dg = tid & 15, q = tid >> 4, pq = dg, ns = q, nj = NP >> 4;
  const int b = blockIdx.x / npt, pt = blockIdx.x - b * npt, p0 = pt * 64, N = k.N;
  const int npx = min(64, k.P - p0);
  const long long base = (long long)b * N * k.P + p0;
  for (int i = tid; i < NP * 64; i += kWT) {
    const int n = i >> 6, pl = i & 63;
    cl[n * kWRS + pl] = (n < N && pl < npx) ? cp_map(k, n, base + (long long)n * k.P + pl, !k.eval) : 0.f;
  }
  float g[4][kWJ];   // [pixel][map]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < kWJ; ++j) g[i][j] = 0.f;
  for (int dB = 0; dB < k.D; dB += kWDT) {
    __syncthreads();   // (the previous block has been read; the first time: cl is written)
    if (tid < kWDT) gp[tid] = dB + tid < k.D ? k.go[(long long)b * k.D + dB + tid] / (float)k.P : 0.f;
    cw_rows(k, NP, dB, tb, sh, cf);
    __syncthreads();
    {
      float a[4][4];
      cw_preact(tb, sh, cl, kWRS, NP, dg, q, a);
      const float4 g4 = *(const float4*)(gp + 4 * dg);
      const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float4 v;
        v.x = a[i][0] > 0.f ? gv[i] : 0.f;
        v.y = a[i][1] > 0.f ? gv[i] : 0.f;
        v.z = a[i][2] > 0.f ? gv[i] : 0.f;
        v.w = a[i][3] > 0.f ? gv[i] : 0.f;
        *(float4*)(tt + (4 * dg + i) * kWRS + 4 * q) = v;
      }
    }
    __syncthreads();
    for (int d4 = 0; d4 < kWDT; d4 += 4) {
      float4 tv[4], wv[kWJ];
#pragma unroll
      for (int i = 0; i < 4; ++i) tv[i] = *(const float4*)(tt + (d4 + i) * kWRS + 4 * pq);
#pragma unroll
      for (int j = 0; j < kWJ; ++j)
        if (j < nj) wv[j] = *(const float4*)(tb + (ns + 16 * j) * kWRS + d4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t[4] = {tv[i].x, tv[i].y, tv[i].z, tv[i].w};
#pragma unroll
        for (int j = 0; j < kWJ; ++j)
          if (j < nj) {
            const float w = i == 0 ? wv[j].x : i == 1 ? wv[j].y : i == 2 ? wv[j].z : wv[j].w;
#pragma unroll
            for (int px = 0; px < 4; ++px) g[px][j] = fmaf(w, t[px], g[px][j]);
          }
      }
    }
  }
  if (!k.eval) {
    __syncthreads();   // (tb and tt have been read: k and Q take their place)
    cp_kq_sum<kWT>(k, kql);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < kWJ; ++j) {
    const int n = ns + 16 * j;
    if (j >= nj || n >= N) continue;
    float v[4] = {g[0][j], g[1][j], g[2][j], g[3][j]};
    if (!k.eval) {
      float qc[4] = {kql[n], kql[n], kql[n], kql[n]};
      for (int n2 = 0; n2 < N; ++n2) {
        const float qv = kql[N + n * N + n2];
        const float4 c = *(const float4*)(cl + n2 * kWRS + 4 * pq);
        qc[0] = fmaf(qv, c.x, qc[0]);
        qc[1] = fmaf(qv, c.y, qc[1]);
        qc[2] = fmaf(qv, c.z, qc[2]);
        qc[3] = fmaf(qv, c.w, qc[3]);
      }
#pragma unroll
      for (int px = 0; px < 4; ++px) v[px] -= qc[px];
    }
#pragma unroll
    for (int px = 0; px < 4; ++px) {
      if (4 * pq + px >= npx) continue;
      cj_store(k, k.gm, base + (long long)n * k.P + 4 * pq + px, v[px]);
    }
  }
}

}  // namespace
}  // namespace nfp
