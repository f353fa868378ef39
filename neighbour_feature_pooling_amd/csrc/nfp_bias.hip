// nfp_bias.hip — NFPPooling(bias=True): the two depthwise convs of the reference carry TRAINABLE biases
// (nfp.py:42-58; only their weights are frozen, nfp.py:61,82), for every measure but SCS and every nn.Conv2d geometry.
//
// The conv adds its bias after padding, so every pair (output o, neighbour n) of channel c sees
//   a = x[c][centre(o)] + bc[c]                                    (centre_value, nfp.py:54-61)
//   v = (diff ? x[c][centre(o)] - x[c][q(o,n)] : x[c][q(o,n)]) + beta[c*N + n]   (comp_neighbors, nfp.py:42-82)
// with a zero-padded tap reading 0 + bias.  The pair symmetry the unbiased kernels build on (pair (p, p+d) serves both
// p and p+d) is gone — v depends on the direction n — so these kernels walk pairs directly:
//   bias_fwd    one thread per (output, channel group), looping over neighbours: the measure's channel sums AND both sides'
//               per-pixel statistics (Meas<M>::stat) of this pair; per-pair saved state (sized like `out`, 2*NSTAT floats)
//   bias_coef   per-pair backward scalars Meas<M>::coef from grad_out, out and the saved per-pair stats -> scratch
//   bias_gx     grad_x in gather form, one thread per (image, channel, input pixel): the inverse of pad / stride /
//               dilation walked per pixel (every padded coordinate that folds onto it, every tap that reads it)
//   bias_part   grad of both biases, one workgroup per (channel, image): sums over (output, neighbour) pairs — also
//               the pairs whose neighbour is a zero-padded tap, which no input pixel sees — into per-image partials
//   bias_reduce the partials summed over the batch in a fixed order
// No atomics: every result is bitwise reproducible.  Meas<M> is called with diff = 0 on (a, v): the measure's own
// arithmetic, with the difference weights already applied in v (nfp_measures.h: term(a, v) = f(v) for Norm / RMSE).
#include "nfp_launch.h"
#include "nfp_measures.h"

#include <climits>
#include <type_traits>

namespace nfp {
namespace {

constexpr int kBiasT = 256;

// element offset of pixel (y, x) of channel c of image b
__device__ __forceinline__ long long px_off(const KP& g, int b, int c, int y, int xx) {
  return (long long)b * g.sB + (long long)c * g.sC + (long long)y * g.sH + (long long)xx * g.sW;
}
// input coordinates (y, x) of tap (ky, kx) of output (oy, ox); false = zero padding
__device__ __forceinline__ bool tap_yx(const KP& g, int oy, int ox, int ky, int kx, int& y, int& xx) {
  y = map_index(oy * g.stride + ky * g.dil - g.pad, g.H, g.mode);
  xx = map_index(ox * g.stride + kx * g.dil - g.pad, g.W, g.mode);
  return y >= 0 && xx >= 0;
}
__device__ __forceinline__ int nbr_tap(const KP& g, int n) { return n < (g.k * g.k) / 2 ? n : n + 1; }

// sum over the 64 lanes of a wavefront, lane 0's result in a fixed order (xor butterfly)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Saved state, per pair i = (b*N + n)*O + o: k < NS the centre side's Meas::save<k>, NS <= k < 2NS the neighbour side's,
// at saved[k * BNO + i].  Attention (M = DOT with dots != null): the raw dots instead, in `dots`.
// Workgroup = (tile of OT outputs, NB neighbours, image); thread = (output, channel group), G = kBiasT / OT groups.
// cfast (channels-last): G = 64, one wavefront per output, lanes along the channels, combined by wave_sum; otherwise the
// G groups of an output are combined through LDS.  Both in a fixed order.
template <int M>
__global__ void __launch_bounds__(kBiasT) bias_fwd(const KP g, int dw, int OT, int cfast, int NB, const void* __restrict__ x,
                                                   const float* __restrict__ bc, const float* __restrict__ beta,
                                                   void* __restrict__ out, float* __restrict__ saved, float* __restrict__ dots) {
  constexpr int NS = Meas<M>::NSTAT;
  __shared__ float red[5 * kBiasT];
  const int t = threadIdx.x, G = kBiasT / OT;
  const int ol = cfast ? t / G : t % OT, cg = cfast ? t % G : t / OT;
  const int o = blockIdx.x * OT + ol, b = blockIdx.z;
  const int n_begin = blockIdx.y * NB, n_end = min(g.N, n_begin + NB);
  const bool live = o < g.O;
  const int oy = live ? o / g.Wo : 0, ox = o - oy * g.Wo;
  int cy, cx;
  const bool hc = live && tap_yx(g, oy, ox, g.R, g.R, cy, cx);
  const long long offc = hc ? px_off(g, b, 0, cy, cx) : 0;
  const long long BNO = (long long)g.B * g.N * g.O;
  for (int n = n_begin; n < n_end; ++n) {
    float acc = 0.f, sa0 = 0.f, sa1 = 0.f, sb0 = 0.f, sb1 = 0.f, pa = 0.f, pb = 0.f;
    if (live) {
      const int tp = nbr_tap(g, n);
      int qy, qx;
      const bool hq = tap_yx(g, oy, ox, tp / g.k, tp % g.k, qy, qx);
      const long long offq = hq ? px_off(g, b, 0, qy, qx) : 0;
      if (Pivot<M>::v) {  // sums about channel 0 of this pair (nfp_measures.h::Pivot)
        const float xa = hc ? ldx(x, offc, g.dtype) : 0.f, xq = hq ? ldx(x, offq, g.dtype) : 0.f;
        pa = xa + (bc ? bc[0] : 0.f);
        pb = (dw ? xa - xq : xq) + beta[n];
      }
      for (int c = cg; c < g.C; c += G) {
        const float xa = hc ? ldx(x, offc + (long long)c * g.sC, g.dtype) : 0.f;
        const float xq = hq ? ldx(x, offq + (long long)c * g.sC, g.dtype) : 0.f;
        const float a = xa + (bc ? bc[c] : 0.f) - pa;
        const float v = (dw ? xa - xq : xq) + beta[c * g.N + n] - pb;
        acc += Meas<M>::term(a, v, g);
        Meas<M>::stat(a, sa0, sa1);
        Meas<M>::stat(v, sb0, sb1);
      }
    }
    float s[5] = {acc, sa0, sa1, sb0, sb1};
    if (cfast) {
#pragma unroll
      for (int k = 0; k < 5; ++k) s[k] = wave_sum(s[k]);
    } else {
      __syncthreads();  // (the previous neighbour's sums are read)
#pragma unroll
      for (int k = 0; k < 5; ++k) red[k * kBiasT + t] = s[k];
      __syncthreads();
      if (cg == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = 0.f;
        for (int j = 0; j < G; ++j)
#pragma unroll
          for (int k = 0; k < 5; ++k) s[k] += red[k * kBiasT + j * OT + ol];
      }
    }
    if (!live || cg != 0) continue;
    const long long i = ((long long)b * g.N + n) * g.O + o;
    if (dots != nullptr) {
      dots[i] = s[0];
      continue;
    }
    stx(out, i, Meas<M>::fin(s[0], s[1], s[2], s[3], s[4], g), g.odtype);
    if constexpr (NS > 0) {
      if (saved != nullptr) {
        saved[i] = Meas<M>::save0(s[1], s[2], g) + pa;
        saved[NS * BNO + i] = Meas<M>::save0(s[3], s[4], g) + pb;
        if (NS > 1) {
          saved[BNO + i] = Meas<M>::save1(s[1], s[2], g);
          saved[(NS + 1) * BNO + i] = Meas<M>::save1(s[3], s[4], g);
        }
      }
    }
  }
}

template <int M>
__global__ void __launch_bounds__(kBiasT) bias_coef(const KP g, const void* __restrict__ go, const void* __restrict__ out,
                                                    const float* __restrict__ saved, float* __restrict__ cf) {
  constexpr int NS = Meas<M>::NSTAT;
  const long long BNO = (long long)g.B * g.N * g.O;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < BNO; i += (long long)gridDim.x * blockDim.x) {
    const float sp0 = NS > 0 ? saved[i] : 0.f, sp1 = NS > 1 ? saved[BNO + i] : 0.f;
    const float sq0 = NS > 0 ? saved[NS * BNO + i] : 0.f, sq1 = NS > 1 ? saved[(NS + 1) * BNO + i] : 0.f;
    store_coef<M>(cf, BNO, i, Meas<M>::coef(ldx(go, i, g.godtype), ldx(out, i, g.odtype), sp0, sp1, sq0, sq1, g));
  }
}

// output coordinate oa that reads unpadded coordinate tc through tap d along an axis of `no` outputs, or -1
__device__ __forceinline__ int reader(const KP& g, int tc, int d, int no) {
  const int nn = tc + g.pad - d * g.dil;
  if (nn < 0) return -1;
  const int oa = g.stride == 1 ? nn : nn / g.stride;
  return (oa * g.stride != nn || oa >= no) ? -1 : oa;
}
// the e-th unpadded coordinate that padding folds onto i (e = 0: i itself, then the margins), or INT_MIN
__device__ __forceinline__ int fold(const KP& g, int i, int n, int e) {
  const int tc = e == 0 ? i : (e <= g.pad ? -e : n - 1 + (e - g.pad));
  return (e == 0 || map_index(tc, n, g.mode) == i) ? tc : INT_MIN;
}

// grad_x[b][c][r]: every (output, tap) that reads r — as the centre: d/da of the output's N pairs (plus d/dv with the
// difference weights); as neighbour n: d/dv (minus it with the difference weights) — in a fixed order.
template <int M>
__global__ void __launch_bounds__(kBiasT) bias_gx(const KP g, int dw, const void* __restrict__ x,
                                                  const float* __restrict__ bc, const float* __restrict__ beta,
                                                  const float* __restrict__ cf, void* __restrict__ gx) {
  const long long BNO = (long long)g.B * g.N * g.O, total = (long long)g.B * g.C * g.P;
  const bool nhwc = g.sC == 1;
  const int mid = (g.k * g.k) >> 1;
  for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
    int b, c, r;
    if (nhwc) {  // channels fastest: neighbouring lanes read neighbouring addresses
      c = (int)(it % g.C);
      const long long br = it / g.C;
      r = (int)(br % g.P);
      b = (int)(br / g.P);
    } else {
      r = (int)(it % g.P);
      const long long bc2 = it / g.P;
      c = (int)(bc2 % g.C);
      b = (int)(bc2 / g.C);
    }
    const int ry = r / g.W, rx = r - ry * g.W;
    const float xr = ldx(x, px_off(g, b, c, ry, rx), g.dtype);
    const float bcc = bc ? bc[c] : 0.f;
    const long long cbase = (long long)b * g.sB + (long long)c * g.sC;
    float acc = 0.f;
    for (int ey = 0; ey <= 2 * g.pad; ++ey) {
      const int ty = fold(g, ry, g.H, ey);
      if (ty == INT_MIN) continue;
      for (int ex = 0; ex <= 2 * g.pad; ++ex) {
        const int tx = fold(g, rx, g.W, ex);
        if (tx == INT_MIN) continue;
        for (int ky = 0; ky < g.k; ++ky) {
          const int oy = reader(g, ty, ky, g.Ho);
          if (oy < 0) continue;
          for (int kx = 0; kx < g.k; ++kx) {
            const int ox = reader(g, tx, kx, g.Wo);
            if (ox < 0) continue;
            const int o = oy * g.Wo + ox, tp = ky * g.k + kx;
            if (tp == mid) {  // r is the centre of output o
              const float a = xr + bcc;
              for (int n = 0; n < g.N; ++n) {
                const int tq = nbr_tap(g, n);
                int qy, qx;
                const float xq = tap_yx(g, oy, ox, tq / g.k, tq % g.k, qy, qx)
                                     ? ldx(x, cbase + (long long)qy * g.sH + (long long)qx * g.sW, g.dtype) : 0.f;
                const float v = (dw ? xr - xq : xq) + beta[c * g.N + n];
                float da, db;
                Meas<M>::grad(a, v, load_coef<M>(cf, BNO, ((long long)b * g.N + n) * g.O + o), g, da, db);
                acc += dw ? da + db : da;
              }
            } else {  // r is neighbour n of output o
              const int n = tp < mid ? tp : tp - 1;
              int cy, cx;
              const float xa = tap_yx(g, oy, ox, g.R, g.R, cy, cx)
                                   ? ldx(x, cbase + (long long)cy * g.sH + (long long)cx * g.sW, g.dtype) : 0.f;
              const float v = (dw ? xa - xr : xr) + beta[c * g.N + n];
              float da, db;
              Meas<M>::grad(xa + bcc, v, load_coef<M>(cf, BNO, ((long long)b * g.N + n) * g.O + o), g, da, db);
              acc += dw ? -db : db;
            }
          }
        }
      }
    }
    stx(gx, (long long)b * g.gB + (long long)c * g.sC + (long long)ry * g.sH + (long long)rx * g.sW, acc, g.dtype);
  }
}

// deterministic sum over the workgroup (fixed tree); the result in thread 0
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = kBiasT / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

// per-image partials of the bias gradients: part[b][c*N + n] = sum_o d/dv, part[b][C*N + c] = sum_{o,n} d/da.
// The workgroup's threads are split into TPN teams of NCH = kBiasT / TPN lanes: lane nl of every team takes neighbour
// n0 + nl, team `team` the outputs team, team + TPN, ...; the teams' sums are then added in team order (a fixed order).
template <int M>
__global__ void __launch_bounds__(kBiasT) bias_part(const KP g, int dw, const void* __restrict__ x,
                                                    const float* __restrict__ bc, const float* __restrict__ beta,
                                                    const float* __restrict__ cf, float* __restrict__ part) {
  __shared__ float red[kBiasT];
  const long long BNO = (long long)g.B * g.N * g.O;
  const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int TPN = max(1, kBiasT / g.N), NCH = kBiasT / TPN, nl = t % NCH, team = t / NCH;
  const long long cbase = (long long)b * g.sB + (long long)c * g.sC;
  float* pb = part + (long long)b * g.C * (g.N + 1);
  const float bcc = bc ? bc[c] : 0.f;
  float sda = 0.f;
  for (int n0 = 0; n0 < g.N; n0 += NCH) {
    const int n = n0 + nl;
    float sdb = 0.f;
    if (n < g.N && team < TPN) {
      const int tq = nbr_tap(g, n);
      const float bn = beta[c * g.N + n];
      for (int o = team; o < g.O; o += TPN) {
        const int oy = o / g.Wo, ox = o - oy * g.Wo;
        int cy, cx, qy, qx;
        const float xa = tap_yx(g, oy, ox, g.R, g.R, cy, cx) ? ldx(x, cbase + (long long)cy * g.sH + (long long)cx * g.sW, g.dtype) : 0.f;
        const float xq = tap_yx(g, oy, ox, tq / g.k, tq % g.k, qy, qx)
                             ? ldx(x, cbase + (long long)qy * g.sH + (long long)qx * g.sW, g.dtype) : 0.f;
        const float v = (dw ? xa - xq : xq) + bn;
        float da, db;
        Meas<M>::grad(xa + bcc, v, load_coef<M>(cf, BNO, ((long long)b * g.N + n) * g.O + o), g, da, db);
        sdb += db;
        sda += da;
      }
    }
    __syncthreads();   // (the previous chunk's sums are read)
    red[t] = sdb;
    __syncthreads();
    if (team == 0 && n < g.N) {
      float s = 0.f;
      for (int i = 0; i < TPN; ++i) s += red[i * NCH + nl];
      pb[c * g.N + n] = s;
    }
  }
  const float s = block_sum(sda, red);
  if (t == 0) pb[g.C * g.N + c] = s;
}

__global__ void __launch_bounds__(kBiasT) bias_reduce(int B, int CN, int C, const float* __restrict__ part,
                                                      float* __restrict__ gbeta, float* __restrict__ gbc) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= CN + C || (j >= CN && gbc == nullptr)) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += part[(long long)b * (CN + C) + j];
  if (j < CN)
    gbeta[j] = s;
  else
    gbc[j - CN] = s;
}

}  // namespace
}  // namespace nfp

namespace nfp_host {
namespace {

// the Meas<> of a bias-path descriptor (g.measure is the descriptor's own: EMD stays EMD, Attention is DotProduct here)
template <typename F>
int bias_switch(const KP& g, F&& f) {
  const int rc = with_measure(g, f);
  return rc == kNotApplicable ? fail(NFP_E_UNSUPPORTED, "measure %d has no biased HIP kernel", g.measure) : rc;
}

unsigned flat_blocks(long long n) { return (unsigned)std::min<long long>((n + kBiasT - 1) / kBiasT, 1LL << 20); }

}  // namespace

int bias_coef_floats(const KP& g) {
  switch (g.measure) {
    case NFP_COSINE: case NFP_GFC: case NFP_SMITH: return 3;
    case NFP_PEARSON: return 5;
    default: return 1;
  }
}

int bias_forward(const KP& g, int dw, const void* x, const float* bc, const float* beta, void* out, float* saved,
                 float* dots, hipStream_t st) {
  // channels-last: the channel groups are the fast thread axis (lanes read neighbouring channels)
  const int cfast = g.sC == 1 ? 1 : 0;
  const int OT = cfast ? 4 : 64;
  // neighbours per workgroup: all of them where the (tile, image) grid alone fills the chip, fewer on small maps
  const long long per_n = (long long)((g.O + OT - 1) / OT) * g.B;
  int NB = g.N;
  while (NB > 1 && per_n * ((g.N + NB - 1) / NB) < 4096) NB = (NB + 1) / 2;
  const dim3 grid((unsigned)((g.O + OT - 1) / OT), (unsigned)((g.N + NB - 1) / NB), (unsigned)g.B);
  return bias_switch(g, [&](auto m) {
    constexpr int M = decltype(m)::value;
    snprintf(g_variant, sizeof(g_variant), "bias_fwd<%d,%s>x%d", M, cfast ? "nhwc" : "nchw", NB);
    return launch("bias_fwd", bias_fwd<M>, grid, dim3(kBiasT), 0, st, g, dw, OT, cfast, NB, x, bc, beta, out, saved, dots);
  });
}

int bias_backward(const KP& g, int dw, const void* x, const float* bc, const float* beta, const void* go, const void* out,
                  const float* saved, void* gx, float* gbc, float* gbeta, float* scratch, hipStream_t st) {
  const long long BNO = (long long)g.B * g.N * g.O;
  float* cf = scratch;
  float* part = scratch + BNO * bias_coef_floats(g);
  return bias_switch(g, [&](auto m) {
    constexpr int M = decltype(m)::value;
    snprintf(g_variant, sizeof(g_variant), "bias_bwd<%d,%s>", M, g.sC == 1 ? "nhwc" : "nchw");
    if (g.B > 0) {
    if (int rc = launch("bias_coef", bias_coef<M>, dim3(flat_blocks(BNO)), dim3(kBiasT), 0, st, g, go, out, saved, cf)) return rc;
    if (int rc = launch("bias_gx", bias_gx<M>, dim3(flat_blocks((long long)g.B * g.C * g.P)), dim3(kBiasT), 0, st, g, dw, x,
                        bc, beta, (const float*)cf, gx))
      return rc;
    if (int rc = launch("bias_part", bias_part<M>, dim3((unsigned)g.C, (unsigned)g.B), dim3(kBiasT), 0, st, g, dw, x, bc, beta,
                        (const float*)cf, part))
      return rc;
    }
    const int CN = g.C * g.N;   // (an empty batch: zero bias gradients)
    return launch("bias_reduce", bias_reduce, dim3((unsigned)((CN + g.C + kBiasT - 1) / kBiasT)), dim3(kBiasT), 0, st, g.B, CN,
                  g.C, (const float*)part, gbeta, gbc);
  });
}

}  // namespace nfp_host
