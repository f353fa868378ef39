// nfp_valid.h — what the "x -> maps" units (nfp_valid.hip: unpadded maps; nfp_strided.hip: stride 2-4) share: the element
// load, the tap numbering, the finished value and the backward scalars of a pair under the descriptor's measure, and the
// host-side layout predicates and chunk sizing.  Everything here is inline; no kernel of its own.
#pragma once
#include "nfp_launch.h"
#include "nfp_measures.h"

namespace nfp {

constexpr int kValidLdsFloats = 20000;   // 80 000 bytes: two workgroups per CU out of 160 KiB

template <int BF>
__device__ __forceinline__ float ldv(const void* p, long long i) {
  return BF ? bf16_to_f32(((const uint16_t*)p)[i]) : ((const float*)p)[i];
}

// tap n of the k x k window without its centre -> (dy, dx)
template <int R>
__device__ __forceinline__ void tap_of(int n, int& dy, int& dx) {
  constexpr int K = 2 * R + 1;
  const int t = n < (K * K) / 2 ? n : n + 1;
  dy = t / K - R;
  dx = t - (t / K) * K - R;
}

// the finished map value of a pair sum (wave-uniform switch on the descriptor's measure)
template <int PROD>
__device__ __forceinline__ float valid_fin(const KP& g, float acc, float n2p, float n2q) {
  if (PROD == 2) return g.similarity ? -acc : acc;   // (Norm p = 1: the sum of |a - t| itself)
  if (PROD) {
    if (g.measure == NFP_COSINE) {
      // ONE correctly rounded division by the product of the clamped norms (not acc * (1 / m_p) * (1 / m_q)): the same
      // value for both orientations of a pair, and exactly +-1 where the two pixels are parallel to rounding (C = 1:
      // |fl(a b)| == fl(|a| |b|)) — which the backward's projected form relies on
      const float s = acc / (fmaxf(sqrtf(n2p), g.eps) * fmaxf(sqrtf(n2q), g.eps));
      return g.similarity ? s : 1.f - s;
    }
    if (g.measure == NFP_GFC) return Meas<NFP_GFC>::fin(acc, n2p, 0.f, n2q, 0.f, g);
    return Meas<NFP_DOT>::fin(acc, 0.f, 0.f, 0.f, 0.f, g);
  }
  if (g.measure == NFP_RMSE) return Meas<NFP_RMSE>::fin(acc, 0.f, 0.f, 0.f, 0.f, g);
  return Meas<kNormP2>::fin(acc, 0.f, 0.f, 0.f, 0.f, g);
}
// the backward scalars of a pair (centre norm np, neighbour norm nq)
template <int PROD>
__device__ __forceinline__ Coef valid_coef(const KP& g, float go, float ov, float np, float nq) {
  if (PROD) {
    if (g.measure == NFP_COSINE) return Meas<NFP_COSINE>::coef(go, ov, np, 0.f, nq, 0.f, g);
    if (g.measure == NFP_GFC) return Meas<NFP_GFC>::coef(go, ov, np, 0.f, nq, 0.f, g);
    return Meas<NFP_DOT>::coef(go, ov, 0.f, 0.f, 0.f, 0.f, g);
  }
  if (g.measure == NFP_RMSE) return Meas<NFP_RMSE>::coef(go, ov, 0.f, 0.f, 0.f, 0.f, g);
  return Meas<kNormP2>::coef(go, ov, 0.f, 0.f, 0.f, 0.f, g);
}

}  // namespace nfp

namespace nfp_host {

// what the kernels read in place: images dense in NCHW or channels-last order (any batch stride)
inline bool valid_nchw(const KP& g) { return g.sW == 1 && g.sH == g.W && g.sC == (long long)g.H * g.W; }
inline bool valid_nhwc(const KP& g) { return g.sC == 1 && g.sW == g.C && g.sH == (long long)g.W * g.C; }
inline int valid_ve(const KP& g) { return g.dtype == NFP_BF16 ? 8 : 4; }

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline int valid_even_chunk(int C, int cap, int mult) {
  cap = std::max(mult, cap / mult * mult);
  const int nch = ceil_div(C, cap);
  return std::min(cap, ceil_div(ceil_div(C, nch), mult) * mult);
}

}  // namespace nfp_host
