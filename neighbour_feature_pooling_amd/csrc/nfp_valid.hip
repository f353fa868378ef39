// nfp_valid.hip — NFP on VALID maps: stride 1, dilation 1, padding 0, R = 1 or 2 (include/nfp.h: nfp_valid_*).  The layer
// models/nfp_heads.py::NFPBottleneck (nfp_heads.py:234-278) puts inside every residual block, and SimilarityAwarePooling
// (nfp_heads.py:204-232) in front of its softmax.  Ho = H - 2R, Wo = W - 2R; output (i, j) has its centre at input pixel
// (i + R, j + R) and every tap inside the image: no padding mode, no fold, no index table.
//
// Forward, fwd_valid<R, PROD, BF, NHWC>: one workgroup per (image, band of rb output rows).  The band's input rows
// [i0, i0 + rb + 2R) are staged in LDS as float32, channel-major (xs[c * S + pixel], S odd), in chunks of Cc channels.
// HALF STENCIL: thread (grp, u) owns staged pixel u and the NH = N/2 pairs {u, u + d} whose offset d points forward in
// row-major order; it sums them (products: x_u . x_t and |x_u|^2; distances: |x_u - x_t|^2) over the channels
// c = grp, grp + G, ... of every chunk, in registers.  The G groups' partial sums are then joined through LDS in group
// order, and one thread per (output, tap) looks its pair up — at its own centre for a forward tap, at the neighbour for a
// backward one — and finishes it (nfp_measures.h: Meas<>::fin).  An output element has one writer; `saved` gets |x| per
// input pixel (cosine / gfc), every pixel from the band that owns its row.  A pair whose ends both lie on the border is
// summed and never looked up.
//
// Backward, bwd_valid<R, FAM, BF, NHWC>: gather form, one workgroup per (image, band of rb INPUT rows, channel block).
//   dot, gfc    grad_x[c][r] = sum_j Wt[j][r] x[c][r + d_j] + diag[r] x[c][r]
//   cosine      the projected form on unit vectors (at the kernel): every pair's bracket cancels before it is scaled
//   distances   grad_x[c][r] = sum_j Wt[j][r] (x[c][r] - x[c][r + d_j])        (inf * 0 = NaN exactly where torch has it)
// Slot j of pixel r joins the coefficient of output r with tap j (r interior) and the one of output r + d_j with the
// opposite tap (r + d_j interior) — Meas<>::coef of grad_out, out and the saved norms, read under those two predicates:
// nothing outside [0, Ho) x [0, Wo) is ever addressed.  Phase A: one thread per band pixel writes its N slots and its
// diagonal to LDS.  Phase B: thread (r, grp) keeps the N slots in registers and walks the channel quads grp, grp + G, ...
// of every staged chunk (input rows [r0 - R, r0 + rb + R) clipped to the image).  Channels-last maps put grp along the
// lanes, so that a lane stores 4 adjacent channels and neighbouring lanes neighbouring quads.
// No atomics, every sum in a fixed order: two runs agree bitwise and image b's results do not depend on B.
//
// The L1 family (include/nfp.h: nfp_valid_abs_* — Norm p = 1 on the difference weights, the reference's default layer, and
// EMD, which make_kp turns into it): fwd_valid<R, 2, ...> sums |x_u - x_t| over the same half stencil and finishes it as
// -+ the sum; no norm, nothing saved.  bwd_valid<R, 3, ...>: the pair's coefficient is -+ grad_out alone, so phase A reads
// grad_out under the two predicates and nothing else (no out, no saved, no diagonal), and phase B is
//   grad_x[c][r] = sum_j Wt[j][r] sgn(x[c][r] - x[c][r + d_j])                   sgn(0) = 0 (torch's abs backward)
// formed as bwd_tile's kNormP1 instantiation forms it: sgn3 (a compare, a select and a sign copy) under one fma.  Same
// sizing, bands, chunks, channel blocks, lane maps and stores as the other families.
#include "nfp_valid.h"   // (ldv, tap_of, valid_fin, valid_coef and the layout predicates: shared with nfp_strided.hip)

namespace nfp {
namespace {

constexpr int kValidFwdT = 1024, kValidBwdT = 512;

struct VP {
  int rb;     // rows per band: output rows (forward) / input rows (backward)
  int npix;   // pixels a full band's threads stand for: (rb + 2R) * W staged (forward) / rb * W owned (backward)
  int S;      // floats between two channels of the staged slab (odd)
  int Cc;     // channels per chunk
  int G;      // channel groups (forward: channels, backward: channel quads)
  int vec;    // 16-byte global loads: rows and pointers allow them
  int Cz;     // backward: channels per workgroup along grid.z (a multiple of 8, or C)
};

// rows [y0, y0 + rows) of image b, channels [c0, c0 + cc) -> xs[c * S + (y - y0) * W + x], float32
template <int BF, int NHWC>
__device__ __forceinline__ void stage_rows(const KP& g, const VP& v, const void* x, long long img, int y0, int rows, int c0,
                                           int cc, float* xs, int tid, int T) {
  const int len = rows * g.W;
  constexpr int VE = BF ? 8 : 4;   // elements per 16 bytes
  if (NHWC) {
    // [pixel][c]: 16 bytes = VE adjacent channels of one pixel (C % VE == 0, images 16-byte aligned: valid_shape)
    const int cq = cc / VE;
    const long long base = img + (long long)y0 * g.W * g.C + c0;
    for (int it = tid; it < len * cq; it += T) {
      const int p = it / cq, q = it - p * cq;
      const uint4 w = *(const uint4*)((const char*)x + (base + (long long)p * g.C + q * VE) * (BF ? 2 : 4));
      float* d = xs + (q * VE) * v.S + p;
      if (BF) {
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          d[(2 * k) * v.S] = __uint_as_float(u[k] << 16);
          d[(2 * k + 1) * v.S] = __uint_as_float(u[k] & 0xffff0000u);
        }
      } else {
        d[0] = __uint_as_float(w.x);
        d[v.S] = __uint_as_float(w.y);
        d[2 * v.S] = __uint_as_float(w.z);
        d[3 * v.S] = __uint_as_float(w.w);
      }
    }
    return;
  }
  // [c][pixel]: the band's rows of one channel are contiguous
  const long long base = img + (long long)c0 * g.sC + (long long)y0 * g.W;
  if (v.vec) {
    const int lq = len / VE;
    for (int it = tid; it < cc * lq; it += T) {
      const int c = it / lq, q = it - c * lq;
      const uint4 w = *(const uint4*)((const char*)x + (base + (long long)c * g.sC + q * VE) * (BF ? 2 : 4));
      float* d = xs + c * v.S + q * VE;
      if (BF) {
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          d[2 * k] = __uint_as_float(u[k] << 16);
          d[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u);
        }
      } else {
        d[0] = __uint_as_float(w.x);
        d[1] = __uint_as_float(w.y);
        d[2] = __uint_as_float(w.z);
        d[3] = __uint_as_float(w.w);
      }
    }
  } else {
    for (int it = tid; it < cc * len; it += T) {
      const int c = it / len, p = it - c * len;
      xs[c * v.S + p] = ldv<BF>(x, base + (long long)c * g.sC + p);
    }
  }
}

// grid = (bands, B).  Dynamic LDS (floats): max(Cc * S, G * (NH + 1) * npix) — the slab, then the groups' partial sums.
// PROD: 0 squared differences, 1 products (and |x_u|^2), 2 absolute differences (the L1 family: `saved` is never written)
template <int R, int PROD, int BF, int NHWC>
__global__ void __launch_bounds__(kValidFwdT) fwd_valid(KP g, VP v, const void* __restrict__ x, void* __restrict__ out,
                                                        float* __restrict__ saved) {
  extern __shared__ __attribute__((aligned(16))) float vlds[];
  constexpr int K = 2 * R + 1, N = K * K - 1, NH = N / 2;
  const int tid = threadIdx.x, T = blockDim.x, W = g.W;
  const int b = blockIdx.y, i0 = blockIdx.x * v.rb;   // first output row = first staged input row
  const int rb = min(v.rb, g.Ho - i0), rin = rb + 2 * R, npix = rin * W;
  const long long img = (long long)b * g.sB;
  const int grp = tid / v.npix, u = tid - grp * v.npix;
  const bool act = grp < v.G && u < npix;
  const int uy = u / W, ux = u - uy * W;
  int off[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    int dy, dx;
    tap_of<R>(NH + h, dy, dx);
    const bool ok = act && ux + dx >= 0 && ux + dx < W && uy + dy < rin;
    off[h] = ok ? dy * W + dx : 0;   // (a pair that leaves the band sums x_u with itself and is never looked up)
  }
  float acc[NH], n2 = 0.f;
#pragma unroll
  for (int h = 0; h < NH; ++h) acc[h] = 0.f;
  for (int c0 = 0; c0 < g.C; c0 += v.Cc) {
    const int cc = min(v.Cc, g.C - c0);
    if (c0 > 0) __syncthreads();   // (the previous chunk has been summed)
    stage_rows<BF, NHWC>(g, v, x, img, i0, rin, c0, cc, vlds, tid, T);
    __syncthreads();
    if (act) {
#pragma unroll 2
      for (int c = grp; c < cc; c += v.G) {
        const float* xc = vlds + c * v.S + u;
        const float a = xc[0];
        if (PROD == 1) n2 = fmaf(a, a, n2);
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          const float t = xc[off[h]];
          if (PROD == 1) {
            acc[h] = fmaf(a, t, acc[h]);
          } else if (PROD == 2) {
            acc[h] += fabsf(a - t);
          } else {
            const float d = a - t;
            acc[h] = fmaf(d, d, acc[h]);
          }
        }
      }
    }
  }
  __syncthreads();   // (the slab has been read: the partial sums take its place)
  // pr[h * v.npix + u]: pair sums h < NH, |x_u|^2 at h = NH; group grp's share (NH + 1) * v.npix floats further on
  constexpr int NS = NH + 1;
  if (act) {
    float* mine = vlds + (grp * NS) * v.npix + u;
#pragma unroll
    for (int h = 0; h < NH; ++h) mine[h * v.npix] = acc[h];
    mine[NH * v.npix] = n2;
  }
  __syncthreads();
  if (v.G > 1) {
    for (int it = tid; it < NS * v.npix; it += T) {
      float s = vlds[it];
      for (int q = 1; q < v.G; ++q) s += vlds[q * NS * v.npix + it];
      vlds[it] = s;   // (slot 0 of an item is read and written by this thread alone)
    }
    __syncthreads();
  }
  const float* pr = vlds;
  const float* n2s = vlds + NH * v.npix;
  // |x| per input pixel for the backward: a band owns the rows of its centres, the first and the last band the border rows
  if (PROD == 1 && g.measure != NFP_DOT && saved != nullptr) {
    const bool first = blockIdx.x == 0, last = blockIdx.x == gridDim.x - 1;
    float* sv = saved + (long long)b * g.P + (long long)i0 * W;
    for (int p = tid; p < npix; p += T) {
      const int py = p / W;
      if ((py >= R || first) && (py < rb + R || last)) sv[p] = sqrtf(n2s[p]);
    }
  }
  // one thread per (tap, output of the band): out[b][n][i0 * Wo + ol], neighbouring lanes neighbouring outputs
  const int no = rb * g.Wo;
  const long long obase = (long long)b * N * g.O + (long long)i0 * g.Wo;
  for (int it = tid; it < N * no; it += T) {
    const int n = it / no, ol = it - n * no;
    const int oi = ol / g.Wo, oj = ol - oi * g.Wo;
    int dy, dx;
    tap_of<R>(n, dy, dx);
    const int uc = (oi + R) * W + oj + R, q = uc + dy * W + dx;
    // forward tap: the pair starts at the centre; backward tap: at the neighbour, under the opposite offset
    const float pairv = n >= NH ? pr[(n - NH) * v.npix + uc] : pr[(NH - 1 - n) * v.npix + q];
    const float val = valid_fin<PROD>(g, pairv, n2s[uc], n2s[q]);
    const long long oidx = obase + (long long)n * g.O + ol;
    if (BF)
      ((uint16_t*)out)[oidx] = f32_to_bf16(val);
    else
      ((float*)out)[oidx] = val;
  }
}

// grid = (bands, B, channel blocks).  Dynamic LDS (floats): wt[N * npix], dg[npix], then the slab xs[round4(Cc) * S].
// A channel's gradient depends on the slots and on that channel of x alone: every channel block repeats phase A and the
// blocks' results are those of one workgroup walking all channels, bit for bit.
// FAM: 0 distances, 1 products in the gather form above (dot, gfc), 3 the L1 family (slots of -+ grad_out alone, signs of
// the differences in phase B; `outm` and `saved` are never read), 2 cosine in the PROJECTED form
//   grad_x[c][r] = (1 / m_r) sum_j G[j][r] (xn[c][r + d_j] - s[j][r] rho_r xn[c][r])      xn = x / m, m = max(|x|, eps)
// G the pair's grad_out (both orientations added), s its cosine, rho_r = m_r / |x_r| (0 at |x_r| = 0).  The gather form
// takes the cosine's gradient as the difference of two sums of size |grad_out| / |x_r|; where pixel and neighbour are
// nearly parallel — exactly so for C = 1, where the gradient is identically zero — that difference is all rounding error
// (1.3e-5 absolute at (2, 1, 6, 6)).  Here every pair's bracket is the neighbour's unit vector minus its projection on
// the pixel's: it cancels before anything is scaled, exactly for C = 1 (xn = +-1 by a correctly rounded division, s = +-1
// from fwd_valid).  Costs a second fma per tap and a pass that normalises the staged chunk.
template <int R, int FAM, int BF, int NHWC>
__global__ void __launch_bounds__(kValidBwdT) bwd_valid(KP g, VP v, const void* __restrict__ x, const void* __restrict__ go,
                                                        const void* __restrict__ outm, const float* __restrict__ saved,
                                                        void* __restrict__ gx) {
  extern __shared__ __attribute__((aligned(16))) float vlds[];
  constexpr int K = 2 * R + 1, N = K * K - 1;
  const int tid = threadIdx.x, T = blockDim.x, W = g.W, H = g.H;
  const int b = blockIdx.y, r0 = blockIdx.x * v.rb;   // first input row of the band
  const int rb = min(v.rb, H - r0), npix = rb * W;
  const int y0 = max(r0 - R, 0), y1 = min(r0 + rb + R, H), rows = y1 - y0;
  constexpr int PROD = (FAM == 1 || FAM == 2) ? 1 : 0;
  constexpr int NW = FAM == 2 ? 2 * N : N;   // slots per pixel: cosine keeps the pair's cosine beside its weight
  float* wt = vlds;
  float* sv = wt + N * v.npix;               // (FAM == 2 only)
  float* dg = wt + NW * v.npix;
  float* xs = vlds + (((NW + 1) * v.npix + 3) & ~3);
  const long long img = (long long)b * g.sB;
  // ---- phase A: the N slots and the diagonal of every pixel of the band
  const long long mbase = (long long)b * N * g.O;
  const float* nrm = saved != nullptr ? saved + (long long)b * g.P : nullptr;
  const bool stats = PROD && g.measure != NFP_DOT;
  for (int r = tid; r < npix; r += T) {
    const int ry = r / W, y = r0 + ry, xc = r - ry * W;
    const bool in_r = y >= R && y < H - R && xc >= R && xc < W - R;
    const int o_r = (y - R) * g.Wo + (xc - R);
    const float n_r = stats ? nrm[y * W + xc] : 0.f;
    float dsum = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      int dy, dx;
      tap_of<R>(j, dy, dx);
      const int y2 = y + dy, x2 = xc + dx;
      const bool in_t = y2 >= R && y2 < H - R && x2 >= R && x2 < W - R;
      float w = 0.f;
      if (FAM == 2) {
        // the pair's grad_out from both orientations and its one cosine (fwd_valid finishes both orientations alike)
        float gsum = 0.f, sj = g.similarity ? 0.f : 1.f;
        if (in_r) {
          const long long i = mbase + (long long)j * g.O + o_r;
          gsum += ldv<BF>(go, i);
          sj = ldv<BF>(outm, i);
        }
        if (in_t) {
          const long long i = mbase + (long long)(N - 1 - j) * g.O + (y2 - R) * g.Wo + (x2 - R);
          gsum += ldv<BF>(go, i);
          sj = ldv<BF>(outm, i);
        }
        w = g.similarity ? gsum : -gsum;
        sv[j * v.npix + r] = g.similarity ? sj : 1.f - sj;
      } else if (FAM == 3) {
        if (in_r) w += dist_sign(g, ldv<BF>(go, mbase + (long long)j * g.O + o_r));
        if (in_t) w += dist_sign(g, ldv<BF>(go, mbase + (long long)(N - 1 - j) * g.O + (y2 - R) * g.Wo + (x2 - R)));
      } else if (in_r || in_t) {   // (then (y2, x2) is a pixel of the image)
        const float n_t = stats ? nrm[y2 * W + x2] : 0.f;
        if (in_r) {
          const long long i = mbase + (long long)j * g.O + o_r;
          const Coef cf = valid_coef<PROD>(g, ldv<BF>(go, i), ldv<BF>(outm, i), n_r, n_t);
          w += cf.k0;
          dsum += cf.k1;
        }
        if (in_t) {
          const long long i = mbase + (long long)(N - 1 - j) * g.O + (y2 - R) * g.Wo + (x2 - R);
          const Coef cf = valid_coef<PROD>(g, ldv<BF>(go, i), ldv<BF>(outm, i), n_t, n_r);
          w += cf.k0;
          dsum += cf.k2;
        }
      }
      wt[j * v.npix + r] = w;
    }
    dg[r] = -dsum;
  }
  // ---- phase B
  int r, grp;
  if (NHWC) {
    r = tid / v.G;
    grp = tid - r * v.G;
  } else {
    grp = tid / v.npix;
    r = tid - grp * v.npix;
  }
  const bool act = r < npix && grp < v.G;
  const int ry = r / W, y = r0 + ry, xcol = r - ry * W;
  const int lp = (y - y0) * W + xcol;   // the pixel inside the staged rows
  float wr[N], sr[FAM == 2 ? N : 1], dr = 0.f, ir = 0.f, rho = 0.f;
  int off[N];
  __syncthreads();   // (wt and dg are complete)
#pragma unroll
  for (int j = 0; j < N; ++j) {
    int dy, dx;
    tap_of<R>(j, dy, dx);
    const bool ok = act && y + dy >= 0 && y + dy < H && xcol + dx >= 0 && xcol + dx < W;
    off[j] = ok ? dy * W + dx : 0;             // (outside the image the slot is 0: any staged address serves)
    wr[j] = act ? wt[j * v.npix + r] : 0.f;
    if (FAM == 2) sr[j] = act ? sv[j * v.npix + r] : 0.f;
  }
  if (act) dr = dg[r];
  if (FAM == 2 && act) {
    const float n = nrm[y * W + xcol], m = fmaxf(n, g.eps);
    ir = 1.f / m;
    rho = n > 0.f ? m / n : 0.f;   // (exactly 1 above eps)
  }
  const long long gimg = (long long)b * g.gB;
  const int cbeg = blockIdx.z * v.Cz, cend = min(g.C, cbeg + v.Cz);   // this workgroup's channels
  for (int c0 = cbeg; c0 < cend; c0 += v.Cc) {
    const int cc = min(v.Cc, cend - c0);
    if (c0 > cbeg) __syncthreads();   // (the previous chunk has been read)
    stage_rows<BF, NHWC>(g, v, x, img, y0, rows, c0, cc, xs, tid, T);
    __syncthreads();
    if (FAM == 2) {   // xn = x / max(|x|, eps): a correctly rounded division (unit vectors of C = 1 are exactly +-1)
      const float* nr = nrm + y0 * W;
      const int len = rows * W;
      for (int it = tid; it < cc * len; it += T) {
        const int c = it / len, p = it - c * len;
        xs[c * v.S + p] = xs[c * v.S + p] / fmaxf(nr[p], g.eps);
      }
      __syncthreads();
    }
    if (!act) continue;
    for (int cq = grp; 4 * cq < cc; cq += v.G) {
      float a4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float* xc = xs + (4 * cq + k) * v.S + lp;   // (channels past cc: inside the slab's round4(Cc) rows, not stored)
        const float a = xc[0];
        float s = FAM == 1 ? dr * a : 0.f;
        if (FAM == 2) {
          const float u = rho * a;
#pragma unroll
          for (int j = 0; j < N; ++j) s = fmaf(wr[j], fmaf(-sr[j], u, xc[off[j]]), s);
          s *= ir;
        } else {
#pragma unroll
          for (int j = 0; j < N; ++j)
            s = PROD ? fmaf(wr[j], xc[off[j]], s) : fmaf(wr[j], FAM == 3 ? sgn3(a - xc[off[j]]) : a - xc[off[j]], s);
        }
        a4[k] = s;
      }
      const int c = c0 + 4 * cq;
      if (NHWC) {
        const long long i = gimg + ((long long)(r0 * W + r)) * g.C + c;   // (C % 4 == 0: the quad is whole)
        if (BF) {
          uint2 pk;
          pk.x = f32_to_bf16x2(a4[0], a4[1]);
          pk.y = f32_to_bf16x2(a4[2], a4[3]);
          *(uint2*)((uint16_t*)gx + i) = pk;
        } else {
          *(float4*)((float*)gx + i) = make_float4(a4[0], a4[1], a4[2], a4[3]);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (4 * cq + k < cc) {
            const long long i = gimg + (long long)(c + k) * g.P + r0 * W + r;
            if (BF)
              ((uint16_t*)gx)[i] = f32_to_bf16(a4[k]);
            else
              ((float*)gx)[i] = a4[k];
          }
        }
      }
    }
  }
}

}  // namespace
}  // namespace nfp

namespace nfp_host {
namespace {

constexpr int kValidMaxW = 128;

// Bands of about 8 rows (a halo of 2R rows on top: a quarter / a half more staged than owned), fewer rows where the
// threads or the LDS ask for it.  NOT a function of the batch: the band height sets the number of channel groups, and with
// it the order of the sums — image b's results must not depend on B.
int valid_bands(int rows, int rb_max) { return std::max(ceil_div(rows, rb_max), ceil_div(rows, 8)); }

}  // namespace

// geometry and layout: what both sets of entry points ask beside their measures
static const char* valid_shape_refusal(const KP& g) {
  if (g.rs == 12) return "one radius per call (inner_R = 0)";
  if (mixed_maps(g)) return "maps in the storage type (map_f32 = 0)";
  if (g.pad != 0 || g.stride != 1 || g.dil != 1 || (g.R != 1 && g.R != 2)) return "stride 1, dilation 1, padding 0, R = 1 or 2";
  if (g.W > kValidMaxW) return "rows of more than 128 pixels";
  if (!valid_nchw(g) && !valid_nhwc(g)) return "images dense in NCHW or channels-last order";
  if (!valid_nchw(g) && g.C % valid_ve(g) != 0) return "channels-last maps with C % 4 (float32) / C % 8 (bf16) != 0";
  if (!valid_nchw(g) && (g.sB % valid_ve(g) != 0 || g.gB % valid_ve(g) != 0)) return "channels-last images off 16-byte boundaries";
  return nullptr;
}

const char* valid_refusal(const KP& g) {
  if (!hot_measure(g)) return "cosine / dot / gfc / L2 (norm p=2) / rmse only";
  if (!hot_product(g) && !g.diff) return "a distance on the pure-neighbour weights";
  return valid_shape_refusal(g);
}

const char* valid_abs_refusal(const KP& g) {
  if (!hot_l1(g)) return "Norm p=1 / EMD only";
  if (!g.diff) return "a distance on the pure-neighbour weights";
  return valid_shape_refusal(g);
}

template <int R, int PROD>
static int valid_forward_rp(const KP& g, const void* x, void* out, float* saved, hipStream_t st) {
  constexpr int NH = ((2 * R + 1) * (2 * R + 1) - 1) / 2;
  const bool nhwc = !valid_nchw(g), bf = g.dtype == NFP_BF16;
  const int ve = valid_ve(g);
  if (nhwc && !aligned16(x)) return fail(NFP_E_UNSUPPORTED, "valid maps: channels-last images off 16-byte boundaries");
  VP v = {};
  const int rb_max = kValidFwdT / g.W - 2 * R;   // (W <= 128: at least 4)
  const int bands0 = valid_bands(g.Ho, rb_max);
  v.rb = ceil_div(g.Ho, bands0);
  const int bands = ceil_div(g.Ho, v.rb);
  v.npix = (v.rb + 2 * R) * g.W;
  v.S = v.npix | 1;
  v.G = std::max(1, std::min(std::min(8, g.C), 512 / v.npix));
  const int T = std::min(kValidFwdT, (v.G * v.npix + 63) & ~63);
  v.Cc = valid_even_chunk(g.C, kValidLdsFloats / v.S, 8);
  v.vec = (!nhwc && g.W % ve == 0 && g.sB % ve == 0 && aligned16(x)) ? 1 : 0;
  const size_t lds = sizeof(float) * (size_t)std::max(v.Cc * v.S, v.G * (NH + 1) * v.npix);
  snprintf(g_variant, sizeof(g_variant), "fwd_valid<%d,%s,%s,%s>", R, PROD == 2 ? "l1" : (PROD ? "prod" : "dist"), bf ? "bf16" : "f32",
           nhwc ? "nhwc" : "nchw");
  const dim3 grid((unsigned)bands, (unsigned)g.B), block(T);
  return with_storage(g, [&](auto bf_, auto nhwc_) {   // (valid_nchw is g.contig: make_kp)
    return launch("fwd_valid", nfp::fwd_valid<R, PROD, bf_(), nhwc_()>, grid, block, lds, st, g, v, x, out, saved);
  });
}

template <int R, int FAM>
static int valid_backward_rp(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                             hipStream_t st) {
  constexpr int N = (2 * R + 1) * (2 * R + 1) - 1;
  const bool nhwc = !valid_nchw(g), bf = g.dtype == NFP_BF16;
  const int ve = valid_ve(g);
  if (nhwc && (!aligned16(x) || !aligned16(gx)))
    return fail(NFP_E_UNSUPPORTED, "valid maps: channels-last images off 16-byte boundaries");
  VP v = {};
  const int rb_max = std::max(1, (R == 1 ? 512 : 256) / g.W);
  const int bands0 = valid_bands(g.H, rb_max);
  v.rb = ceil_div(g.H, bands0);
  const int bands = ceil_div(g.H, v.rb);
  v.npix = v.rb * g.W;
  const int rows = std::min(g.H, v.rb + 2 * R);
  v.S = (rows * g.W) | 1;
  constexpr int PROD = (FAM == 1 || FAM == 2) ? 1 : 0;
  const int head = (((FAM == 2 ? 2 * N : N) + 1) * v.npix + 3) & ~3;   // wt (cosine: and the pairs' cosines) and dg in front of the slab
  // channel blocks along grid.z where bands and batch leave CUs idle: at least 32 channels each
  const int nz0 = std::max(1, std::min(ceil_div(512, bands * g.B), g.C / 32));
  v.Cz = nz0 > 1 ? ceil_div(ceil_div(g.C, nz0), 8) * 8 : g.C;
  const int nz = ceil_div(g.C, v.Cz);
  v.Cc = valid_even_chunk(v.Cz, (kValidLdsFloats - head) / v.S, 8);
  v.G = std::max(1, std::min(std::min(16, ceil_div(std::min(v.Cc, g.C), 4)), kValidBwdT / v.npix));
  const int T = std::min(kValidBwdT, (v.G * v.npix + 63) & ~63);
  v.vec = (!nhwc && g.W % ve == 0 && g.sB % ve == 0 && aligned16(x)) ? 1 : 0;
  const size_t lds = sizeof(float) * (size_t)(head + round4(v.Cc) * v.S);
  snprintf(g_variant, sizeof(g_variant), "bwd_valid<%d,%s,%s,%s>", R, FAM == 3 ? "l1" : (PROD ? "prod" : "dist"), bf ? "bf16" : "f32",
           nhwc ? "nhwc" : "nchw");
  const dim3 grid((unsigned)bands, (unsigned)g.B, (unsigned)nz), block(T);
  return with_storage(g, [&](auto bf_, auto nhwc_) {
    return launch("bwd_valid", nfp::bwd_valid<R, FAM, bf_(), nhwc_()>, grid, block, lds, st, g, v, x, go, out, saved, gx);
  });
}

int valid_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st) {
  if (const char* why = valid_refusal(g)) return fail(NFP_E_UNSUPPORTED, "valid maps: %s", why);
  return with_radius(g, [&](auto r) {
    return with_hot(g, [&](auto m) {   // PROD: the product form
      return valid_forward_rp<decltype(r)::value, m() == NFP_COSINE ? 1 : 0>(g, x, out, saved, st);
    });
  });
}

int valid_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st) {
  if (const char* why = valid_refusal(g)) return fail(NFP_E_UNSUPPORTED, "valid maps: %s", why);
  return with_radius(g, [&](auto r) {
    return with_hot(g, [&](auto m) {   // FAM: 0 the distances, 1 dot / gfc, 2 cosine (the pairs' cosines are kept too)
      constexpr int R = decltype(r)::value;
      if constexpr (m() == NFP_COSINE)
        return g.measure == NFP_COSINE ? valid_backward_rp<R, 2>(g, x, go, out, saved, gx, st)
                                       : valid_backward_rp<R, 1>(g, x, go, out, saved, gx, st);
      else
        return valid_backward_rp<R, 0>(g, x, go, out, saved, gx, st);
    });
  });
}

// the L1 family: no `out`, no `saved` (null to the kernels, which never read them)
int valid_abs_forward(const KP& g, const void* x, void* out, hipStream_t st) {
  if (const char* why = valid_abs_refusal(g)) return fail(NFP_E_UNSUPPORTED, "valid L1 maps: %s", why);
  return with_radius(g, [&](auto r) { return valid_forward_rp<decltype(r)::value, 2>(g, x, out, nullptr, st); });
}

int valid_abs_backward(const KP& g, const void* x, const void* go, void* gx, hipStream_t st) {
  if (const char* why = valid_abs_refusal(g)) return fail(NFP_E_UNSUPPORTED, "valid L1 maps: %s", why);
  return with_radius(g, [&](auto r) { return valid_backward_rp<decltype(r)::value, 3>(g, x, go, nullptr, nullptr, gx, st); });
}

}  // namespace nfp_host
