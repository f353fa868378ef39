// nfp_strided.hip — NFP maps at STRIDE 2 to 4: dilation 1, R = 1 or 2, padding 0 or R with zeros / reflect / replicate
// (include/nfp.h: nfp_strided_*).  The `--nfp_stride` layers of RESNET18_NFP_AT_LAYER, *_NFP_CONV_ONLY / _CONV_MLP and
// MOBILENETV3_NFP_INSERT (demo.py: nfp_kwargs).  Output (i, j) has its centre at padded position (s i + R, s j + R) — input
// pixel (s i + R - P, s j + R - P); Ho = (H + 2P - 2R - 1) / s + 1, Wo likewise.  The stride is a run-time, wave-uniform
// value; no tables, no workspace, one launch each way, no atomics.
//
// Both kernels work on the PADDED band the reference's F.pad would build (nfp_tile.h::Fold: a ring position is a second copy
// of an image pixel, a zero-padded one a zero vector), staged in LDS as float32, channel-major (xs[c * S + position], S
// odd), in chunks of Cc channels: every tap sits at a constant offset from its centre.  16-byte global loads where rows
// and pointers allow (NCHW: whole image rows, the 2P ring columns of a row one by one; channels-last: every position).
//
// Forward, fwd_strided<R, PROD, BF, NHWC>: one workgroup per (image, band of rb output rows); staged: the padded rows
// [s i0, s (i1 - 1) + 2R].  FULL stencil — at stride >= 2 almost no pair is shared between two outputs: thread (grp, o) owns
// output o of the band and sums its N taps (products x_u . x_t, or |x_u - x_t|^2) over the channels c = grp, grp + G, ...
// of every chunk, in registers.  The squared norms (cosine / gfc) are taken once per staged position, by threads of their
// own (G2 channel groups), not once per tap.  The groups' partial sums are joined through LDS in group order by the one
// thread that finishes the (output, tap) (nfp_valid.h::valid_fin: the one-division cosine, else Meas<>::fin).  An output
// element has one writer.  `saved` gets |x| of EVERY input pixel: a band owns the padded rows from its first to the next
// band's first (the last band: to the end); the rows of those it has not staged — no window reads them: s > 2R + 1, or the
// trailing rows — it sums straight from memory.
//
// Backward, bwd_strided<R, FAM, BF, NHWC>: the gather form of bwd_valid with "is a centre" in place of "is interior"; one
// workgroup per (image, band of image rows, channel block).  A band EVALUATES the padded positions of its own rows (ring
// columns included) and — first / last band, reflect / replicate — of the ring rows above / below the image, whose fold
// sources lie in it (every band has at least R + 1 rows, or there is one band).  Slot j of padded position u joins the
// coefficient of the output centred at u with tap j (u a centre) and the one of the output centred at u + d_j with the
// opposite tap (u + d_j a centre): Meas<>::coef of grad_out, out and the saved norms, read under those two predicates
// only.  A position is a centre when (u - R) is divisible by s on both axes with the quotient inside [0, Ho) x [0, Wo):
// two small LDS tables (padded row -> output row or -1, padded column -> output column or -1), so that no thread divides.
//   phase A   one thread per evaluated position: its N slots, its diagonal and whether any slot is present, to LDS
//   phase B   thread (u, grp), the N slots in registers, over the channel quads grp, grp + G, ... of the staged chunk:
//               dot, gfc   r[c][u] = sum_j Wt[j][u] xpad[c][u + d_j] + diag[u] xpad[c][u]
//               cosine     the projected form of bwd_valid on unit vectors
//               distances  r[c][u] = sum_j Wt[j][u] (xpad[c][u] - xpad[c][u + d_j])
//             into a second LDS slab r[c][u]; a position without a present slot writes an explicit 0
//   store     one thread per (channel, own pixel) — channels-last: per (own pixel, channel quad) — adds to r[c][pixel]
//             what the ring positions that fold onto the pixel collected, in a fixed order (a bit mask per pixel, built
//             once), and stores grad_x: fully overwritten, zeros where no window reaches.
// Every sum in a fixed order: two runs agree bitwise and image b's results do not depend on B.  lds_poison() at entry.
//
// Bank layout: a wavefront's outputs lie s positions apart in the slab — a 2-way (s = 2) to 4-way (s = 4) conflict on the
// forward's tap reads, accepted here (the channel groups of a wavefront are S apart, S odd); the backward reads positions
// side by side.
#include "nfp_tile.h"    // (Fold, lds_poison)
#include "nfp_valid.h"   // (ldv, tap_of, valid_fin, valid_coef, the layout predicates)

namespace nfp {
namespace {

constexpr int kStridedT = 1024;   // threads of a workgroup at most: 16 wavefronts, 128 registers each

struct SG {          // by value in kernarg
  int Hp, Wp;        // the padded image: H + 2P, W + 2P
  int S;             // floats between two channels of the staged slab (odd)
  int Cc, G, vec;    // channels per chunk; channel groups (forward: channels, backward: quads); 16-byte loads of NCHW rows
  int ldsw;          // 32-bit words of dynamic LDS (lds_poison)
  // forward
  int rb, npix, no;  // output rows per band; staged positions and outputs of a full band
  int G2, n2w;       // channel groups of the norm sums; floats of their partial sums in front of the slab
  // backward
  int nb, hq, hr;    // bands per image: H = nb * hq + hr, the first hr bands one row more
  int er, EP;        // evaluated rows and positions of the largest band
  int SPn;           // staged positions of the largest band
  int own;           // own pixels of the largest band
  int Sr, Cz;        // floats between two channels of the result slab (odd); channels per workgroup along grid.z
};

__device__ __forceinline__ void unpack16(const uint4& w, float* d, int st, bool bf) {
  if (bf) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[(2 * k) * st] = __uint_as_float(u[k] << 16);
      d[(2 * k + 1) * st] = __uint_as_float(u[k] & 0xffff0000u);
    }
  } else {
    d[0] = __uint_as_float(w.x);
    d[st] = __uint_as_float(w.y);
    d[2 * st] = __uint_as_float(w.z);
    d[3 * st] = __uint_as_float(w.w);
  }
}

// padded rows [pr0, pr0 + rows) of image b, every padded column, channels [c0, c0 + cc) -> xs[c * S + (pr - pr0) * Wp + pc]
template <int BF, int NHWC>
__device__ __forceinline__ void stage_padded(const KP& g, const SG& v, const Fold& fo, const void* x, long long img, int pr0,
                                             int rows, int c0, int cc, float* xs, int tid, int T) {
  const int Wp = v.Wp, P = g.pad, W = g.W, H = g.H;
  constexpr int VE = BF ? 8 : 4, ES = BF ? 2 : 4;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  if (NHWC) {
    // [pixel][c]: 16 bytes = VE adjacent channels of the position's fold source (C % VE == 0, images 16-byte aligned)
    const int cq = cc / VE, len = rows * Wp;
    for (int it = tid; it < len * cq; it += T) {
      const int p = it / cq, q = it - p * cq;
      const int py = p / Wp, px = p - py * Wp;
      const int sy = fo.y(pr0 + py - P, H), sx = fo.x(px - P, W);
      uint4 w = zero4;
      if ((sy | sx) >= 0) w = *(const uint4*)((const char*)x + (img + ((long long)sy * W + sx) * g.C + c0 + q * VE) * ES);
      unpack16(w, xs + (q * VE) * v.S + p, v.S, BF);
    }
    return;
  }
  const long long base = img + (long long)c0 * g.sC;
  if (v.vec) {
    // whole image rows (a ring row: its fold source's) by 16-byte loads, then the 2P ring columns of every row
    const int wq = W / VE, per = rows * wq;
    for (int it = tid; it < cc * per; it += T) {
      const int c = it / per, r2 = it - c * per, py = r2 / wq, q = r2 - py * wq;
      const int sy = fo.y(pr0 + py - P, H);
      uint4 w = zero4;
      if (sy >= 0) w = *(const uint4*)((const char*)x + (base + (long long)c * g.sC + (long long)sy * W + q * VE) * ES);
      unpack16(w, xs + c * v.S + py * Wp + P + q * VE, 1, BF);
    }
    const int perc = rows * 2 * P;   // (P == 0: no ring, no iteration)
    for (int it = tid; it < cc * perc; it += T) {
      const int c = it / perc, r2 = it - c * perc, py = r2 / (2 * P), j = r2 - py * (2 * P);
      const int px = j < P ? j : W + j;
      const int sy = fo.y(pr0 + py - P, H), sx = fo.x(px - P, W);
      xs[c * v.S + py * Wp + px] = (sy | sx) >= 0 ? ldv<BF>(x, base + (long long)c * g.sC + (long long)sy * W + sx) : 0.f;
    }
    return;
  }
  const int len = rows * Wp;
  for (int it = tid; it < cc * len; it += T) {
    const int c = it / len, p = it - c * len, py = p / Wp, px = p - py * Wp;
    const int sy = fo.y(pr0 + py - P, H), sx = fo.x(px - P, W);
    xs[c * v.S + p] = (sy | sx) >= 0 ? ldv<BF>(x, base + (long long)c * g.sC + (long long)sy * W + sx) : 0.f;
  }
}

template <int BF>
__device__ __forceinline__ void stv(void* p, long long i, float val) {
  if (BF)
    ((uint16_t*)p)[i] = f32_to_bf16(val);
  else
    ((float*)p)[i] = val;
}

// grid = (bands, B).  Dynamic LDS (floats): n2[G2][npix] (products) | max(Cc * S, G * N * no): the slab, then the groups'
// partial pair sums.  PROD: 0 squared differences, 1 products
template <int R, int PROD, int BF, int NHWC>
__global__ void __launch_bounds__(kStridedT) fwd_strided(KP g, SG v, const void* __restrict__ x, void* __restrict__ out,
                                                         float* __restrict__ saved) {
  extern __shared__ __attribute__((aligned(16))) float slds[];
  lds_poison(slds, v.ldsw);
  constexpr int K = 2 * R + 1, N = K * K - 1;
  const int tid = threadIdx.x, T = blockDim.x, Wp = v.Wp, s = g.stride, P = g.pad;
  const int b = blockIdx.y, i0 = blockIdx.x * v.rb;          // first output row of the band
  const int rb = min(v.rb, g.Ho - i0), rin = s * (rb - 1) + K, npix = rin * Wp, no = rb * g.Wo;
  const int pr0 = s * i0;                                    // first staged padded row
  const Fold fo(g);
  const long long img = (long long)b * g.sB;
  const bool stats = PROD && g.measure != NFP_DOT;           // (wave-uniform)
  float* n2p = slds;
  float* xs = slds + v.n2w;
  const int grp = tid / v.no, o = tid - grp * v.no;
  const bool act = grp < v.G && o < no;
  const int oi = o / g.Wo, oj = o - oi * g.Wo;
  const int uc = act ? (s * oi + R) * Wp + s * oj + R : 0;   // the output's centre inside the staged rows
  float acc[N];
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n] = 0.f;
  if (stats)
    for (int it = tid; it < v.G2 * v.npix; it += T) n2p[it] = 0.f;
  for (int c0 = 0; c0 < g.C; c0 += v.Cc) {
    const int cc = min(v.Cc, g.C - c0);
    if (c0 > 0) __syncthreads();   // (the previous chunk has been summed)
    stage_padded<BF, NHWC>(g, v, fo, x, img, pr0, rin, c0, cc, xs, tid, T);
    __syncthreads();
    if (stats) {
      // |x_u|^2 once per staged position: item (g2, u) stays with its thread from chunk to chunk
      for (int it = tid; it < v.G2 * npix; it += T) {
        const int g2 = it / npix, u = it - g2 * npix;
        float a = n2p[g2 * v.npix + u];
        for (int c = g2; c < cc; c += v.G2) {
          const float t = xs[c * v.S + u];
          a = fmaf(t, t, a);
        }
        n2p[g2 * v.npix + u] = a;
      }
    }
    if (act) {
#pragma unroll 2
      for (int c = grp; c < cc; c += v.G) {
        const float* xc = xs + c * v.S + uc;
        const float a = xc[0];
#pragma unroll
        for (int n = 0; n < N; ++n) {
          int dy, dx;
          tap_of<R>(n, dy, dx);
          const float t = xc[dy * Wp + dx];
          if (PROD) {
            acc[n] = fmaf(a, t, acc[n]);
          } else {
            const float d = a - t;
            acc[n] = fmaf(d, d, acc[n]);
          }
        }
      }
    }
  }
  __syncthreads();   // (the slab has been read: the partial sums take its place; the norm sums are complete)
  float* pr = xs;    // pr[(grp * N + n) * v.no + o]
  if (act) {
#pragma unroll
    for (int n = 0; n < N; ++n) pr[(grp * N + n) * v.no + o] = acc[n];
  }
  if (stats && v.G2 > 1) {
    for (int u = tid; u < npix; u += T) {
      float a = n2p[u];
      for (int q = 1; q < v.G2; ++q) a += n2p[q * v.npix + u];
      n2p[u] = a;   // (group 0's slot of a position is read and written by this thread alone)
    }
  }
  __syncthreads();
  // |x| per input pixel for the backward: this band's padded rows [pr0, the next band's first), the last band's to the end
  if (stats && saved != nullptr) {
    const int own1 = blockIdx.x == gridDim.x - 1 ? v.Hp : pr0 + s * v.rb;
    float* sv = saved + (long long)b * g.P;
    for (int it = tid; it < (own1 - pr0) * g.W; it += T) {
      const int ry = it / g.W, xx = it - ry * g.W, y = pr0 + ry - P;
      if (y < 0 || y >= g.H) continue;   // (a ring row)
      float n2;
      if (ry < rin) {
        n2 = n2p[ry * Wp + xx + P];
      } else {   // a row no window of this band reads
        n2 = 0.f;
        for (int c = 0; c < g.C; ++c) {
          const float t = ldv<BF>(x, img + (long long)c * g.sC + (long long)y * g.sH + (long long)xx * g.sW);
          n2 = fmaf(t, t, n2);
        }
      }
      sv[y * g.W + xx] = sqrtf(n2);
    }
  }
  // one thread per (tap, output of the band): the groups joined in order, out[b][n][i0 * Wo + ol]
  const long long obase = (long long)b * N * g.O + (long long)i0 * g.Wo;
  for (int it = tid; it < N * no; it += T) {
    const int n = it / no, ol = it - n * no;
    const int oi2 = ol / g.Wo, oj2 = ol - oi2 * g.Wo;
    int dy, dx;
    tap_of<R>(n, dy, dx);
    const int u2 = (s * oi2 + R) * Wp + s * oj2 + R, q2 = u2 + dy * Wp + dx;
    float pairv = pr[n * v.no + ol];
    for (int q = 1; q < v.G; ++q) pairv += pr[(q * N + n) * v.no + ol];
    const float val = valid_fin<PROD>(g, pairv, stats ? n2p[u2] : 0.f, stats ? n2p[q2] : 0.f);
    stv<BF>(out, obase + (long long)n * g.O + ol, val);
  }
}

// Where the backward's LDS regions start (floats), from the launch's sizes: the same arithmetic on host and device
struct BwdLds {
  int sv, dg, tch, cm, ns, rowc, colc, xs, res, total;
  __host__ __device__ BwdLds(const SG& v, int N, int NW, int R) {
    sv = N * v.EP;            // (cosine: the pairs' cosines behind the weights)
    dg = NW * v.EP;
    tch = dg + v.EP;
    cm = tch + v.EP;
    ns = cm + v.own;
    rowc = ns + v.SPn;
    colc = rowc + v.er + 2 * R;
    xs = (colc + v.Wp + 2 * R + 3) & ~3;
    res = xs + ((v.Cc + 3) & ~3) * v.S;
    total = res + v.Cc * v.Sr;
  }
};

// grid = (bands, B, channel blocks).  Dynamic LDS: BwdLds.  FAM: 0 distances, 1 dot / gfc, 2 cosine in the projected form
// (nfp_valid.hip::bwd_valid).  Every channel block repeats phase A; the blocks' results are those of one workgroup
// walking all channels, bit for bit.
template <int R, int FAM, int BF, int NHWC>
__global__ void __launch_bounds__(kStridedT) bwd_strided(KP g, SG v, const void* __restrict__ x, const void* __restrict__ go,
                                                         const void* __restrict__ outm, const float* __restrict__ saved,
                                                         void* __restrict__ gx) {
  extern __shared__ __attribute__((aligned(16))) float slds[];
  lds_poison(slds, v.ldsw);
  constexpr int K = 2 * R + 1, N = K * K - 1;
  constexpr int PROD = (FAM == 1 || FAM == 2) ? 1 : 0;
  constexpr int NW = FAM == 2 ? 2 * N : N;
  const int tid = threadIdx.x, T = blockDim.x, W = g.W, H = g.H, Wp = v.Wp, s = g.stride, P = g.pad;
  const int b = blockIdx.y, band = blockIdx.x;
  const int y0 = band * v.hq + min(band, v.hr), y1 = (band + 1) * v.hq + min(band + 1, v.hr);   // own image rows
  const int ring = g.mode == NFP_PAD_ZEROS ? 0 : P;   // (the gradient of a zero padding belongs to nobody)
  const int e0 = y0 + P - (band == 0 ? ring : 0), e1 = y1 + P + (band == v.nb - 1 ? ring : 0);   // evaluated padded rows
  const int EPn = (e1 - e0) * Wp;
  const int sp0 = max(e0 - R, 0), sp1 = min(e1 + R, v.Hp), srows = sp1 - sp0, SPn = srows * Wp;   // staged padded rows
  const int nown = (y1 - y0) * W;
  const BwdLds L(v, N, NW, R);
  float* wt = slds;
  float* sv = slds + L.sv;
  float* dg = slds + L.dg;
  int* tch = (int*)(slds + L.tch);
  int* cm = (int*)(slds + L.cm);
  float* ns = slds + L.ns;
  int* rowc = (int*)(slds + L.rowc);
  int* colc = (int*)(slds + L.colc);
  float* xs = slds + L.xs;
  float* res = slds + L.res;
  const Fold fo(g);
  const long long img = (long long)b * g.sB;
  const long long mbase = (long long)b * N * g.O;
  const bool stats = PROD && g.measure != NFP_DOT;
  // ---- tables: padded row / column -> output row / column or -1; the norm of every staged position; the ring positions
  // that fold onto every own pixel
  for (int k = tid; k < e1 - e0 + 2 * R; k += T) {
    const int t = e0 - R + k - R;   // (padded row e0 - R + k, measured from the first centre)
    const int q = t >= 0 ? t / s : -1;
    rowc[k] = (t >= 0 && q * s == t && q < g.Ho) ? q : -1;
  }
  for (int k = tid; k < Wp + 2 * R; k += T) {
    const int t = k - 2 * R;        // (padded column k - R)
    const int q = t >= 0 ? t / s : -1;
    colc[k] = (t >= 0 && q * s == t && q < g.Wo) ? q : -1;
  }
  if (stats) {
    const float* nrm = saved + (long long)b * g.P;
    for (int p = tid; p < SPn; p += T) {
      const int py = p / Wp, px = p - py * Wp;
      const int sy = fo.y(sp0 + py - P, H), sx = fo.x(px - P, W);
      ns[p] = (sy | sx) >= 0 ? nrm[sy * W + sx] : 0.f;
    }
  }
  for (int r = tid; r < nown; r += T) {
    const int ry = r / W, y = y0 + ry, xx = r - ry * W;
    int m = 0;
    if (ring > 0) {   // (then P == R)
      for (int a = 0; a < K; ++a) {
        const int yy = a == 0 ? y : (a <= R ? -a : H + a - R - 1);
        if (a > 0 && fo.y(yy, H) != y) continue;
        for (int c = 0; c < K; ++c) {
          const int x2 = c == 0 ? xx : (c <= R ? -c : W + c - R - 1);
          if ((a | c) != 0 && (c == 0 || fo.x(x2, W) == xx)) m |= 1 << (a * K + c);
        }
      }
    }
    cm[r] = m;
  }
  __syncthreads();
  // ---- phase A: the N slots, the diagonal and "any slot present" of every evaluated position
  for (int u = tid; u < EPn; u += T) {
    const int ur = u / Wp, px = u - ur * Wp;
    const int lp = (e0 + ur - sp0) * Wp + px;   // the position inside the staged rows
    const int ci = rowc[ur + R], cj = colc[px + R];
    const bool in_r = (ci | cj) >= 0;
    const int o_r = ci * g.Wo + cj;
    const float n_r = stats ? ns[lp] : 0.f;
    float dsum = 0.f;
    bool any = in_r;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      int dy, dx;
      tap_of<R>(j, dy, dx);
      const int ti = rowc[ur + R + dy], tj = colc[px + R + dx];
      const bool in_t = (ti | tj) >= 0;
      const int o_t = ti * g.Wo + tj;
      any = any || in_t;
      float w = 0.f;
      if (FAM == 2) {
        // the pair's grad_out from both orientations and its one cosine (fwd_strided finishes both orientations alike)
        float gsum = 0.f, sj = g.similarity ? 0.f : 1.f;
        if (in_r) {
          const long long i = mbase + (long long)j * g.O + o_r;
          gsum += ldv<BF>(go, i);
          sj = ldv<BF>(outm, i);
        }
        if (in_t) {
          const long long i = mbase + (long long)(N - 1 - j) * g.O + o_t;
          gsum += ldv<BF>(go, i);
          sj = ldv<BF>(outm, i);
        }
        w = g.similarity ? gsum : -gsum;
        sv[j * v.EP + u] = g.similarity ? sj : 1.f - sj;
      } else if (in_r || in_t) {   // (then u + d_j is a position of the padded image, staged)
        const float n_t = stats ? ns[lp + dy * Wp + dx] : 0.f;
        if (in_r) {
          const long long i = mbase + (long long)j * g.O + o_r;
          const Coef cf = valid_coef<PROD>(g, ldv<BF>(go, i), ldv<BF>(outm, i), n_r, n_t);
          w += cf.k0;
          dsum += cf.k1;
        }
        if (in_t) {
          const long long i = mbase + (long long)(N - 1 - j) * g.O + o_t;
          const Coef cf = valid_coef<PROD>(g, ldv<BF>(go, i), ldv<BF>(outm, i), n_t, n_r);
          w += cf.k0;
          dsum += cf.k2;
        }
      }
      wt[j * v.EP + u] = w;
    }
    dg[u] = -dsum;
    tch[u] = any ? 1 : 0;
  }
  // ---- phase B
  const int grp = tid / v.EP, u = tid - grp * v.EP;
  const bool act = u < EPn && grp < v.G;
  const int ur = u / Wp, px = u - ur * Wp;
  const int lp = (e0 + ur - sp0) * Wp + px;
  float wr[N], sr[FAM == 2 ? N : 1], dr = 0.f, ir = 0.f, rho = 0.f;
  int off[N];
  bool touched = false;
  __syncthreads();   // (wt, sv, dg and tch are complete)
#pragma unroll
  for (int j = 0; j < N; ++j) {
    int dy, dx;
    tap_of<R>(j, dy, dx);
    const int py = e0 + ur + dy;
    const bool ok = act && py >= sp0 && py < sp1 && px + dx >= 0 && px + dx < Wp;
    off[j] = ok ? dy * Wp + dx : 0;              // (past the padded image the slot is absent: any staged address serves)
    wr[j] = act ? wt[j * v.EP + u] : 0.f;
    if (FAM == 2) sr[j] = act ? sv[j * v.EP + u] : 0.f;
  }
  if (act) {
    dr = dg[u];
    touched = tch[u] != 0;
  }
  if (FAM == 2 && act) {
    const float n = ns[lp], m = fmaxf(n, g.eps);
    ir = 1.f / m;
    rho = n > 0.f ? m / n : 0.f;   // (exactly 1 above eps)
  }
  const long long gimg = (long long)b * g.gB;
  const int cbeg = blockIdx.z * v.Cz, cend = min(g.C, cbeg + v.Cz);   // this workgroup's channels
  for (int c0 = cbeg; c0 < cend; c0 += v.Cc) {
    const int cc = min(v.Cc, cend - c0);
    // (the slab is free: every thread has passed the barrier behind the previous chunk's sums)
    stage_padded<BF, NHWC>(g, v, fo, x, img, sp0, srows, c0, cc, xs, tid, T);
    __syncthreads();   // (... and the previous chunk's results have been stored)
    if (FAM == 2) {    // xn = x / max(|x|, eps): a correctly rounded division
      for (int it = tid; it < cc * SPn; it += T) {
        const int c = it / SPn, p = it - c * SPn;
        xs[c * v.S + p] = xs[c * v.S + p] / fmaxf(ns[p], g.eps);
      }
      __syncthreads();
    }
    if (act) {
      for (int cq = grp; 4 * cq < cc; cq += v.G) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float* xc = xs + (4 * cq + k) * v.S + lp;   // (channels past cc: inside the slab's round4(Cc) rows, not kept)
          const float a = xc[0];
          float t = FAM == 1 ? dr * a : 0.f;
          if (FAM == 2) {
            const float un = rho * a;
#pragma unroll
            for (int j = 0; j < N; ++j) t = fmaf(wr[j], fmaf(-sr[j], un, xc[off[j]]), t);
            t *= ir;
          } else {
#pragma unroll
            for (int j = 0; j < N; ++j) t = PROD ? fmaf(wr[j], xc[off[j]], t) : fmaf(wr[j], a - xc[off[j]], t);
          }
          if (4 * cq + k < cc) res[(4 * cq + k) * v.Sr + u] = touched ? t : 0.f;
        }
      }
    }
    __syncthreads();   // (the results of every evaluated position)
    // ---- store: an own pixel's result and what its ring copies collected, in ascending order of the mask's bits
    auto gather = [&](int c, int r, int y, int xx) {
      float t = res[c * v.Sr + (y + P - e0) * Wp + xx + P];
      int m = cm[r];
      while (m) {
        const int bit = __ffs(m) - 1;
        m &= m - 1;
        const int a = bit / K, cb = bit - a * K;
        const int yy = a == 0 ? y : (a <= R ? -a : H + a - R - 1);
        const int x2 = cb == 0 ? xx : (cb <= R ? -cb : W + cb - R - 1);
        t += res[c * v.Sr + (yy + P - e0) * Wp + x2 + P];
      }
      return t;
    };
    if (NHWC) {
      const int nq = cc >> 2;   // (C % 4 == 0 and chunks of 8: the quads are whole)
      for (int it = tid; it < nown * nq; it += T) {
        const int r = it / nq, q = it - r * nq, ry = r / W, xx = r - ry * W, y = y0 + ry;
        float a4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a4[k] = gather(4 * q + k, r, y, xx);
        const long long i = gimg + ((long long)y * W + xx) * g.C + c0 + 4 * q;
        if (BF) {
          uint2 pk;
          pk.x = f32_to_bf16x2(a4[0], a4[1]);
          pk.y = f32_to_bf16x2(a4[2], a4[3]);
          *(uint2*)((uint16_t*)gx + i) = pk;
        } else {
          *(float4*)((float*)gx + i) = make_float4(a4[0], a4[1], a4[2], a4[3]);
        }
      }
    } else {
      for (int it = tid; it < cc * nown; it += T) {
        const int c = it / nown, r = it - c * nown, ry = r / W, xx = r - ry * W, y = y0 + ry;
        stv<BF>(gx, gimg + (long long)(c0 + c) * g.P + (long long)y * W + xx, gather(c, r, y, xx));
      }
    }
  }
}

}  // namespace
}  // namespace nfp

namespace nfp_host {
namespace {

constexpr int kStridedMaxWp = 128;   // W + 2P at most
constexpr int kStridedFwdPix = 1250;   // staged positions of a forward band at most: 16 channels of them per chunk

}  // namespace

// measure, geometry and layout: what lies outside the kernels' set, or null
const char* strided_refusal(const KP& g) {
  if (!hot_measure(g)) return "cosine / dot / gfc / L2 (norm p=2) / rmse only";
  if (!hot_product(g) && !g.diff) return "a distance on the pure-neighbour weights";
  if (g.rs == 12) return "one radius per call (inner_R = 0)";
  if (mixed_maps(g)) return "maps in the storage type (map_f32 = 0)";
  if (g.stride < 2 || g.stride > 4) return "stride 2 to 4";
  if (g.dil != 1) return "dilation 1";
  if (g.R != 1 && g.R != 2) return "R = 1 or 2";
  if (g.pad != 0 && g.pad != g.R) return "padding 0 or R";
  if (g.pad != 0 && g.mode == NFP_PAD_CIRCULAR) return "zeros / reflect / replicate padding";
  if (g.W + 2 * g.pad > kStridedMaxWp) return "padded rows of more than 128 positions";
  if (!valid_nchw(g) && !valid_nhwc(g)) return "images dense in NCHW or channels-last order";
  if (!valid_nchw(g) && g.C % valid_ve(g) != 0) return "channels-last maps with C % 4 (float32) / C % 8 (bf16) != 0";
  if (!valid_nchw(g) && (g.sB % valid_ve(g) != 0 || g.gB % valid_ve(g) != 0)) return "channels-last images off 16-byte boundaries";
  return nullptr;
}

namespace {

const char* strided_fam(int fam_prod) { return fam_prod ? "prod" : "dist"; }

template <int R, int PROD>
int strided_forward_rp(const KP& g, const void* x, void* out, float* saved, hipStream_t st) {
  constexpr int K = 2 * R + 1, N = K * K - 1;
  const bool nhwc = !valid_nchw(g), bf = g.dtype == NFP_BF16;
  const int ve = valid_ve(g), s = g.stride;
  if (nhwc && !aligned16(x)) return fail(NFP_E_UNSUPPORTED, "strided maps: channels-last images off 16-byte boundaries");
  SG v = {};
  v.Hp = g.H + 2 * g.pad;
  v.Wp = g.W + 2 * g.pad;
  // Bands of at most 8 output rows, fewer where the threads (one per output) or the slab (16 channels of a band per chunk)
  // ask for it.  NOT a function of the batch: the band sets the channel groups, and with them the order of the sums.
  constexpr int ocap = R == 1 ? kStridedT : 768;   // (output, group) threads at most: their N partial sums share the slab's LDS
  int rb_max = 1;
  while (rb_max < 8 && (rb_max + 1) * g.Wo <= ocap && (s * rb_max + K) * v.Wp <= kStridedFwdPix) ++rb_max;
  v.rb = ceil_div(g.Ho, ceil_div(g.Ho, rb_max));
  const int bands = ceil_div(g.Ho, v.rb);
  v.npix = (s * (v.rb - 1) + K) * v.Wp;
  v.S = v.npix | 1;
  v.no = v.rb * g.Wo;
  v.G = std::max(1, std::min(std::min(32, g.C), ocap / v.no));
  const int T = std::min(kStridedT, (v.G * v.no + 63) & ~63);
  v.G2 = std::max(1, std::min(std::min(8, g.C), T / v.npix));
  v.n2w = PROD ? round4(v.G2 * v.npix) : 0;
  v.Cc = valid_even_chunk(g.C, (nfp::kValidLdsFloats - v.n2w) / v.S, 8);
  v.vec = (!nhwc && g.W % ve == 0 && g.sB % ve == 0 && aligned16(x)) ? 1 : 0;
  v.ldsw = v.n2w + std::max(v.Cc * v.S, v.G * N * v.no);
  snprintf(g_variant, sizeof(g_variant), "fwd_strided<%d,%s,%s,%s>", R, strided_fam(PROD), bf ? "bf16" : "f32", nhwc ? "nhwc" : "nchw");
  const dim3 grid((unsigned)bands, (unsigned)g.B), block(T);
  return with_storage(g, [&](auto bf_, auto nhwc_) {
    return launch("fwd_strided", nfp::fwd_strided<R, PROD, bf_(), nhwc_()>, grid, block, sizeof(float) * (size_t)v.ldsw, st, g, v, x,
                  out, saved);
  });
}

template <int R, int FAM>
int strided_backward_rp(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx,
                        hipStream_t st) {
  constexpr int K = 2 * R + 1, N = K * K - 1, NW = FAM == 2 ? 2 * N : N;
  constexpr int PROD = (FAM == 1 || FAM == 2) ? 1 : 0;
  const bool nhwc = !valid_nchw(g), bf = g.dtype == NFP_BF16;
  const int ve = valid_ve(g), P = g.pad;
  if (nhwc && (!aligned16(x) || !aligned16(gx)))
    return fail(NFP_E_UNSUPPORTED, "strided maps: channels-last images off 16-byte boundaries");
  SG v = {};
  v.Hp = g.H + 2 * P;
  v.Wp = g.W + 2 * P;
  // Bands of about 8 image rows: one thread per evaluated position (R = 2: half as many, its 24 slots cost the registers
  // and the LDS), and — with a ring — at least R + 1 rows each, so that a ring row's fold source lies in the first / last band
  const int cap = R == 1 ? kStridedT : kStridedT / 2;
  int rb_max = std::max(1, cap / v.Wp - 2 * P);
  // ... and fewer rows while the slots of a band and 8 channels of its two slabs exceed half a CU's LDS
  const int rb_min = P > 0 ? R + 1 : 1;
  while (rb_max > rb_min && ((NW + 3) * (rb_max + P) + 8 * (2 * (rb_max + P) + 2 * R)) * v.Wp > nfp::kValidLdsFloats) --rb_max;
  int nb =std::max(ceil_div(g.H, rb_max), ceil_div(g.H, 8));
  if (P > 0) nb = std::min(nb, std::max(1, g.H / (R + 1)));
  v.nb = nb;
  v.hq = g.H / nb;
  v.hr = g.H % nb;
  const int rbm = v.hq + (v.hr ? 1 : 0);
  v.er = rbm + (nb == 1 ? 2 * P : P);
  v.EP = v.er * v.Wp;
  if (v.EP > kStridedT)
    return fail(NFP_E_UNSUPPORTED, "strided maps: a band of %d padded rows of %d positions exceeds a workgroup", v.er, v.Wp);
  v.SPn = std::min(v.Hp, v.er + 2 * R) * v.Wp;
  v.S = v.SPn | 1;
  v.Sr = v.EP | 1;
  v.own = rbm * g.W;
  // channel blocks along grid.z where bands and batch leave CUs idle: at least 32 channels each
  const int nz0 = std::max(1, std::min(ceil_div(512, nb * g.B), g.C / 32));
  v.Cz = nz0 > 1 ? ceil_div(ceil_div(g.C, nz0), 8) * 8 : g.C;
  const int nz = ceil_div(g.C, v.Cz);
  v.Cc = 8;
  const int head = nfp::BwdLds(v, N, NW, R).xs;
  v.Cc = valid_even_chunk(v.Cz, std::max(0, nfp::kValidLdsFloats - head) / (v.S + v.Sr), 8);
  v.G = std::max(1, std::min(std::min(16, ceil_div(std::min(v.Cc, g.C), 4)), kStridedT / v.EP));
  const int T = std::min(kStridedT, (v.G * v.EP + 63) & ~63);
  v.vec = (!nhwc && g.W % ve == 0 && g.sB % ve == 0 && aligned16(x)) ? 1 : 0;
  v.ldsw = nfp::BwdLds(v, N, NW, R).total;
  snprintf(g_variant, sizeof(g_variant), "bwd_strided<%d,%s,%s,%s>", R, strided_fam(PROD), bf ? "bf16" : "f32", nhwc ? "nhwc" : "nchw");
  const dim3 grid((unsigned)nb, (unsigned)g.B, (unsigned)nz), block(T);
  return with_storage(g, [&](auto bf_, auto nhwc_) {
    return launch("bwd_strided", nfp::bwd_strided<R, FAM, bf_(), nhwc_()>, grid, block, sizeof(float) * (size_t)v.ldsw, st, g, v, x,
                  go, out, saved, gx);
  });
}

}  // namespace

int strided_forward(const KP& g, const void* x, void* out, float* saved, hipStream_t st) {
  if (const char* why = strided_refusal(g)) return fail(NFP_E_UNSUPPORTED, "strided maps: %s", why);
  return with_radius(g, [&](auto r) {
    return with_hot(g, [&](auto m) {   // PROD: the product form
      return strided_forward_rp<decltype(r)::value, m() == NFP_COSINE ? 1 : 0>(g, x, out, saved, st);
    });
  });
}

int strided_backward(const KP& g, const void* x, const void* go, const void* out, const float* saved, void* gx, hipStream_t st) {
  if (const char* why = strided_refusal(g)) return fail(NFP_E_UNSUPPORTED, "strided maps: %s", why);
  return with_radius(g, [&](auto r) {
    return with_hot(g, [&](auto m) {   // FAM: 0 the distances, 1 dot / gfc, 2 cosine (the pairs' cosines are kept too)
      constexpr int R = decltype(r)::value;
      if constexpr (m() == NFP_COSINE)
        return g.measure == NFP_COSINE ? strided_backward_rp<R, 2>(g, x, go, out, saved, gx, st)
                                       : strided_backward_rp<R, 1>(g, x, go, out, saved, gx, st);
      else
        return strided_backward_rp<R, 0>(g, x, go, out, saved, gx, st);
    });
  });
}

}  // namespace nfp_host
