/*
 * nfp.h — C ABI of libnfp_hip.so, the MI355X (gfx950) Neighbourhood Feature
 * Pooling forward/backward.
 *
 * The reference has no FFI layer: its operator API is the Python class
 * models/pooling/nfp.py::NFPPooling (nfp.py:15-134).  This header is the
 * boundary a binding for that class calls; every entry point names the
 * reference code it stands in for.  Plain pointers and sizes only — no torch
 * types.  All tensor pointers are DEVICE pointers; the caller owns every
 * buffer (the library never allocates, frees or retains one), kernels are
 * enqueued on the caller's hipStream_t and nothing synchronises the device.
 * Re-entrant: calls from several threads (autograd runs the backward on its own
 * thread) share only a launch counter and the lock-protected "last variant"
 * string; the error string, the dispatcher's scratch and nfp_plan's output are
 * per calling thread.  No entry point reads the environment.
 *
 * Return value of every int function: 0 = ok, <0 = NFP_E_* below (message in
 * nfp_last_error(), thread-local).  Nothing throws or aborts.
 */
#ifndef NFP_H_
#define NFP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFP_ABI_VERSION 7

/* error codes */
#define NFP_OK 0
#define NFP_E_INVALID (-1)     /* malformed descriptor / null pointer          */
#define NFP_E_UNSUPPORTED (-2) /* valid for the reference, not built here yet  */
#define NFP_E_HIP (-3)         /* a HIP runtime call failed                    */

/* nfp.py:85-120 — the `measure` string, lower-cased, dispatches to one of
 * these (same order as the if/elif chain there; 'scs' aliases 16). */
enum nfp_measure {
  NFP_NORM = 0,         /* nfp.py:141-148  LA.norm(centre-neigh, ord=p, dim=C)      */
  NFP_COSINE = 1,       /* nfp.py:150-159  F.cosine_similarity(centre, neigh, eps)  */
  NFP_DOT = 2,          /* nfp.py:161-170                                           */
  NFP_RMSE = 3,         /* nfp.py:172-179                                           */
  NFP_GEMAN = 4,        /* nfp.py:181-193                                           */
  NFP_ATTENTION = 5,    /* nfp.py:195-205  softmax over the N neighbours            */
  NFP_EMD = 6,          /* nfp.py:207-216                                           */
  NFP_CANBERRA = 7,     /* nfp.py:218-227                                           */
  NFP_HELLINGER = 8,    /* nfp.py:229-241                                           */
  NFP_CHISQUARED1 = 9,  /* nfp.py:243-252                                           */
  NFP_CHISQUARED2 = 10, /* nfp.py:254-263                                           */
  NFP_GFC = 11,         /* nfp.py:265-276                                           */
  NFP_PEARSON = 12,     /* nfp.py:278-293                                           */
  NFP_JEFFREY = 13,     /* nfp.py:295-308                                           */
  NFP_SQUAREDCHORD = 14,/* nfp.py:310-324                                           */
  NFP_SMITH = 15,       /* nfp.py:326-342                                           */
  NFP_SCS = 16,         /* nfp.py:344-374  (batch-mixing broadcast)  */
  NFP_MEASURE_COUNT = 17
};

/* nn.Conv2d padding_mode of the two frozen depthwise convs (nfp.py:42-58). */
enum nfp_pad_mode { NFP_PAD_ZEROS = 0, NFP_PAD_REFLECT = 1, NFP_PAD_REPLICATE = 2, NFP_PAD_CIRCULAR = 3 };

enum nfp_dtype { NFP_F32 = 0, NFP_BF16 = 1 }; /* storage type of x / out / grads; arithmetic is f32 */

/*
 * One NFP call.  Mirrors NFPPooling.__init__ (nfp.py:16-39) plus the input
 * geometry forward() sees (nfp.py:132-134).  Strides are in ELEMENTS, so NCHW
 * and channels-last inputs are both read in place (no transpose kernel).
 */
typedef struct nfp_desc {
  int32_t B, C, H, W;        /* input  [B,C,H,W]                                        */
  int32_t R;                 /* radius; kernel_size k = 2R+1, N = k*k-1   nfp.py:38-39  */
  int32_t pad, stride, dilation; /* conv geometry                         nfp.py:42-47  */
  int32_t pad_mode;          /* enum nfp_pad_mode                                       */
  int32_t measure;           /* enum nfp_measure                                        */
  int32_t similarity;        /* nfp.py:29 — sign / (1-x) convention of each measure     */
  int32_t diff_weights;      /* 1 when the RAW measure string was in
                                ['norm','rmse','mahalanobis'] (nfp.py:74-76): the conv
                                yields centre-neighbour; 0: pure neighbour (nfp.py:79-80) */
  int32_t dtype;             /* enum nfp_dtype                                          */
  float p;                   /* nfp.py:30 — ord of Norm, exponent of SCS                */
  float eps;                 /* nfp.py:33                                               */
  float q_scs;               /* nfp.py:34                                               */
  int64_t sxB, sxC, sxH, sxW; /* element strides of x; grad_x shares sxC / sxH / sxW    */
  int64_t sgB;               /* batch stride of grad_x in elements, 0 = sxB.  A view whose
                                images are dense but spaced apart (ViT tokens behind a class
                                token, texture_pooling.py:181-188) is read in place and still
                                gets a dense gradient                                       */
  const void* ws;            /* DEVICE pointer to the descriptor's workspace (constant tables +
                                the pooled tail's arrival counters), filled by
                                nfp_workspace_init, or NULL.  The hot-path kernels (stride 1,
                                pad = R) read their index maps from it; without it the call is
                                served by the general kernels                               */
  int32_t inner_R;           /* 0, or 1 with R = 2: ALSO produce the maps of radius 1 (padding 1)
                                from the same pass — models/nfp_heads.py:80-118 concatenates
                                NFP(R=1, padding=1) and NFP(R=2, padding=2) of one feature map.
                                out / grad_out are then [B, 8 + 24, H, W], the 8 maps of radius 1
                                first (torch.cat order).  Hot-path descriptors only (cosine / L2,
                                stride 1, padding = R, workspace set)                      */
  int32_t map_f32;           /* 0, or 1 with dtype = NFP_BF16: x / grad_x are bf16, out / grad_out (and the out
                                the backward reads) are FLOAT32 [B,N,Ho,Wo] — the call torch.autocast makes: its
                                float32 list holds cosine_similarity and linalg.norm, so a bf16 feature map yields
                                float32 maps and takes a bf16 gradient.  `saved` as before.  NFP_E_INVALID with
                                dtype = NFP_F32 or any other value; NFP_E_UNSUPPORTED (keep a float32 copy of x
                                instead) with inner_R = 1, Attention, SCS and from the nfp_bias_* calls;
                                nfp_pool_supported / nfp_gap_supported answer 0.  Additive to ABI 7: the field was
                                reserved_ (0) and no earlier library reads it.  Cosine / dot / gfc / L2 / rmse on
                                "same" maps run on the hot-path vector kernels (variant tag `mix`; not the
                                matrix-core or LDS-DMA ones), everything else on the any-geometry kernels     */
} nfp_desc;

int nfp_abi_version(void);
const char* nfp_last_error(void);

/*
 * Workspace of a descriptor: what the kernels keep between launches.  Two parts:
 *  - constant tables.  What the reference re-derives inside every conv call — which input pixel each kernel tap reads
 *    under the padding mode (nn.Conv2d's padding_mode, nfp.py:42-58) — depends only on (H, W, R, pad, stride, dilation,
 *    pad_mode), not on the batch, the channels or the data.  The hot-path kernels for maps of up to 512 pixels read it
 *    from a table instead of recomputing it per launch;
 *  - (ABI 6) one arrival counter per image for the fused pooling tail with several row bands per image: the band that
 *    finishes last adds up every band's share of the pooled sums inside the same launch (no second launch).  The
 *    counters are zero between launches; ONE nfp_pool_forward at a time may use a workspace — launches on one stream are
 *    ordered, a second stream needs a workspace of its own.
 *   bytes = nfp_workspace_bytes(d)        0 = this descriptor has neither (it is served without a workspace)
 *   nfp_workspace_init(d, ws, stream)     enqueue the fill of `ws` (>= bytes, 16-byte aligned, caller-owned)
 * then set d->ws = ws for nfp_forward / nfp_backward / nfp_pool_*.  One buffer serves every descriptor that
 * differs only in B, C, measure, similarity, dtype, strides, p, eps (the tables do not depend on them).  Without it
 * (d->ws = NULL) every call is still served: maps of up to 512 pixels by the general kernels, the pooled tail by one
 * band per image or a second, tiny launch.
 */
int64_t nfp_workspace_bytes(const nfp_desc* d);
int nfp_workspace_init(const nfp_desc* d, void* ws, void* hip_stream);

/* out is [B, N, Ho, Wo] contiguous; Ho/Wo as nn.Conv2d computes them
 * (nfp.py:125-130 is the square-only helper of the same formula). */
int nfp_output_shape(const nfp_desc* d, int32_t* N, int32_t* Ho, int32_t* Wo);

/* Floats of per-call state forward() hands to backward() (the autograd
 * "saved tensors" that replace the [B,C,N,H,W] graph of nfp.py:152-156).
 * 0 when the measure needs none. */
int64_t nfp_saved_floats(const nfp_desc* d);

/* NFPPooling.forward (nfp.py:132-134) for the measure in d.
 *   x      [B,C,H,W] by strides, dtype d->dtype
 *   out    [B,N,Ho,Wo] contiguous, dtype d->dtype (float32 when d->map_f32)
 *   saved  float[nfp_saved_floats(d)] or NULL when no backward will follow
 *          (Attention on bf16 maps always needs it: the raw dots live there) */
int nfp_forward(const nfp_desc* d, const void* x, void* out, float* saved, void* hip_stream);

/* The autograd backward of the same call: grad_x = d(sum(out*grad_out))/dx.
 *   grad_out [B,N,Ho,Wo] contiguous, the dtype of out;  out / saved as written by nfp_forward
 *   grad_x   [B,C,H,W] with the strides of x; fully overwritten */
int nfp_backward(const nfp_desc* d, const void* x, const void* grad_out, const void* out,
                 const float* saved, void* grad_x, void* hip_stream);

/*
 * Fused tail of models/NFP_Pooling.py:27-31 (the wrapper every live model uses): one pass over x yields
 *   gap  [B,C] f32 = AdaptiveAvgPool2d(1)(x)                          NFP_Pooling.py:27
 *   nfpm [B,N] f32 = adaptive_avg_pool2d(NFPPooling(x), 1)            NFP_Pooling.py:29-31
 * out_map [B,N,Ho,Wo] (dtype of x) is also written: the backward needs it, callers may ignore it.
 * ABI 6: `gap` may be NULL — MobileNetV3_MultiStageNFP / MidNFP consume adaptive_avg_pool2d(NFP(feat), 1) alone
 * (texture_pooling.py:251-252, 320-321): the channel sums are then skipped; `out_map` may be NULL when no backward will
 * follow (inference): the maps are then never stored.  nfp_pool_backward takes grad_gap = NULL likewise (GAP(x) took no
 * part in the loss): no adjoint of the mean is added.
 * Served only where nfp_pool_supported(d) != 0 — cosine / dot / gfc / L2 / rmse on "same" maps (stride 1, padding = R),
 * NCHW or channels-last, float32 or bf16: maps of at most 512 pixels with the descriptor's workspace set, larger maps
 * with rows of W <= 254 (k = 3) / W <= 142 (k = 5) pixels — (W + 2R)(3R + 1) <= 1024, one thread per padded position of
 * the smallest row band — and any height the descriptor allows (H <= 32767); the answer is a dry
 * run of both launchers, so a 1 means both nfp_pool_forward and nfp_pool_backward will launch.  Otherwise compose
 * nfp_forward with ordinary pooling.
 */
int nfp_pool_supported(const nfp_desc* d);
/* Floats of `saved` the fused tail needs: the per-pixel state of nfp_saved_floats plus, for maps served by the row-band
 * kernels (above 512 pixels), every band's share of the two pooled sums (joined in a fixed order by a second, tiny
 * launch).  nfp_pool_forward requires a non-NULL `saved` of at least this size (min 1 float). */
int64_t nfp_pool_saved_floats(const nfp_desc* d);
int nfp_pool_forward(const nfp_desc* d, const void* x, float* gap, float* nfpm, void* out_map, float* saved,
                     void* hip_stream);
/* grad_x = d( sum(gap*grad_gap) + sum(nfpm*grad_nfpm) ) / dx;  out_map / saved from nfp_pool_forward. */
int nfp_pool_backward(const nfp_desc* d, const void* x, const float* grad_gap, const float* grad_nfpm,
                      const void* out_map, const float* saved, void* grad_x, void* hip_stream);

/*
 * GAP(x) beside the FULL maps — the first step of every head of models/nfp_heads.py (NFPHead, MultiRadiusNFPHead,
 * AdaptiveFusionNFP: gap(fmap) and nfp(fmap) of one feature map, the maps then consumed by a trainable 1x1 conv): one
 * pass over x yields
 *   gap     [B,C] f32 = AdaptiveAvgPool2d(1)(x)
 *   out_map [B,N,Ho,Wo] (dtype of x) = NFPPooling(x), exactly what nfp_forward writes
 * and the backward takes BOTH gradients: grad_x = d( sum(gap*grad_gap) + sum(out_map*grad_out) ) / dx, grad_out a map as
 * in nfp_backward, grad_gap[b,c] / (H*W) added in the same store.  grad_gap may be NULL (GAP(x) took no part in the
 * loss): nothing is added and nothing is read.  No atomics: several row bands per image write partial channel sums to
 * the scratch in `saved` and a second, tiny launch joins them in band order.
 * Served where nfp_gap_supported(d) != 0 — the set of nfp_pool_supported: cosine / dot / gfc / L2 / rmse on "same" maps,
 * NCHW or channels-last, f32 or bf16; the answer is a host-only dry run of both launchers.  Otherwise compose
 * nfp_forward with an ordinary mean.
 * inner_R = 1 (radii 1 and 2 from one pass, MultiRadiusNFPHead: R = 2, pad = 2, stride 1, dilation 1) is served too:
 * out_map / grad_out are [B, 8 + 24, H, W] in torch.cat order, exactly as nfp_forward writes them for such a descriptor.
 * Its set is what both parents serve: the measures above, maps of at most 512 pixels with the descriptor's workspace set,
 * C % 4 == 0, either layout (or a batch-strided view of it), f32 or bf16 — one launch each way on the table kernels, one
 * band per image, no second launch (Norm p = 1 / EMD, which nfp_forward fuses for two radii, stay composed here;
 * nfp_pool_supported keeps answering 0 for inner_R = 1).  Additive to ABI 7 (nfp_desc is unchanged); the length convention of the bias calls:
 * `saved` comes with its length in floats, and a buffer shorter than nfp_gap_saved_floats(d) (min 1 float; the backward
 * reads the per-pixel part alone) returns NFP_E_INVALID and launches nothing.
 */
int nfp_gap_supported(const nfp_desc* d);
int64_t nfp_gap_saved_floats(const nfp_desc* d);
int nfp_gap_forward(const nfp_desc* d, const void* x, float* gap, void* out_map, float* saved, int64_t saved_floats,
                    void* hip_stream);
int nfp_gap_backward(const nfp_desc* d, const void* x, const float* grad_gap, const void* grad_out, const void* out_map,
                     const float* saved, int64_t saved_floats, void* grad_x, void* hip_stream);

/*
 * ABI 7 — NFPPooling(bias=True) (nfp.py:42-58 with bias=True: both depthwise convs carry a TRAINABLE bias, only their
 * weights are frozen, nfp.py:61,82).  The conv adds the bias after padding: a zero-padded tap reads 0 + bias.  Per pair
 * (output o, neighbour n) of channel c the measure then sees
 *   centre      a = x_c + centre_bias[c]
 *   neighbour   v = x_n + neighbour_bias[c*N + n]            (d->diff_weights: x_c - x_n + neighbour_bias[c*N + n])
 * Every measure but SCS, every geometry, f32 / bf16, any strides; inner_R must be 0.  centre_bias [C] and
 * neighbour_bias [C*N] (reshape order of nfp.py:136-139, n in tap order without the centre) and their gradients are f32
 * DEVICE pointers.  Norm and RMSE never read the centre bias: centre_bias / grad_centre_bias may be NULL there (and
 * grad_centre_bias is then not written).  The bias gradients are sums over the batch in a fixed order (no atomics).
 *   nfp_bias_saved_floats(d)     per-call state forward hands to backward: per-pair statistics (2 * stats per pair) or,
 *                                for Attention, the raw dots (needed also without a backward); -1 for a refused d
 *   nfp_bias_scratch_floats(d)   scratch of the backward (per-pair coefficients, per-image bias partials)
 * Both calls take the LENGTH of every caller buffer and return NFP_E_INVALID, launching nothing, when one is short.
 * `saved` may be NULL in nfp_bias_forward when no backward follows (not for Attention).
 */
int64_t nfp_bias_saved_floats(const nfp_desc* d);
int64_t nfp_bias_scratch_floats(const nfp_desc* d);
int nfp_bias_forward(const nfp_desc* d, const void* x, const float* centre_bias, const float* neighbour_bias, void* out,
                     float* saved, int64_t saved_floats, void* hip_stream);
int nfp_bias_backward(const nfp_desc* d, const void* x, const float* centre_bias, const float* neighbour_bias,
                      const void* grad_out, const void* out, const float* saved, int64_t saved_floats, void* grad_x,
                      float* grad_centre_bias, float* grad_neighbour_bias, float* scratch, int64_t scratch_floats,
                      void* hip_stream);

/*
 * The tail of models/nfp_heads.py::SimilarityAwarePooling.forward (nfp_heads.py:224-232) on the maps an NFP layer has
 * produced: att_proj (a trainable 1x1 conv N -> 1: w [N], b [1]), a softmax over the P = Ho*Wo pixels and the
 * attention-weighted sum — six ATen launches in the reference, one kernel each way here (csrc/nfp_attpool.hip):
 *   l_p = b + sum_n w_n m_np      att = softmax_p(l)      pooled_n = sum_p att_p m_np
 *   maps    [B,N,P] dense (the layer's [B,N,Ho,Wo] output), dtype = enum nfp_dtype; w, b, pooled [B,N], att [B,P] and
 *           every gradient but grad_maps are float32 DEVICE pointers; all arithmetic is float32
 *   att     written for the backward; NULL when none will follow
 * nfp_attpool_backward, given grad_pooled [B,N] and the att the forward wrote: grad_maps [B,N,P] in the maps' dtype (one
 * rounding), grad_w [N] and grad_b [1] — sums over the batch in image order through per-image partials in `scratch`
 * (nfp_attpool_scratch_floats(B, N) = B*(N+1) floats, min 1; needed only with grad_w or grad_b).  Each of the three may be
 * NULL: it is then neither computed nor written.  No atomics: two runs agree bitwise, and image b's pooled / grad_maps do
 * not depend on B.  The launch counter moves by 1 (forward), by 1 or — with grad_w or grad_b — 2 (backward);
 * nfp_last_variant names attpool_fwd<f32|bf16> / attpool_bwd<f32|bf16>.
 * NFP_E_INVALID, launching nothing (checked before any HIP call): a NULL required pointer, B < 0, N < 1, P < 1, an unknown
 * dtype, a scratch shorter than nfp_attpool_scratch_floats.  NFP_E_UNSUPPORTED: N*P >= 2^31, N > 1024.  B = 0 returns
 * NFP_OK without a launch (and writes nothing).  Additive to ABI 7: no descriptor, no workspace.
 */
int64_t nfp_attpool_scratch_floats(int32_t B, int32_t N);
int nfp_attpool_forward(int32_t B, int32_t N, int64_t P, int32_t dtype, const void* maps, const float* w, const float* b,
                        float* pooled, float* att, void* hip_stream);
int nfp_attpool_backward(int32_t B, int32_t N, int64_t P, int32_t dtype, const void* maps, const float* w, const float* att,
                         const float* grad_pooled, void* grad_maps, float* grad_w, float* grad_b, float* scratch,
                         int64_t scratch_floats, void* hip_stream);

/*
 * The encoding layer of the Deep-TEN baseline, models/deepten.py::DeepTENEncoding.forward (deepten.py:51-58), without its
 * [B,N,K,D] residual tensor (csrc/nfp_deepten.hip).  x [B,D,H,W] read as N = H*W pixels of D channels, K codewords:
 *   dist[b,n,k] = sum_d (x[b,n,d] - c[k,d])^2      A = softmax_k(-scale[k] * dist)      out[b,k,d] = sum_n A[b,n,k] (x[b,n,d] - c[k,d])
 *   x          dtype = enum nfp_dtype; layout = enum nfp_act_layout: NFP_ACT_NCHW, element (n, d) of image b at
 *              b*sxB + d*N + n, or NFP_ACT_NHWC (channels-last, a token sequence [B,N,D]), at b*sxB + n*D + d; sxB >= 0 in
 *              elements (the class token in front of a ViT's patch tokens stays where it is)
 *   codewords  [K,D], scale [K], saved, scratch, grad_out [B,K,D], grad_codewords [K,D], grad_scale [K]: float32 DEVICE
 *              pointers; out [B,K,D] and grad_x (dense, in x's layout) in x's dtype, one rounding; all arithmetic is float32
 *   saved      nfp_deepten_saved_floats(B, N, K) = 2*B*N*K floats (min 1): A, then dist.  Written by the forward for the
 *              backward — and for the forward's own second launch, which reads A from it: it is required also when no
 *              backward follows
 *   scratch    nfp_deepten_scratch_floats(B, N, K, D, want_params) floats (min 1): w [B,N,K] and, with want_params (either
 *              parameter gradient asked for), the per-image partials of grad_codewords [B,K,D] and the per-tile ones of
 *              grad_scale
 * Each of grad_x, grad_codewords, grad_scale may be NULL: it is then neither computed nor written.  No atomics: two runs
 * agree bitwise, and image b's out / grad_x do not depend on B.
 * The launch counter moves by 2 (forward: dten_assign, dten_aggregate); backward: dten_bwd_assign, then dten_bwd_x with
 * grad_x or grad_codewords, then dten_reduce with either parameter gradient — 2 with grad_x alone, 3 with everything, 0
 * with none.  nfp_last_variant names dten_fwd<f32|bf16,nchw|nhwc> / dten_bwd<f32|bf16,nchw|nhwc>.
 * NFP_E_INVALID, launching nothing (checked before any HIP call): a NULL required pointer, B < 0, N < 1, K < 1, D < 1, an
 * unknown dtype or layout, sxB < 0, a saved or scratch shorter than its query.  NFP_E_UNSUPPORTED: K > 64; N*D, N*K or K*D
 * of 2^31 and more.  B = 0 returns NFP_OK without a launch (and writes nothing).  Additive to ABI 7: no descriptor, no
 * workspace.
 */
int64_t nfp_deepten_saved_floats(int32_t B, int64_t N, int32_t K);
int64_t nfp_deepten_scratch_floats(int32_t B, int64_t N, int32_t K, int32_t D, int32_t want_params);
int nfp_deepten_forward(int32_t B, int64_t N, int32_t K, int32_t D, int32_t dtype, int32_t layout, int64_t sxB, const void* x,
                        const float* codewords, const float* scale, void* out, float* saved, int64_t saved_floats,
                        void* hip_stream);
int nfp_deepten_backward(int32_t B, int64_t N, int32_t K, int32_t D, int32_t dtype, int32_t layout, int64_t sxB, const void* x,
                         const float* codewords, const float* scale, const float* saved, int64_t saved_floats,
                         const float* grad_out, void* grad_x, float* grad_codewords, float* grad_scale, float* scratch,
                         int64_t scratch_floats, void* hip_stream);

/*
 * NFP on VALID maps — stride 1, dilation 1, pad = 0, R = 1 or 2: the layer inside every block of
 * models/nfp_heads.py::NFPBottleneck (nfp_heads.py:234-278) and in front of SimilarityAwarePooling's softmax.  Kernels of
 * their own (csrc/nfp_valid.hip: fwd_valid / bwd_valid), one launch each way, no workspace, no atomics: two runs agree
 * bitwise and image b's results do not depend on B.  out / grad_out are [B, N, H-2R, W-2R] contiguous in d->dtype, exactly
 * what nfp_forward writes for the descriptor; grad_x is fully overwritten, border pixels included.
 *   nfp_valid_supported(d)     1: both calls below will launch (a host-only dry run; 4 KiB-aligned buffers assumed)
 *   nfp_valid_saved_floats(d)  floats of `saved` (|x| per input pixel for cosine / gfc, else 0); -1 for a malformed d
 * Served: cosine / dot / gfc / Norm p = 2 / rmse (the distances on the difference weights), either `similarity`,
 * float32 / bf16, rows of W <= 128 pixels, any height and batch the descriptor allows; images dense in NCHW order (any
 * C) or in channels-last order (C % 4 == 0 for float32, C % 8 == 0 for bf16, images on 16-byte boundaries), any batch
 * stride.  NFP_E_UNSUPPORTED, launching nothing: everything else — pad != 0, map_f32 = 1, inner_R != 0, other measures,
 * wider rows.  The length convention of the bias / gap calls: a `saved` shorter than nfp_valid_saved_floats(d) returns
 * NFP_E_INVALID and launches nothing (forward: `saved` may be NULL when no backward follows).  B = 0 returns NFP_OK
 * without a launch.  nfp_last_variant names fwd_valid<R,prod|dist,f32|bf16,nchw|nhwc> / bwd_valid<...>.  Additive to ABI 7.
 */
int nfp_valid_supported(const nfp_desc* d);
int64_t nfp_valid_saved_floats(const nfp_desc* d);
int nfp_valid_forward(const nfp_desc* d, const void* x, void* out, float* saved, int64_t saved_floats, void* hip_stream);
int nfp_valid_backward(const nfp_desc* d, const void* x, const void* grad_out, const void* out, const float* saved,
                       int64_t saved_floats, void* grad_x, void* hip_stream);

/*
 * The L1 family of the valid-map kernels: Norm p = 1 on the difference weights (diff_weights = 1) — the reference's
 * NFPPooling() with no keywords (measure='norm', p=1, padding=0, R=1), the layer NFPInsert builds — and EMD, which the
 * library turns into exactly that descriptor (the same sum of |centre - neighbour| and the same sign gradient, 0 at 0;
 * its p and diff_weights fields are ignored).  Entry points of their own because their contract is smaller: the backward
 * needs neither `out` nor a saved statistic (a pair's coefficient is -+ grad_out), so there is no `saved` and the caller
 * may overwrite `out` before the backward.  grad_x[c][r] = sum_j W[j][r] sgn(x[c][r] - x[c][r + d_j]), sgn(0) = 0.
 *   nfp_valid_abs_supported(d)  1: both calls below will launch (a host-only dry run; 4 KiB-aligned buffers assumed);
 *                               changes neither nfp_launch_count, nfp_last_variant nor nfp_last_error
 * Served: NFP_NORM with p == 1 and diff_weights = 1, NFP_EMD, either `similarity`; geometry, types and layouts exactly
 * those of nfp_valid_* above (pad 0, stride 1, dilation 1, R = 1 or 2, 2R+1 <= W <= 128, NCHW with any C and any batch
 * stride or 16-byte-aligned channels-last with C % 4 == 0 (float32) / C % 8 == 0 (bf16), map_f32 = 0, inner_R = 0).
 * NFP_E_UNSUPPORTED, launching nothing: every other measure, Norm with p != 1, 'Norm' on the pure-neighbour weights
 * (diff_weights = 0), and what the geometry and layout rules exclude.  A null tensor is NFP_E_INVALID; B = 0 returns
 * NFP_OK without a launch.  One launch each way, no workspace, no atomics, the same bands and channel blocks as
 * nfp_valid_*: two runs agree bitwise and image b's results do not depend on B.
 * nfp_last_variant names fwd_valid<R,l1,f32|bf16,nchw|nhwc> / bwd_valid<R,l1,...>.  Additive to ABI 7.
 */
int nfp_valid_abs_supported(const nfp_desc* d);
int nfp_valid_abs_forward(const nfp_desc* d, const void* x, void* out, void* hip_stream);
int nfp_valid_abs_backward(const nfp_desc* d, const void* x, const void* grad_out, void* grad_x, void* hip_stream);

/*
 * NFP at STRIDE 2 to 4 — dilation 1, R = 1 or 2, pad = 0 or pad = R with zeros / reflect / replicate: the `--nfp_stride`
 * layers of the reference's demo.py (RESNET18_NFP_AT_LAYER, *_NFP_CONV_ONLY / _CONV_MLP, MOBILENETV3_NFP_INSERT).  Kernels of
 * their own (csrc/nfp_strided.hip: fwd_strided / bwd_strided) on the padded row band, one launch each way, no tables, no
 * workspace, no atomics: two runs agree bitwise and image b's results do not depend on B.  out / grad_out are
 * [B, N, Ho, Wo] contiguous in d->dtype, exactly what nfp_forward writes for the descriptor; grad_x is fully overwritten,
 * with zeros at the pixels no window reaches.  Signatures and length convention of the nfp_valid_* quartet:
 *   nfp_strided_supported(d)     1: both calls below will launch (a host-only dry run; 4 KiB-aligned buffers assumed)
 *   nfp_strided_saved_floats(d)  floats of `saved` (|x| per input pixel for cosine / gfc, else 0); -1 for a malformed d
 * Served: cosine / dot / gfc / Norm p = 2 / rmse (the distances on the difference weights), either `similarity`,
 * 2 <= stride <= 4, float32 / bf16, H + 2 pad >= 2R + 1 (W likewise) and W + 2 pad <= 128; images dense in NCHW order (any
 * C) or in channels-last order (C % 4 == 0 for float32, C % 8 == 0 for bf16, images on 16-byte boundaries), any batch
 * stride.  The backward keeps the slots of a band of at least R + 1 image rows and its ring rows in LDS: R = 2 with
 * pad = 2 is served up to W + 2 pad <= 64 at every height, wider where that band still fits (the query answers).
 * NFP_E_UNSUPPORTED, launching nothing: stride 1 or above 4, dilation != 1, any other padding amount, circular padding,
 * R >= 3, every other measure, wider rows, map_f32 = 1, inner_R != 0.  A null tensor or a `saved` shorter than
 * nfp_strided_saved_floats(d) is NFP_E_INVALID and launches nothing (forward: `saved` may be NULL when no backward
 * follows).  B = 0 returns NFP_OK without a launch.  nfp_forward / nfp_backward / nfp_plan keep strided descriptors on
 * fwd_pairs / bwd_gather.  nfp_last_variant names fwd_strided<R,prod|dist,f32|bf16,nchw|nhwc> / bwd_strided<...>.
 * Additive to ABI 7.
 */
int nfp_strided_supported(const nfp_desc* d);
int64_t nfp_strided_saved_floats(const nfp_desc* d);
int nfp_strided_forward(const nfp_desc* d, const void* x, void* out, float* saved, int64_t saved_floats, void* hip_stream);
int nfp_strided_backward(const nfp_desc* d, const void* x, const void* grad_out, const void* out, const float* saved,
                         int64_t saved_floats, void* grad_x, void* hip_stream);

/*
 * The tail the three trained heads of models/nfp_heads.py share behind their NFP maps (NFPHead nfp_heads.py:28-32,42-43,
 * MultiRadiusNFPHead 98-102,114-115, AdaptiveFusionNFP 301-305,323-324):
 *   compress = Conv2d(N, D, 1, bias=False) -> BatchNorm2d(D) -> ReLU        out [B,D] = GAP(compress(maps))
 * without the [B,D,P] activation (csrc/nfp_cpool.hip): train-mode BatchNorm statistics of a 1x1 conv's output follow from
 * the mean mu [N] and the biased covariance Sigma [N,N] of its input over the M = B*P pixels of the batch, the pre-activation
 * is formed from the image's maps in LDS and averaged at once, and the backward recomputes it.
 *   maps    [B,N,P] dense, dtype = enum nfp_dtype; w [D,N], gamma [D], beta [D], the running statistics [D], out [B,D] and
 *           every gradient but grad_maps (the maps' dtype, one rounding) are float32 DEVICE pointers
 *   training != 0   batch statistics (second moments taken centred, joined in float64); running_mean / running_var, given
 *                   together or both NULL, are updated in the same call: rm <- (1 - momentum) rm + momentum mean,
 *                   rv <- (1 - momentum) rv + momentum var M / (M - 1).  `saved` (nfp_cpool_saved_floats(N, D) = 2N + N*N + D
 *                   floats: mu as two floats, Sigma, 1/sqrt(var + eps)) is written for the backward and required;
 *                   `scratch` holds nfp_cpool_scratch_floats(B, N, P, D, 0) floats
 *   training == 0   the running statistics stand for mean and var (both required; read again by the backward); saved and
 *                   scratch are not touched and may be NULL
 * nfp_cpool_backward, given grad_out [B,D]: grad_maps [B,N,P], grad_w [D,N], grad_gamma [D], grad_beta [D] — each may be
 * NULL and is then neither computed nor written; scratch of nfp_cpool_scratch_floats(B, N, P, D, 1) floats (not needed for
 * an eval-mode grad_maps alone).  Launches: forward 3 in training (moments, finish, main) and 1 in eval; backward at most 3
 * (per-slice partial sums, the batch reduce with the parameter gradients, grad_maps), the last skipped without grad_maps,
 * the first two for an eval-mode grad_maps alone.  No atomics: two runs agree bitwise, and in eval image b's row of out /
 * grad_maps does not depend on the batch around it.  nfp_last_variant names cpool_fwd<f32|bf16,train|eval> / cpool_bwd<...>.
 * Every caller buffer that has a length query comes with its length: a short (or missing) one returns NFP_E_INVALID and
 * launches nothing, as do a NULL required pointer, B < 0, N < 1, P < 1, D < 1, an unknown dtype, a negative eps — all checked
 * before any HIP call.  NFP_E_UNSUPPORTED: N > 32, N*P >= 2^31, D > 2^22, B*P < 2 in training.  B = 0 returns NFP_OK
 * without a launch.  Additive to ABI 7: no descriptor, no workspace.
 */
int64_t nfp_cpool_saved_floats(int32_t N, int32_t D);
int64_t nfp_cpool_scratch_floats(int32_t B, int32_t N, int64_t P, int32_t D, int32_t backward);
int nfp_cpool_forward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, const void* maps,
                      const float* w, const float* gamma, const float* beta, float* running_mean, float* running_var,
                      double momentum, double eps, float* out, float* saved, int64_t saved_floats, float* scratch,
                      int64_t scratch_floats, void* hip_stream);
int nfp_cpool_backward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, const void* maps,
                       const float* w, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, double eps, const float* saved, int64_t saved_floats, const float* grad_out,
                       void* grad_maps, float* grad_w, float* grad_gamma, float* grad_beta, float* scratch,
                       int64_t scratch_floats, void* hip_stream);

/*
 * The same tail for 1 <= N <= 96 maps (csrc/nfp_cpool.hip, the cpw kernels): the heads at R = 3 (48 maps), R = 4 (80) and
 * R_list = (1, 2, 3) (80).  The weight rows of 64 channels and the chunk's centred maps sit in LDS and a lane owns a small
 * tile of outputs, so nothing in registers grows with N.  Arguments, formulas, `saved` (nfp_cpool_saved_floats(N, D) floats,
 * the same layout) and every convention and refusal are those of nfp_cpool_* above, with these differences:
 *   N         up to 96; NFP_E_UNSUPPORTED above
 *   scratch   nfp_cpool_wide_scratch_floats(B, N, P, D, backward) floats; the forward's must be 8-byte aligned
 *   launches  forward 5 in training (moments, mu, Sigma, var, main) and 1 in eval; backward at most 3, skipped as above
 * nfp_last_variant names cpool_wide_fwd<f32|bf16,train|eval,nK> / cpool_wide_bwd<...>, K = N rounded up to 16.  The results
 * are not bitwise those of nfp_cpool_* (other sums, other orders); two runs of these entries agree bitwise.  Additive to ABI 7.
 */
int64_t nfp_cpool_wide_scratch_floats(int32_t B, int32_t N, int64_t P, int32_t D, int32_t backward);
int nfp_cpool_wide_forward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, const void* maps,
                           const float* w, const float* gamma, const float* beta, float* running_mean, float* running_var,
                           double momentum, double eps, float* out, float* saved, int64_t saved_floats, float* scratch,
                           int64_t scratch_floats, void* hip_stream);
int nfp_cpool_wide_backward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, const void* maps,
                            const float* w, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, double eps, const float* saved, int64_t saved_floats,
                            const float* grad_out, void* grad_maps, float* grad_w, float* grad_gamma, float* grad_beta,
                            float* scratch, int64_t scratch_floats, void* hip_stream);

/*
 * The same projection with the map kept (csrc/nfp_cpool.hip, the cproj kernels) — NFPInsert's nfp_proj
 * (models/mobilenetv3.py:346-350: Conv2d(N, D, 1, bias=False) -> BatchNorm2d(D) -> ReLU) and NFPBottleneck's bn2(conv2(.))
 * (models/nfp_heads.py:270-272, relu = 0):
 *   out [B,D,P] = [relu](batch_norm(conv1x1(maps)))
 * stored once, dense, in the maps' dtype (float32 arithmetic, one rounding).  Arguments, statistics, `saved`
 * (nfp_cpool_saved_floats(N, D) floats) and every convention are those of nfp_cpool_* above, with three differences:
 *   relu      != 0: the ReLU behind the BatchNorm; 0: none (the pre-activation is the output)
 *   out       [B,D,P] and grad_out [B,D,P] are DEVICE pointers of the maps' dtype
 *   scratch   holds nfp_cproj_scratch_floats(B, N, P, D, backward) floats
 * The backward reads the maps, the parameters, `saved` and grad_out — never `out`, which the caller may have modified in
 * place — and recomputes the pre-activation for the ReLU's mask.  Launches: forward 3 in training (moments, finish,
 * cproj_fwd) and 1 in eval; backward at most 3 (cproj_bwd_part, the batch reduce, cproj_bwd_maps), skipped as in
 * nfp_cpool_backward for the gradients passed as NULL.  No atomics: two runs agree bitwise, and in eval image b's rows of
 * out / grad_maps do not depend on the batch around it.  nfp_last_variant names cproj_fwd<f32|bf16,train|eval,relu|lin> /
 * cproj_bwd<...>.  NFP_E_INVALID, launching nothing: a short or missing buffer, a NULL required pointer, B < 0, N < 1, P < 1,
 * D < 1, an unknown dtype, a negative eps.  NFP_E_UNSUPPORTED: N > 32, N*P >= 2^31, D*P >= 2^31, D > 2^22, B*P < 2 in
 * training.  B = 0 returns NFP_OK without a launch.  Additive to ABI 7.
 */
int64_t nfp_cproj_scratch_floats(int32_t B, int32_t N, int64_t P, int32_t D, int32_t backward);
int nfp_cproj_forward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, int32_t relu,
                      const void* maps, const float* w, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, double momentum, double eps, void* out, float* saved, int64_t saved_floats,
                      float* scratch, int64_t scratch_floats, void* hip_stream);
int nfp_cproj_backward(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, int32_t relu,
                       const void* maps, const float* w, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, double eps, const float* saved, int64_t saved_floats, const void* grad_out,
                       void* grad_maps, float* grad_w, float* grad_gamma, float* grad_beta, float* scratch,
                       int64_t scratch_floats, void* hip_stream);

/*
 * The same two calls with a memory layout for the [B,D,P] activation — `out` in the forward, `grad_out` in the backward;
 * the maps and grad_maps stay [B,N,P]:
 *   NFP_ACT_NCHW  [b][d][p], element (b*D + d)*P + p: the calls above — the same kernels, the same bytes
 *   NFP_ACT_NHWC  [b][p][d], element (b*P + p)*D + d: a channels-last [B,D,H,W] tensor, P = H*W
 * The layout is the last argument, behind hip_stream; every other argument, length query (nfp_cproj_scratch_floats serves
 * both layouts), refusal and launch count is as documented for nfp_cproj_forward / nfp_cproj_backward, and the two calls
 * of one step need not use the same layout.  With NFP_ACT_NHWC every element of `out` has the bits the NCHW call stores
 * for it, the parameter gradients are summed in the NCHW call's order, and no atomics are used.  nfp_last_variant names
 * cproj_fwd<...,nhwc> / cproj_bwd<...,nhwc>.  Any other layout value: NFP_E_INVALID, launching nothing.  Additive to ABI 7.
 */
enum nfp_act_layout { NFP_ACT_NCHW = 0, NFP_ACT_NHWC = 1 };
int nfp_cproj_forward_fmt(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, int32_t relu,
                          const void* maps, const float* w, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, double momentum, double eps, void* out, float* saved, int64_t saved_floats,
                          float* scratch, int64_t scratch_floats, void* hip_stream, int32_t out_layout);
int nfp_cproj_backward_fmt(int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t training, int32_t relu,
                           const void* maps, const float* w, const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, double eps, const float* saved, int64_t saved_floats,
                           const void* grad_out, void* grad_maps, float* grad_w, float* grad_gamma, float* grad_beta,
                           float* scratch, int64_t scratch_floats, void* hip_stream, int32_t grad_out_layout);

/*
 * The train-mode step of nfp_cpool_* / nfp_cproj_*_fmt in stages, for BatchNorm statistics taken over the batches of
 * several ranks (nn.SyncBatchNorm): the caller gathers a small record between the stages, by whatever collective it has —
 * this library makes none.  A rank is any holder of a share of the batch; B, P and the maps are the rank's own, N and D
 * everyone's.  kind: NFP_CP_POOL (out [B,D] float32, the ReLU always; relu and the layout are ignored) or NFP_CP_PROJ
 * (out / grad_out [B,D,P] in the maps' dtype, `relu` and the layout the caller's).  Up to 32 maps; the wide form has no
 * staged calls.
 *   nfp_cpsync_moments   the rank's record, float64 [n, mu (N), S (N*N)] = nfp_cpsync_record_doubles(N) doubles: its count
 *                        n = B*P of values per map, their mean, their scatter about that mean (not divided).  scratch:
 *                        nfp_cpool_scratch_floats(B, N, P, 1, 0) floats.  2 launches (moments, the join); B = 0 writes the
 *                        zero record with the join alone
 *   nfp_cpsync_forward   `records`: the records of `world` ranks, row r rank r's, the same rows in the same order on every
 *                        rank.  They are joined in rank order in float64 — M = sum n_r, mu = sum n_r mu_r / M,
 *                        Sigma = sum_r (S_r + n_r d_r d_r') / M with d_r = mu_r - mu — and from there on everything is as in
 *                        nfp_cpool_forward: inv_d, the running statistics (updated with the counts' sum M, so they come out
 *                        bitwise equal on every rank) and `saved`, then the rank's rows of `out`.  `saved` holds
 *                        nfp_cpsync_saved_floats(N, D) = 2N + 2 N*N + D + 1 floats: nfp_cpool_saved_floats' layout, then
 *                        (float)M, then what Sigma [N*N] loses as a float (the backward's grad_w reads both).
 *                        global_count: sum n_r where the caller knows it on the host, else 0; it is only checked (the
 *                        kernels use the records' own counts).  2 launches (the join, the main kernel); B = 0 the join alone
 *   nfp_cpsync_reduce    the rank's grad_w, grad_gamma, grad_beta (each may be NULL; their sum over the ranks is the batch's
 *                        gradient) and its row [k (N), Q (N*N)] = nfp_cpsync_kq_floats(N) floats, with M the count over all
 *                        ranks.  scratch: nfp_cpool_scratch_floats / nfp_cproj_scratch_floats (B, N, P, D, 1).  3 launches;
 *                        B = 0 one, which writes zeros
 *   nfp_cpsync_maps      `kq_rows`: the rows of `world` ranks, summed in rank order; grad_maps [B,N,P] of the rank.  1
 *                        launch; B = 0 none
 * With world = 1 the stages compute what the one-call entries do, with another summation order in the statistics (the
 * results agree to float32 rounding, not bitwise).  No atomics: two runs agree bitwise.  nfp_last_variant names
 * cpsync_moments<f32|bf16> and cpsync_fwd|bwd_reduce|bwd_maps<pool|proj,relu|proj,lin,f32|bf16[,nhwc]>.
 * NFP_E_INVALID, before any HIP call: a NULL required pointer, a short buffer (every buffer comes with its length),
 * records not 8-byte aligned, world < 1, an unknown kind, dtype or layout, B < 0, N < 1, P < 1, D < 1, a negative eps or
 * global_count.  NFP_E_UNSUPPORTED: N > 32, the size limits of nfp_cpool_* / nfp_cproj_*, global_count = 1 (or below this
 * rank's own count).  A rank's own B*P may be 0 or 1.  Additive to ABI 7.
 */
enum nfp_cp_kind { NFP_CP_POOL = 0, NFP_CP_PROJ = 1 };
int64_t nfp_cpsync_record_doubles(int32_t N);
int64_t nfp_cpsync_kq_floats(int32_t N);
int64_t nfp_cpsync_saved_floats(int32_t N, int32_t D);
int nfp_cpsync_moments(int32_t B, int32_t N, int64_t P, int32_t dtype, const void* maps, double* record, int64_t record_doubles,
                       float* scratch, int64_t scratch_floats, void* hip_stream);
int nfp_cpsync_forward(int32_t kind, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t relu, const void* maps,
                       const float* w, const float* gamma, const float* beta, float* running_mean, float* running_var,
                       double momentum, double eps, const double* records, int32_t world, int64_t records_doubles,
                       int64_t global_count, void* out, float* saved, int64_t saved_floats, void* hip_stream,
                       int32_t out_layout);
int nfp_cpsync_reduce(int32_t kind, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t relu, const void* maps,
                      const float* w, const float* gamma, const float* beta, double eps, const float* saved,
                      int64_t saved_floats, const void* grad_out, float* grad_w, float* grad_gamma, float* grad_beta,
                      float* kq_row, int64_t kq_floats, float* scratch, int64_t scratch_floats, void* hip_stream,
                      int32_t grad_out_layout);
int nfp_cpsync_maps(int32_t kind, int32_t B, int32_t N, int64_t P, int32_t D, int32_t dtype, int32_t relu, const void* maps,
                    const float* w, const float* gamma, const float* beta, double eps, const float* saved, int64_t saved_floats,
                    const void* grad_out, const float* kq_rows, int32_t world, int64_t kq_floats, void* grad_maps,
                    void* hip_stream, int32_t grad_out_layout);

/* Telemetry: kernels enqueued by this process so far (tests use it to prove
 * the HIP path, not a fallback, produced a result). */
uint64_t nfp_launch_count(void);

/* Name of the kernel variant the last successful nfp_forward / nfp_backward /
 * nfp_pool_* of this PROCESS selected (for bench / profile bookkeeping),
 * copied into a buffer of the calling thread. */
const char* nfp_last_variant(void);

/* Telemetry: the NEXT forward / backward kernel this PROCESS launches — from whichever thread: autograd runs the
 * backward on a thread of its own, so the arming cannot be per calling thread — is bracketed by the two hipEvent_t
 * (hipExtLaunchKernel: recorded at the kernel's own start and end on the device, as a profiler's kernel trace
 * would) — per-kernel durations without a profiler and without inter-kernel gaps.  One shot; pass NULLs to
 * disarm.  SINGLE-LAUNCHER USE ONLY: while it is armed no second thread may enqueue NFP work, or the events bracket
 * that thread's kernel instead.  bench.py's *_eager_event_us figures come from here (one launch in flight at a time). */
void nfp_time_next_launch(void* start_event, void* stop_event);

/* Test hook: re-read the NFP_* A/B switches (NFP_FORCE_GENERIC, NFP_FWD_SCALAR,
 * NFP_BWD_ATOMIC, NFP_BWD_BANDS, NFP_MFMA) from the environment.  They are
 * otherwise read once, when the library is loaded. */
void nfp_reload_env(void);

/* Describe, WITHOUT touching the GPU, what nfp_forward (backward = 0) or
 * nfp_backward (backward != 0) would launch for `d` with 4 KiB-aligned buffers:
 *   "<variant> | <kernel> grid=(x,y,z) block=t lds=bytes[; <kernel> ...]"
 * written NUL-terminated into buf.  Returns what the real call would return for
 * the descriptor (NFP_E_UNSUPPORTED / NFP_E_INVALID with nfp_last_error set).
 * No reference counterpart: lets the dispatch rules (which kernel serves which
 * geometry, every launch within the device's LDS / grid limits) be tested on a
 * machine without a GPU. */
int nfp_plan(const nfp_desc* d, int32_t backward, char* buf, int32_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* NFP_H_ */
