/* libflair_hip.so -- C ABI of the MI355X (gfx950) kernels behind FLAIR's sampling hot path.
 *
 * Drop-in boundary.  The reference has no FFI on this path: its
 * Python calls ATen / torchvision / flash-attn / mmcv operators.  Each entry point below
 * names the reference call site(s) it replaces (paths relative to the reference root,
 * guided_diffusion/...).  The only native precedent in the reference is the pybind
 * module dcn/src/deform_conv_ext.cpp:150-163, whose conventions are kept: the caller owns
 * and pre-allocates every buffer, inputs are contiguous, work is enqueued on the caller's
 * stream, and nothing synchronises with the host.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers;
 *   - every function returns FLAIR_OK (0) or a negative flair_status and records a
 *     message retrievable with flair_last_error() (thread-local);
 *   - functions are asynchronous on `stream`, re-entrant, allocate nothing, and may be
 *     captured into a hipGraph;
 *   - activations are "clip tensors": [T][H][W][C] with C innermost ("NHWC"), element
 *     type FLAIR_F32 or FLAIR_BF16; per-channel parameters (bias, norm scale) are f32;
 *   - `ld` arguments are the element distance between consecutive pixels, so a tensor
 *     may be a channel slice of a wider buffer (this is how torch.cat is avoided).
 */
#ifndef FLAIR_HIP_H
#define FLAIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

typedef enum {
    FLAIR_OK = 0,
    FLAIR_ERR_ARG = -1, /* bad shape / alignment / null pointer */
    FLAIR_ERR_HIP = -2  /* HIP runtime refused the launch */
} flair_status;

typedef enum { FLAIR_F32 = 0, FLAIR_BF16 = 1 } flair_dtype;

typedef enum {
    FLAIR_ACT_NONE = 0,
    FLAIR_ACT_RELU = 1,
    FLAIR_ACT_LRELU01 = 2, /* LeakyReLU(0.1) */
    FLAIR_ACT_SILU = 3,
    /* offset / mask activation of SecondOrderDeformableAlignment (unet_new.py:879-885) applied by the
     * convolution that PRODUCES the 27*G tap-major offset channels: with period = 3*G (act_period),
     * channel co -> act_param * tanh(v) if co % period < 2*period/3 (the (dy,dx) residues, act_param =
     * max_residue_magnitude), else sigmoid(v) (the modulation mask).  flair_dcn_align then takes the
     * finished values (raw_activated = 1) instead of re-deriving them per gathered channel group. */
    FLAIR_ACT_DCN_OFFSETS = 4,
    FLAIR_ACT_LRELU02 = 5, /* LeakyReLU(0.2): SFT scale / shift branches, codeformer.py:579-588 */
    FLAIR_ACT_GELU = 6     /* exact (erf) GELU: transformer MLP, codeformer.py:520-528 */
} flair_act;

/* Last error message of the calling thread ("" if none). */
const char* flair_last_error(void);
/* ABI version of this header: bumped whenever entry points are added or a struct changes
 * (3: round 2; 4: + face crop / paste entries, flair_bcast_weights; 5: round 4 entries; 6: + calibration launches;
 * 7: flair_tattn_params.head_dim; 8: + flair_dwconv_nhwc; 9: + flair_vq_nearest_nhwc;
 * 10: + flair_dwconv7_nhwc, flair_dcn_params.raw_activated = 2 (VQFR's DCNv2Pack);
 * 11: + flair_global_avgpool_nhwc, flair_channel_gate_nhwc, flair_upsample_argmax_nhwc (BiSeNet face parsing);
 * 12: + flair_warp_affine_cubic_indexed, flair_face_paste (several faces per frame, frames without a face);
 * 13: + flair_maxpool2x2s2_nhwc, flair_spp_maxpool_nhwc, flair_channel_interleave_nhwc, flair_yolo_face_decode,
 *     flair_letterbox_nhwc (the YOLOv5-face detectors); 14: + flair_jpeg_roundtrip_hw (rectangular frames);
 * 15: + flair_image_metrics_workspace, flair_image_metrics (PSNR / SSIM of written frames);
 * 16: + flair_slomo_warp_pack, flair_slomo_blend (SuperSloMo); 17: + flair_corr_scale, flair_corr_pool, flair_corr_lookup,
 *     flair_prelu_nhwc, flair_depth_to_space2_nhwc, flair_axpby_nhwc,
 *     flair_amt_multiflow_prepare, flair_amt_multiflow_combine, flair_instnorm_workspace_bytes, flair_instnorm_nhwc (AMT-G);
 * 18: + flair_block_luma_sums (scene cuts).
 * The library may be used from several devices of one process: per-kernel launch attributes and
 * CU counts are cached per device. */
int flair_abi_version(void);

/* ------------------------------------------------------------------ convolution
 * Y = act(conv(X, W) + bias) + res0 + res1, times out_scale.  "same" zero padding,
 * stride 1, odd kernel sizes; KT > 1 convolves across frames (Conv3d), KT == 1 treats
 * frames as a batch (Conv2d / Conv1d-1x1 / Linear on pixels).
 * Replaces: unet_new.py:240-295 (ResBlock conv_nd 2-D/3-D, 1x1 skip), :359,:367,:409,:417
 * (qkv / proj_out Conv1d), :455-459 (TemporalAttention linears/proj), :659-668
 * (ResidualBlocksWithInputConv trunks, conv_last), :859-867 (offset conv stack), :993,
 * :1220 (stem / head convs); mmedit SPyNet 7x7 convs (unet_new.py:985).
 *   x[i]   : input segment i, [T][H][W] pixels of seg_c[i] channels, pixel stride seg_ld[i];
 *            the segments are the channel-wise concatenation the reference builds with
 *            th.cat (seg_c[i] must be a multiple of 32 (bf16) / 16 (f32); pad with zeros)
 *   w      : [Cout][KT*KH*KW][sum seg_c] in the activation dtype
 *   bias   : [Cout] f32 or NULL;  res0/res1: [T][H][W][Cout-slice] or NULL, pixel stride res_ld[i] >= Cout
 *   frame_bias : [T][frame_bias_ld] f32 or NULL, added before the activation (the per-frame
 *            embedding terms `h + emb_out` of unet.py:246 and sr3.py:82)
 *   y      : [T][H][W] pixels, y_ld elements apart, Cout (multiple of 4) written per pixel, 16-byte aligned
 *   strides: segments, y_ld and res_ld are multiples of 16 bytes and res0 / res1 16-byte aligned (the epilogues move
 *            16-byte pieces), except for bf16 with Cout % 8 == 4, whose outputs and residuals move as 8-byte quads:
 *            there y_ld, res_ld and the residual pointers need 8 bytes only
 *   workspace : optional device scratch of flair_conv_workspace_bytes(p) bytes; when given,
 *            deep-K convolutions on few pixels (the 16x16..4x4 levels) are split over K
 *            (f32 partial sums + a reduce/epilogue launch) */
typedef struct {
    int dtype;
    int T, H, W;
    int KT, KH, KW;
    int Cout;
    int nseg;
    int seg_c[4];
    int seg_ld[4];
    int y_ld;
    int res_ld[2];
    int act;
    float out_scale;
    int frame_bias_ld;
    int stride; /* spatial stride 1 (default when 0) or 2: T,H,W describe the INPUT, the output is
                 * ceil(H/stride) x ceil(W/stride) (PyTorch Conv2d(k, stride, padding=k//2)) */
    float act_param; /* FLAIR_ACT_DCN_OFFSETS: max_residue_magnitude */
    int act_period;  /* FLAIR_ACT_DCN_OFFSETS: 3 * deform_groups (multiple of 24) */
    int asym_pad;    /* 1 (stride 2 only): taps at stride*i .. stride*i + K-1, zeros past the bottom / right edge =
                      * F.pad(x, (0, 1, 0, 1)) + Conv2d(k, stride 2, padding 0), CodeFormer's Downsample
                      * (codeformer.py:138-149); 0: taps centred (padding k//2) */
    int reflect_pad; /* 1: taps that fall outside the frame read the mirrored pixel (nn.ReflectionPad2d(k//2) + Conv2d
                      * without padding: ParseNet's ConvLayer, facelib/parsing/parsenet.py:92-104) instead of zeros;
                      * im2col kernels only (any stride) */
} flair_conv_params;

size_t flair_conv_workspace_bytes(const flair_conv_params* p);
int flair_conv_nhwc(const flair_conv_params* p, const void* const* x, const void* w,
                    const float* bias, const float* frame_bias, const void* res0, const void* res1,
                    void* y, void* workspace, size_t workspace_bytes, hipStream_t stream);
/* Which kernel variant flair_conv_nhwc launches for these parameters (profiling aid):
 * im2col tiles 0 = 128 couts x 128 pixels, 1 = 64 x 128, 2 = 64 x 64 per workgroup;
 * halo kernel (3x3 spatial taps, W % 32 == 0) 3 / 4 / 5 = 8 / 4 / 2 image rows per workgroup;
 * 6 / 7 = K-split halo kernel with 8 / 4 rows (launches of exactly 256 workgroups: one frame). */
int flair_conv_variant(const flair_conv_params* p);


/* ------------------------------------------------- fused chain of two 3x3 convolutions
 * M = actA(conv3x3(cat(x), WA) + biasA)   (C = 64 or 128 channels, never leaves the LDS)
 * Y = (actB(conv3x3(M, WB) + biasB) + res0 + res1) * out_scale        (CoutB channels)
 * per frame, zero "same" padding on both convolutions.  With WA == NULL there is no stage A: the
 * single input segment (C channels) is staged once per tile and kept resident while CoutB is walked
 * in blocks of 64 (wide-output convolutions: the c -> 27*G offset convolution).  For bf16, C = 64, W % 32 == 0,
 * H % 8 == 0, CoutB % 8 == 0 and no residual inputs this form runs on conv_resident_kernel (round 4: halo by LDS-DMA,
 * three-stage weight ring, the epilogue of one 64-cout block issued between the MFMAs of the next); same results.
 * Replaces pairs of dependent launches of the BasicVSR++ recurrence: conv_offset[2]+[4] and
 * conv_offset[4]+[6] of SecondOrderDeformableAlignment (unet_new.py:859-867), conv1+conv2 of mmedit's
 * ResidualBlockNoBN inside ResidualBlocksWithInputConv with its residual adds (unet_new.py:659-668,
 * :731-739) -- same rounding points as the two launches (the intermediate is rounded to the element type).
 *   x[i], seg_c, seg_ld : input segments as in flair_conv_nhwc (T frames of H x W, W % 8 == 0)
 *   wA : [C][9][sum seg_c] or NULL;  wB : [CoutB][9][C];  biases f32 or NULL
 *   res0 / res1 : [T][H][W][CoutB-slice] or NULL, added after actB;  y : pixel stride y_ld
 *   y_ld, res_ld >= CoutB; segment, output and residual strides and pointers at 16-byte granularity */
typedef struct {
    int dtype;
    int T, H, W;
    int C;      /* channels of the intermediate (= output channels of stage A) */
    int CoutB;
    int nseg;
    int seg_c[4];
    int seg_ld[4];
    int y_ld;
    int res_ld[2];
    int actA, actB;
    float out_scale;
    float act_param; /* actB == FLAIR_ACT_DCN_OFFSETS: max_residue_magnitude */
    int act_period;  /* actB == FLAIR_ACT_DCN_OFFSETS: 3 * deform_groups */
} flair_chain_params;

int flair_conv_chain(const flair_chain_params* p, const void* const* x, const void* wA, const float* biasA,
                     const void* wB, const float* biasB, const void* res0, const void* res1, void* y,
                     hipStream_t stream);


/* ------------------------------------------------------- GroupNorm + SiLU (+ FiLM)
 * y = act( GroupNorm(x) * (1 + scale) + shift ), statistics joint over
 * (C/groups) x frames_per_stat x H x W (frames_per_stat = T for the FLAIR video UNet,
 * 1 for per-frame norms).  The input may be the channel concatenation of two stored
 * tensors (x0: first c0 channels, x1: the remaining C - c0).  resample: 0 none,
 * 1 = 2x2 average pooling of the activated result, 2 = nearest 2x upsampling; `raw`
 * (optional) receives the identically resampled un-normalised input.
 * Replaces: nn_new.py:17-19 GroupNorm32 behind nn.py:359-367 LazyReshaper3D, with the
 * SiLU / (1+scale)*h+shift / Upsample / Downsample steps of unet_new.py:237-329, the
 * attention norms (:358,:408,:461) and the head (:1216-1222).
 *   gamma, beta : [C] f32;  film : [F][film_ld] f32 rows of (scale[C] | shift[C]) or NULL
 *   workspace   : flair_groupnorm_workspace_bytes(p) bytes of device scratch
 *   limits      : C <= 2048 (f32) / 4096 (bf16): one 16-byte channel piece per thread of a <= 512-thread row group
 *                 (FLAIR_ERR_ARG "too wide" beyond that); C a multiple of 4 (f32) / 8 (bf16).
 *   strides     : ld0 / ld1 / y_ld / raw_ld at least the channels they hold and multiples of 16 bytes; x0, x1, y, raw
 *                 16-byte aligned (film rows may have any stride >= 2C and any 4-byte alignment). */
typedef struct {
    int dtype;
    int C, c0;   /* channels in total / in segment 0 */
    int ld0, ld1;
    int groups;
    int F, H, W;
    int frames_per_stat;
    float eps;
    int act;
    int resample;
    int y_ld, raw_ld;
    int film_ld;
} flair_gn_params;

/* y (and raw) must not alias x0 / x1. */
size_t flair_groupnorm_workspace_bytes(const flair_gn_params* p);
int flair_groupnorm_nhwc(const flair_gn_params* p, const void* x0, const void* x1,
                         const float* gamma, const float* beta, const float* film, void* y,
                         void* raw, void* workspace, hipStream_t stream);

/* ----------------------------------------------------------------- API-edge layout
 * (N,C,H,W) f32 <-> channel slice [coff, coff+C) of an NHWC clip tensor.  Replaces the
 * rearrange/cat/type casts at unet_new.py:1330-1331,1353,1361-1362. */
int flair_nchw_f32_to_nhwc(const float* src, int N, int C, int H, int W, void* dst, int dtype,
                           int dst_ld, int dst_coff, hipStream_t stream);
int flair_nhwc_to_nchw_f32(const void* src, int dtype, int src_ld, int src_coff, int N, int C,
                           int H, int W, float* dst, hipStream_t stream);

/* timestep_embedding (nn_new.py:103-121): out[n] = [cos(t_n f_i) | sin(t_n f_i)], f32;
 * sin_first != 0 gives sr3's PositionalEncoding order [sin | cos] (sr3.py:45-60). */
int flair_timestep_embedding(const float* t, int N, int dim, float max_period, int sin_first,
                             float* out, hipStream_t stream);

/* y = act_out(act_in(x) @ w^T + bias), f32, M <= 32 rows (one per frame).  Replaces the
 * time_embed MLP (unet_new.py:980-984,1351) and every emb_layers Linear (:258-264,:399). */
int flair_linear_f32(const float* x, int M, int K, const float* w, const float* bias, int N,
                     int act_in, int act_out, float* y, int y_ld, hipStream_t stream);

/* ------------------------------------------------------------------- sampler step
 * flair_predict_xstart: x0 = clamp(c_recip*x - c_recipm1*eps) with eps = first C of Cm
 * model channels (gaussian_diffusion.py:278-327).  flair_sampler_update: data
 * consistency x0 -= gamma*restored (+clamp), aux blend w*x0 + (1-w)*clamp(aux), prev_recon
 * pinning of the first prev_frames frames, eps' and the generalised DDIM update
 * (gaussian_diffusion.py:465-515).  All tensors (N,C,H,W) f32, flat length n. */
typedef struct {
    float gamma, w_aux;
    float sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod;
    float sqrt_alphas_cumprod_prev, sqrt_one_minus_alphas_cumprod_prev;
    float sqrt_one_minus_rho, sqrt_rho;
    int clip_denoised, nonzero;
    long frame_elems;
    int frames, prev_frames;
} flair_sampler_coefs;

int flair_predict_xstart(const float* x, const float* model_out, int N, int C, int Cm, int H, int W,
                         float c_recip, float c_recipm1, int clip, float* x0, hipStream_t stream);
int flair_sampler_update(const flair_sampler_coefs* c, const float* x, float* x0,
                         const float* restored, const float* aux, const float* z,
                         const float* prev_recon, long n, float* x_prev, hipStream_t stream);
/* out = clamp(a*x + b*y, lo, hi) on flat f32 tensors (y may be NULL): q_sample,
 * posterior mean, eps-from-x0 (gaussian_diffusion.py:206-248,361-365). */
int flair_axpby_f32(const float* x, const float* y, float a, float b, float lo, float hi, long n,
                    float* out, hipStream_t stream);
/* LEARNED_RANGE model variance (gaussian_diffusion.py:285-292) from channels [C,2C) of the
 * (N,2C,H,W) model output. */
int flair_learned_range_variance(const float* model_out, int N, int C, int H, int W, float min_log,
                                 float max_log, float* variance, float* log_variance,
                                 hipStream_t stream);
/* y[p][c] = (clamp(x[p][c]*a + b, lo, hi) - sub[c]) * mul[c] on f32 pixels (SPyNet input
 * normalisation: unet_new.py:1300 and mmedit SPyNet's mean/std). */
int flair_affine_channels_f32(const float* x, int x_ld, int C, long P, float a, float b, float lo,
                              float hi, const float* sub, const float* mul, float* y, int y_ld,
                              hipStream_t stream);
/* y = x + sigmoid(gate[f][c]) * (m - x): TemporalWrapper2's emb-gated residual mix
 * (sr3.py:203-226).  x, m, y: [F][HW] pixels of C channels; gate: [F][gate_ld] f32 logits.
 *   strides: x_ld / m_ld / y_ld at least C and multiples of 16 bytes, C a multiple of 4 (f32) / 8 (bf16); x, m, y 16-byte
 *            aligned (FLAIR_ERR_ARG naming the argument otherwise); gate rows may have any stride gate_ld >= C. */
int flair_gated_blend(const void* x, int x_ld, const void* m, int m_ld, const float* gate, int gate_ld,
                      int dtype, int C, int F, long HW, void* y, int y_ld, hipStream_t stream);
/* y = act(x0 + x1) on P pixels of C channels (x1 may be NULL): the residual sum of the RetinaFace detector's ResNet-50
 * Bottleneck (`out += identity; out = relu(out)`: torchvision resnet.py as built by
 * facelib/detection/retinaface/retinaface.py:99-102) and FPN's lateral sums (retinaface_net.py:88-94). */
int flair_add_act_nhwc(const void* x0, int x0_ld, const void* x1, int x1_ld, int dtype, int C, long P,
                       int act, void* y, int y_ld, hipStream_t stream);
/* nn.MaxPool2d(3, stride 2, padding 1) on [F][H][W][C] -> [F][(H+1)/2][(W+1)/2][C] (the stem of that ResNet-50). */
int flair_maxpool3x3s2_nhwc(const void* x, int x_ld, int dtype, int F, int H, int W, int C, void* y,
                            int y_ld, hipStream_t stream);
/* `conv_dw` of the detector's MobileNet-0.25 body (retinaface_net.py:25-33, built by MobileNetV1 at :100-135 for
 * retinaface.py:95-98, cfg_mnet at :31-49) on f32 [T][H][W][x_ld] clip tensors:
 *   d = act(depthwise3x3(x, w_dw) + b_dw)   groups = C, stride 1 or 2, zero padding 1, out ceil(H/s) x ceil(W/s)
 *   y = act(d @ w_pw^T + b_pw)              1x1 C -> Cout, in the same launch (d stays on chip)
 * w_dw: [9][C] (tap-major, BatchNorm scale folded in); w_pw: [Cout][C]; biases f32 [C] / [Cout] (NULL = 0).  w_pw == NULL:
 * y = d alone (Cout ignored).  act applies to both stages (ACT_LRELU01 for conv_dw).  C and Cout multiples of 4, C <= 512
 * with the 1x1 stage; y_ld >= the channels written; all pointers 16-byte aligned. */
int flair_dwconv_nhwc(const float* x, int x_ld, int T, int H, int W, int C, int stride, const float* w_dw,
                      const float* b_dw, const float* w_pw, const float* b_pw, int Cout, int act, float* y,
                      int y_ld, hipStream_t stream);
/* Depthwise 7x7 convolution of VQFR's TextureWarpingModule (`nn.Conv2d(c, c, groups=c, kernel_size=7, padding=3)`,
 * vqfr.py:394) on [T][H][W][x_ld] clip tensors, dtype F32 / BF16 (f32 accumulation):
 *   y[t][h][w][c] = bias[c] + sum_{i,j < 7} w[7i + j][c] * x[t][h + i - 3][w + j - 3][c]   (zero outside the frame)
 * stride 1, same size out.  w: [49][C] f32 (tap-major), bias: [C] f32 or NULL.  C a multiple of 8 (bf16) / 4 (f32);
 * x_ld >= C and y_ld >= C multiples of that; x, y, w, bias 16-byte aligned. */
int flair_dwconv7_nhwc(const void* x, int x_ld, int dtype, int T, int H, int W, int C, const float* w,
                       const float* bias, void* y, int y_ld, hipStream_t stream);
/* x[f][p][c] += bias[f][c]  (AttentionbottleBlock h + emb_out, unet_new.py:426-428). */
int flair_add_frame_bias(void* x, int dtype, int ld, int C, int F, long HW, const float* bias,
                         int bias_ld, hipStream_t stream);
/* dst[p][coff+c] = cast(src[p][c]): f32 flow fields into a conv input segment (th.cat at
 * unet_new.py:875). */
int flair_cast_channels(const float* src, int src_ld, int C, long P, void* dst, int dtype,
                        int dst_ld, int dst_coff, hipStream_t stream);
/* x[p][:] *= wmap[p]  (BasicVSR++ per-pixel vsrpp_weights, unet_new.py:739); ld >= C, 16-byte granular, x 16-byte aligned. */
int flair_scale_pixels(void* x, int dtype, int ld, int C, long P, const float* wmap,
                       hipStream_t stream);

/* ---------------------------------------------------------------------- attention
 * Spatial attention over the L tokens of each frame, per head of width d = head_dim
 * (unet_new.py:540-605).  qkv: [frames][L][ld]; q/k/v of head h start at channel
 * {q,k,v}_off + h*head_stride (legacy order: 0/d/2d + h*3d; new order: 0/C/2C + h*d);
 * out: [frames][L][out_ld], channel h*d + j.  scale multiplies q.k (1/sqrt(d)).
 * d = 32, 64, 128 and the multiples of 64 from 192 to 1024: MFMA kernels (bf16; from 192 the
 * head's channels are split across the waves of a workgroup) / exact row kernels (f32) at any
 * L; any other multiple of 8 runs on flair_attention_wide while d + L <= 2048; else -1. */
typedef struct {
    int dtype;
    int frames, L, heads, head_dim;
    int ld, out_ld;
    int q_off, k_off, v_off, head_stride;
    float scale;
} flair_attn_params;
int flair_qkv_attention(const flair_attn_params* p, const void* qkv, void* out, hipStream_t stream);

/* Temporal window attention per pixel (unet_new.py:473-515 + nn.py:370-386): query = own
 * frame, keys/values = the window-1 neighbouring frames (replicate padded), softmax scale
 * `scale` (flash_attn_func's default is 1/sqrt(head_dim)).  qkv: [T][H*W][ld] holding q|k|v
 * (C each, C/head_dim heads of head_dim channels); kpos: [window-1][C] f32 added to the
 * keys of each window slot (W_k applied to the positional code of that offset);
 * round_fp16 reproduces the reference's fp16 cast of q/k/v and of the result.
 * head_dim: a multiple of 8 from 8 to 256; 0 means 64 (ABI version <= 6 callers). */
typedef struct {
    int dtype;
    int T, H, W, C, window;
    int ld, out_ld;
    int round_fp16;
    float scale;
    int head_dim;
} flair_tattn_params;
int flair_temporal_attention(const flair_tattn_params* p, const void* qkv, const float* kpos,
                             void* out, hipStream_t stream);

/* ------------------------------------------------------------------ warps / resize
 * flow_warp (mmedit; unet_new.py:706,718,719): y[p] = bilinear(x, p + flow[p]),
 * flow [F][H][W] pixels of (dx,dy) f32, flow_ld floats apart; align_corners=True, zeros
 * (border=0) or border padding.
 *   strides: x_ld / y_ld at least C and multiples of 16 bytes, C a multiple of 4 (f32) / 8 (bf16); x, y 16-byte aligned;
 *            flow_ld even and >= 2; the source clip spans < 2 GiB (FLAIR_ERR_ARG otherwise). */
int flair_flow_warp(const void* x, int dtype, int x_ld, const float* flow, int flow_ld, int F,
                    int H, int W, int C, int border, void* y, int y_ld, hipStream_t stream);
/* out = f1 + warp(f2, f1) on flow fields (unet_new.py:716-718). */
int flair_flow_compose(const float* f1, const float* f2, int F, int H, int W, float* out,
                       hipStream_t stream);
/* The two warps of one BasicVSR++ propagation step with both flows given (unet_new.py:706,719):
 * cond1 = warp(prop, flow1), cond2 = warp(feat2, flow2); flow2 == NULL: first-order step (cond1 only).
 * The second-order flow (unet_new.py:716-718) depends on the optical flows alone, so the caller composes it
 * once per clip (flair_vsrpp_prep on the first denoising step) and reuses it for the other steps.
 * One frame: tensors are [H][W][*]; the flows are dense [H][W][2] f32.
 *   strides: prop_ld / feat2_ld / cond1_ld / cond2_ld at least C and multiples of 16 bytes, C a multiple of 4 (f32) /
 *            8 (bf16); prop, feat2, cond1, cond2 16-byte aligned (FLAIR_ERR_ARG naming the argument otherwise; feat2 and
 *            cond2 are looked at on a second-order step only); a source frame of H * W * ld elements spans < 2 GiB. */
int flair_vsrpp_warp2(const void* prop, int prop_ld, const void* feat2, int feat2_ld, const float* flow1,
                      const float* flow2, int dtype, int H, int W, int C, void* cond1, int cond1_ld,
                      void* cond2, int cond2_ld, hipStream_t stream);
/* One BasicVSR++ propagation step's alignment inputs in one launch (unet_new.py:704-722):
 * cond1 = warp(prop, flow1); flow2 = flow1 + warp(flow_prev, flow1); cond2 = warp(feat2, flow2);
 * flowpad[p][0..3] = (flow1, flow2) in the activation dtype (channels 4 .. pad_ld - 1 are left as they are).
 * flow_prev == NULL: first-order step (cond2 / flow2_out untouched, flowpad[2..3] = 0).  One frame: tensors are
 * [H][W][*]; flow1, flow_prev and flow2_out are dense [H][W][2] f32.
 *   strides: as flair_vsrpp_warp2 for prop / feat2 / cond1 / cond2; flowpad is an input segment of the offset convolution,
 *            so pad_ld is at least 4 and a multiple of 16 bytes and flowpad 16-byte aligned (FLAIR_ERR_ARG otherwise). */
int flair_vsrpp_prep(const void* prop, int prop_ld, const void* feat2, int feat2_ld,
                     const float* flow1, const float* flow_prev, int dtype, int H, int W, int C,
                     void* cond1, int cond1_ld, void* cond2, int cond2_ld, float* flow2_out,
                     void* flowpad, int pad_ld, hipStream_t stream);
/* mode 0/1: bilinear (align_corners False/True), 2: bicubic (A=-0.75), 3: 2x2 avg-pool,
 * 4: nearest;  x_ld, y_ld >= C;
 * channel 0 / 1 of the result are multiplied by scale_c0 / scale_c1 (flow rescaling). */
int flair_resize_nhwc(const void* x, int dtype, int x_ld, int F, int Hi, int Wi, int C, int mode,
                      int Ho, int Wo, void* y, int y_ld, float scale_c0, float scale_c1,
                      hipStream_t stream);

/* ------------------------------------------------- deformable alignment (DCNv2)
 * Fused offset/mask activation + modulated deformable 3x3 conv (unet_new.py:877-898;
 * same operator as dcn/src/deform_conv_cuda_kernel.cu:571-633 + deform_conv_cuda.cpp:540-560).
 *   x0|x1 : the two halves of the 2c input channels (feat_prop | feat_n2)
 *   raw   : conv_offset output, 27*G channels, pixel stride raw_ld, in TAP-MAJOR order
 *           (tap k owns the 3*G contiguous channels [3*G*k, 3*G*(k+1))):
 *             raw[3*G*k + 2*g + {0,1}] = (dy,dx) pre-activation of group g / tap k,
 *             raw[3*G*k + 2*G + g]     = mask pre-activation
 *           (the reference's o1|o2|mask order is 2*(g*9+k)+{0,1} and 18*G + g*9 + k; the
 *           caller permutes the output channels of the last conv_offset convolution once,
 *           when it packs that layer's weights).  G in {8, 16}; Cin/G a power of two.
 *   flow1, flow2 : [F][H][W][2] f32 or NULL (zero);  w : [Cout][9][Cin];  bias f32
 *   x_ld[i] >= Cin/2 and raw_ld multiples of 16 bytes; x0, x1, raw 16-byte aligned; y_ld >= Cout
 * raw_activated = 2 is the DCNv2Pack of VQFR's TextureWarpingModule (vqfr.py:341-427): the offsets are taken as they
 * are and only the mask goes through a sigmoid; flow1 = flow2 = NULL and x0 | x1 are the two channel halves of the one
 * input (x_main).  It also takes G = 4 and Cout up to 1024 (computed as cout slices of 64 or 128 in separate launches);
 * Cin from 64 (bf16: 32-channel K steps when Cin / 2 is not a multiple of 64). */
typedef struct {
    int dtype;
    int F, H, W;
    int Cin, Cout, G;
    int x_ld[2];
    int raw_ld, y_ld;
    float max_residue_magnitude;
    int raw_activated; /* 1: raw already holds max_residue_magnitude*tanh / sigmoid values
                        * (produced with FLAIR_ACT_DCN_OFFSETS); 0: pre-activations;
                        * 2: offsets as they are, mask = sigmoid (max_residue_magnitude unused) */
} flair_dcn_params;
int flair_dcn_align(const flair_dcn_params* p, const void* x0, const void* x1, const void* raw,
                    const float* flow1, const float* flow2, const void* w, const float* bias,
                    void* y, hipStream_t stream);

/* ------------------------------------------------- degradation operators (restore_fn)
 * Images here are the sampler's (N,C,H,W) f32 tensors.
 *
 * flair_depthwise_filter: pseudoSR's Filter_Layer (pseudoSR.py:15-44,174-246): every plane is
 * cross-correlated with one kh x kw filter after replication padding:
 *   out[i][j] = sum_{u,v} K[u][v] * IN(i*out_stride + out_offset + u - pad, j*... + v - pad)
 * where IN clamps to the virtual image of size (Hin*stuff, Win*stuff) whose samples are zero
 * except at coordinates == stuff_offset (mod stuff) (zero-stuffing up-sampler).
 *   Down  : pad 4, out_stride 4, out_offset pre_stride;  InvHtH: pad 19;  Up: stuff 4.
 * reflect != 0 uses F.pad(mode="reflect") instead of replication (imresize_efficient, the
 * forward operator A: imresize_pseudoSR.py:163-178): one reflection only, as there -- a call whose taps reach more
 * than size - 1 beyond a border of the (virtual) plane is refused. */
int flair_depthwise_filter(const float* x, int planes, int Hin, int Win, const float* filt, int kh,
                           int kw, int pad, int out_stride, int out_offset, int stuff,
                           int stuff_offset, int Hout, int Wout, int reflect, float* y,
                           hipStream_t stream);
/* jpeg_decode(jpeg_encode(x, qf), qf) of jpeg.py:72-167 on (N,3,S,S) images in [-1,1].
 * q_luma, q_chroma, dct8 are HOST arrays of 64 floats (quantisation tables of
 * general_quant_matrix, jpeg.py:35-65, and the 8x8 orthonormal DCT-II matrix); workspace:
 * N*3*S*S device floats.  luma_q / chroma_q (both or neither, may be NULL): the quantised integer
 * levels round(DCT / q) that jpeg_encode returns (jpeg.py:108-114), as f32 planes (N,1,S,S) and
 * (N,2,S/2,S/2) in the reference's block layout. */
int flair_jpeg_roundtrip(const float* x, int N, int S, const float* q_luma, const float* q_chroma,
                         const float* dct8, float* workspace, float* y, float* luma_q, float* chroma_q,
                         hipStream_t stream);
/* The same round trip on rectangular images (N,3,H,W), H % 16 == 0 and W % 16 == 0 (H == W allowed): the codec is
 * independent per 16x16 MCU, so nothing but the indexing knows the frame's shape.  One launch and no workspace: a
 * wave owns ten MCUs, keeps their YCbCr blocks in LDS and gives each 8x8 block (four luma, Cb, Cr per MCU) to one
 * lane.  Every value goes through the expressions of flair_jpeg_roundtrip (shared device functions), so on square
 * input the two entries agree bit for bit, level planes included.  Tables and level planes as above: luma_q
 * (N,1,H,W), chroma_q (N,2,H/2,W/2), both or neither.  Offsets are 64-bit; N*(H/16)*(W/16)/10 must stay below 2^31. */
int flair_jpeg_roundtrip_hw(const float* x, int N, int H, int W, const float* q_luma, const float* q_chroma,
                            const float* dct8, float* y, float* luma_q, float* chroma_q, hipStream_t stream);
/* C[b] = A[b] (MxK) * B[b] (KxN), row-major f32; a stride of 0 shares the matrix across the
 * batch.  SRConv's separable U/V products (restore_util.py:102-227).  batch and ceil(M / 16) are grid extents:
 * at most 65535 each, refused beyond. */
int flair_matmul_f32(const float* A, long a_batch_stride, const float* B, long b_batch_stride,
                     float* C, int batch, int M, int N, int K, hipStream_t stream);
/* Resizer (resizer.py:54-73) along one axis of a tensor viewed [outer][Lin][inner]:
 * y[o][i][n] = sum_k w[k][i] * x[o][fov[k][i]][n]; fov int32 [taps][Lout], w f32 [taps][Lout]. */
int flair_gather_mac_f32(const float* x, long outer, int Lin, long inner, const int* fov,
                         const float* w, int taps, int Lout, float* y, hipStream_t stream);

/* ------------------------------------------------------------- CodeFormer auxiliary prior
 * (guided_diffusion/codeformer.py, called from gaussian_diffusion.py:471-496 as
 * aux_model(pred_xstart, t, x)).  Its convolutions, GroupNorms, 1x1 projections and 8 x 64 multi-head attention
 * run on the entry points above; these are the pieces only the prior needs. */
/* nn.LayerNorm(C) over the channels of each of `rows` pixels (codeformer.py:541-542, :639), eps inside the
 * square root.  Optional second output y2 = y + pos[row % pos_rows][C] (q = k = norm(x) + pos, :561-562).
 *   limits : C a multiple of 4 (f32) / 8 (bf16), at most 1024 (f32) / 2048 (bf16): a wave holds the row, four 16-byte
 *            pieces per lane.
 *   strides: x_ld / y_ld / y2_ld at least C and multiples of 16 bytes; x, y, y2 16-byte aligned (FLAIR_ERR_ARG naming the
 *            argument otherwise; y2_ld is looked at only when y2 is given); gamma, beta, pos dense f32. */
int flair_layernorm_nhwc(const void* x, int dtype, int x_ld, long rows, int C, const float* gamma,
                         const float* beta, float eps, void* y, int y_ld, const float* pos, int pos_rows,
                         void* y2, int y2_ld, hipStream_t stream);
/* Attention with heads of any width (AttnBlock.forward, codeformer.py:217-241: one head of C = 512 over the 256
 * pixels of the 16x16 level).  Same layout contract as flair_qkv_attention; head_dim a multiple of 8 (bf16) / 4
 * (f32), 64 * (head_dim + L) bytes of LDS <= 128 KiB.  A 16-row VALU kernel: flair_qkv_attention calls it only for
 * widths it has no MFMA kernel for (multiples of 8 other than 32, 64, 128 and 192 ... 1024 in steps of 64).
 *   strides: ld, out_ld, q_off, k_off, v_off and head_stride multiples of 16 bytes; the last head fits its row,
 *            max(q_off, k_off, v_off) + (heads - 1) * head_stride + head_dim <= ld, and heads * head_dim <= out_ld; qkv and
 *            out 16-byte aligned (FLAIR_ERR_ARG otherwise: the rules of flair_qkv_attention). */
int flair_attention_wide(const flair_attn_params* p, const void* qkv, void* out, hipStream_t stream);
/* idx[row] = argmax_n logits[row][n] (softmax + topk(1) of codeformer.py:727-728; first index on ties) and
 * y[row][0..D) = codebook[idx[row]] (VectorQuantizer.get_codebook_feat, :82-94).  codebook: [N][D] f32.
 * forced_idx (or NULL): use these indices instead of the arg-max (tests).  idx may be NULL. */
int flair_argmax_codebook(const void* logits, int dtype, int ld, long rows, int N, const float* codebook, int D,
                          const int* forced_idx, int* idx, void* y, int y_ld, hipStream_t stream);
/* Nearest codebook row of every token (VectorQuantizer.forward of RestoreFormer, restoreformer.py:43-62): idx[row] =
 * argmin_n |z|^2 + |e_n|^2 - 2 z.e_n over the f32 distances (first index on ties, as torch.min), z = the D channels of
 * row `row` of an NHWC tensor (stride ld, dtype F32 / BF16, read as f32), and y[row][0..D) = codebook[idx[row]] in
 * that dtype.  codebook: [N][D] f32, 16-byte aligned; D a multiple of 4, <= 1024.  forced_idx (or NULL): use these
 * indices instead of the search (tests; z may then be NULL).  idx may be NULL. */
int flair_vq_nearest_nhwc(const void* z, int dtype, int ld, long rows, int D, const float* codebook, int N,
                          const int* forced_idx, int* idx, void* y, int y_ld, hipStream_t stream);
/* adaptive_instance_normalization(content, style) of codeformer.py:437-470 on [frames][HW][C] tensors:
 * per (frame, channel) mean and sqrt(unbiased variance + eps) of both, y = (content - mc) / sc * ss + ms. */
int flair_adain_nhwc(const void* content, int c_ld, const void* style, int s_ld, int dtype, int frames, int HW,
                     int C, float eps, void* y, int y_ld, hipStream_t stream);
/* Fuse_sft_block tail (codeformer.py:595-596): y = dec + w * (dec * scale + shift) over n dense elements.
 *   strides: none (dense); n a multiple of 4 (f32) / 8 (bf16); dec, scale, shift, y 16-byte aligned (FLAIR_ERR_ARG naming
 *            the pointer otherwise). */
int flair_sft_fuse(const void* dec, const void* scale, const void* shift, float w, int dtype, long n, void* y,
                   hipStream_t stream);

/* ------------------------------------------------------------- BiSeNet face parsing (facelib/parsing/bisenet.py)
 * The second parser of facelib/parsing/__init__.py:8-25.  Its convolutions, the stem pool, the residual sums and the nearest
 * enlargements run on the entry points above; these are the pieces only it needs.  All three take F32 / BF16 NHWC tensors
 * with explicit pixel strides, refuse a stride or pointer that breaks their 16-byte accesses with FLAIR_ERR_ARG, and use no
 * float atomics (fixed summation order: a replayed graph gives the same bits). */
/* F.avg_pool2d(feat, feat.size()[2:]) (bisenet.py:45, :70, :100): y[f][c] = mean over the H*W pixels of x[f][.][.][c], f32.
 * C and x_ld multiples of 4 (F32) / 8 (BF16), x 16-byte aligned; y: [F][y_ld] f32, y_ld >= C. */
int flair_global_avgpool_nhwc(const void* x, int dtype, int x_ld, int F, int H, int W, int C, float* y, int y_ld,
                              hipStream_t stream);
/* y = x * g[f][c] (+ x if add_x) (+ bias[f][c]) (+ a) on [F][HW] pixels of C channels.  gate: [F][gate_ld] f32, a gate or,
 * with gate_is_logit != 0, its pre-sigmoid logit (g = 1 / (1 + exp(-gate))); bias: [F][bias_ld] f32 or NULL; a: a full
 * tensor of x's dtype (pixel stride a_ld) or NULL.  One launch each for torch.mul(feat, atten) + avg_up of arm32
 * (bisenet.py:49, :74-75: avg_up is a 1x1 map enlarged by nearest, i.e. `bias`), arm16(feat16) + feat32_up (:79-80: `a`)
 * and feat * atten + feat of FeatureFusionModule (:105-106: add_x).  y may alias x.  C, x_ld, y_ld, a_ld multiples of
 * 4 (F32) / 8 (BF16); x, y, a 16-byte aligned. */
int flair_channel_gate_nhwc(const void* x, int x_ld, int dtype, int F, long HW, int C, const float* gate, int gate_ld,
                            int gate_is_logit, int add_x, const float* bias, int bias_ld, const void* a, int a_ld,
                            void* y, int y_ld, hipStream_t stream);
/* idx[f][Y][X] = argmax_n of F.interpolate(logits, (H, W), mode='bilinear', align_corners=True)[f][n][Y][X] (bisenet.py:127
 * followed by the .argmax(dim=1) of facelib/utils/face_restoration_helper.py:279-281 and scripts/video_sample.py:428-429),
 * first index on ties, without the enlarged tensor: logits [F][h][w] pixels of N <= 32 classes (pixel stride ld >= N, dtype
 * F32 / BF16, blended in f32 with ATen's arithmetic: source = dst * (h - 1) / (H - 1) in float, the four-term blend).
 * H == h, W == w is the plain arg-max.  idx: [F][H][W] int32 (or NULL); y (or NULL): [F][H][W] rows of f32, stride y_ld,
 * y[row][0..D) = table[idx[row]] with table [N][D] f32 (the face_weight table of video_sample.py:431). */
int flair_upsample_argmax_nhwc(const void* logits, int dtype, int ld, int F, int h, int w, int N, int H, int W,
                               const float* table, int D, int* idx, float* y, int y_ld, hipStream_t stream);

/* ------------------------------------------------------------- un-aligned prior branch: face crop / inverse paste
 * (second half; gaussian_diffusion.py:476-493 calls facelib/utils/face_restoration_helper.py:225-254
 * and :264-335 every denoising step and round-trips the frames through numpy / OpenCV).  Images are the sampler's
 * (N,C,H,W) f32 tensors; the affine matrices are an INPUT (computed once per window, scripts/video_sample.py:446-448).
 * OpenCV's arithmetic is restated from its published algorithm (cv2 absent here: parity unpinned). */
/* cv2.warpAffine(src, M, (Wd, Hd), flags=INTER_CUBIC, borderMode=BORDER_CONSTANT, borderValue=border) per image n.
 * minv: DEVICE [N][6] doubles, the dst -> src matrix warpAffine derives from M (its inverse, computed in double on the
 * host exactly as imgwarp.cpp does).  src: [N][C][Hs][Ws] f32, or f64 when src_is_f64 (masks).  border: HOST floats [C].
 * pre = 1 applies clamp((x + 1) / 2, 0, 1) * 255 to every source sample (face_restoration_helper.py:230), post = 1 applies
 * clamp((y / 255 - 0.5) / 0.5, -1, 1) to the result (:246-253); dst: [N][C][Hd][Wd] f32.  C <= 4. */
int flair_warp_affine_cubic(const void* src, int src_is_f64, int N, int C, int Hs, int Ws, const double* minv,
                            int Hd, int Wd, const float* border, int pre, int post, float* dst, hipStream_t stream);
/* flair_warp_affine_cubic with a source index per output image: dst image n is cropped from src image src_index[n]
 * (DEVICE int32 [N], every entry in [0, Nsrc)), so several faces come out of one frame without a copy of the frame
 * (face_restoration_helper.py:225-254 applied per face).  src: [Nsrc][C][Hs][Ws]; minv: [N][6]; dst: [N][C][Hd][Wd].  Same
 * kernel and arithmetic as flair_warp_affine_cubic: with src_index = 0 .. N-1 the two agree bit for bit.  N = 0 is a no-op. */
int flair_warp_affine_cubic_indexed(const void* src, int src_is_f64, int Nsrc, const int* src_index, int N, int C, int Hs,
                                    int Ws, const double* minv, int Hd, int Wd, const float* border, int pre, int post,
                                    float* dst, hipStream_t stream);
/* The paste of any number of faces per frame in one launch: per output pixel, v = x0, then for every face k of the pixel's
 * frame in list order  f = flair_warp_affine_cubic(faces[k], minv[k], pre = 1, post = 1, border 0),
 * m = (float) flair_warp_affine_cubic(masks[k], minv[k]) (the f64 form),  v = v * (1 - m) + f * m  -- inverse_faces' two warps
 * (face_restoration_helper.py:264-335) and the blend of gaussian_diffusion.py:491 composed per face; a later face lands on top
 * of an earlier one, and the result equals those three launches applied face by face bit for bit.  (The reference pastes
 * exactly one face per frame.)  x0, out: [T][C][H][W] f32, C <= 4, out may not overlap x0; faces: [K][C][h][w] f32 in
 * [-1, 1]; masks: [K][1][h][w] f64 (flair_face_mask_blur's result); minv: DEVICE [K][6] doubles, dst -> src; frame_start:
 * DEVICE int32 [T + 1], faces sorted by frame, frame t owns faces frame_start[t] .. frame_start[t + 1] - 1 (non-decreasing,
 * frame_start[0] = 0, frame_start[T] = K: checked by the caller on its host copy).  (H, W) and (h, w) are independent.
 * K = 0 copies x0 (faces, masks, minv may then be null). */
int flair_face_paste(const float* x0, int T, int C, int H, int W, const float* faces, const double* masks, const double* minv,
                     int K, int h, int w, const int* frame_start, float* out, hipStream_t stream);
/* The paste mask of inverse_faces (face_restoration_helper.py:283-317): mask = lut[parse_idx] (MASK_COLORMAP, DEVICE
 * doubles [nlut]), `repeats` x cv2.GaussianBlur(mask, (ksize, ksize), sigma) in float64 with BORDER_REFLECT_101 (kern:
 * DEVICE doubles [ksize] = cv2.getGaussianKernel), the `edge` outermost pixels zeroed, / div.  parse_idx: [N][H][W]
 * int32 (flair_argmax_codebook's idx); tmp, mask: [N][H][W] doubles (mask is the result). */
int flair_face_mask_blur(const int* parse_idx, int N, int H, int W, const double* lut, int nlut, const double* kern,
                         int ksize, int repeats, int edge, double div, double* tmp, double* mask, hipStream_t stream);
/* x0 * (1 - mask) + face * mask (gaussian_diffusion.py:491); x0, face, out: [N][C][H][W] f32; mask: [N][1][H][W] f32. */
int flair_face_blend(const float* x0, const float* face, const float* mask, int N, int C, int H, int W, float* out,
                     hipStream_t stream);

/* ------------------------------------------------------------- YOLOv5-face detectors (facelib/detection/yolov5face)
 * The operations of YOLOv5n / YOLOv5l that are neither a convolution (flair_conv_nhwc with FLAIR_ACT_SILU, flair_dwconv_nhwc)
 * nor a nearest enlargement (flair_resize_nhwc).  Clip tensors [F][H][W][ld]; every view's pixel stride may exceed its
 * channel count (channels past C are never written), pointers and strides are 16-byte granular, and every entry validates
 * before it launches (FLAIR_ERR_ARG with a message that names the argument).
 *
 * flair_maxpool2x2s2_nhwc: nn.MaxPool2d(kernel_size=2, stride=2, ceil_mode=True) of StemBlock (models/common.py:63, :70):
 *   [F][H][W][C] -> [F][(H+1)/2][(W+1)/2][C], windows clipped at the bottom / right edge.  F32 / BF16, C a multiple of
 *   4 / 8; bit-exact.  y is usually the second channel slice of the buffer stem_3 reads (the torch.cat of :71). */
int flair_maxpool2x2s2_nhwc(const void* x, int x_ld, int dtype, int F, int H, int W, int C, void* y, int y_ld,
                            hipStream_t stream);
/* The three nn.MaxPool2d(k, stride 1, padding k // 2) of SPP (models/common.py:173-184) in one launch: reads channels
 * [0, C) of buf ([F][H][W][ld], ld >= 4 C) and writes the pools for k0 < k1 < k2 (odd, 3 .. 13) into channels [C, 2C),
 * [2C, 3C), [3C, 4C) of the same buffer -- so SPP.cv1 writes slice 0 and SPP.cv2 reads one 4C-channel segment, the
 * torch.cat of :184.  Padding behaves as -inf; bit-exact.  F32 / BF16, C a multiple of 4 / 8. */
int flair_spp_maxpool_nhwc(void* buf, int ld, int dtype, int F, int H, int W, int C, int k0, int k1, int k2,
                           hipStream_t stream);
/* torch.cat((a, b), 1) followed by channel_shuffle(., 2) of ShuffleV2Block (models/common.py:25-34, :163-170):
 * y[p][2i] = a[p][i], y[p][2i+1] = b[p][i] on P pixels; a, b: C channels each (a is usually the untouched half of a
 * stride-1 unit's input, a strided view), y: 2C channels.  F32 / BF16, C a multiple of 4 / 8; bit-exact. */
int flair_channel_interleave_nhwc(const void* a, int a_ld, const void* b, int b_ld, int dtype, int C, long P, void* y,
                                  int y_ld, hipStream_t stream);
/* Detect.forward's inference branch for one level (models/yolo.py:52-86) on the head convolution's NHWC output
 * x: [B][ny][nx][x_ld] f32 with channel a * 16 + j = output j of anchor a (what view(bs, na, no, ny, nx).permute(0, 1, 3,
 * 4, 2) reorders).  Writes rows [b][row0 + a ny nx + y nx + x][0..16) of z: [B][N][16] f32 (three launches fill z; no
 * torch.cat): columns 0-1 (2 sigmoid - 0.5 + grid) * stride, 2-3 (2 sigmoid)^2 * anchor_grid, 4 and 15 sigmoid, 5-14
 * v * anchor_grid + grid * stride.  anchor_grid: HOST array [na][2] (w, h) in pixels (copied into the launch arguments);
 * na <= 8; no must be 16 (nc = 1); row0 + na ny nx <= N. */
int flair_yolo_face_decode(const float* x, int x_ld, int B, int ny, int nx, int na, int no, float stride,
                           const float* anchor_grid, float* z, long N, long row0, hipStream_t stream);
/* YoloDetector._preprocess with letterbox (face_detector.py:56-79, utils/datasets.py:5-35) in one launch:
 * src: [B][3][H][W] f32 NCHW frames -> y: [B][Ho][Wo][y_ld] f32 clip tensor, channels 0-2 the image, 3-15 zero.
 * Every source value is first mapped to clamp(a x + b, lo, hi); the new_h x new_w interior at (top, left) is that image
 * (copied when new_h == H and new_w == W, else sampled bilinearly with half-pixel centres and clamped edges, cv2.INTER_LINEAR
 * on floats = F.interpolate(mode="bilinear", align_corners=False) at an explicit size) times s; every other pixel is
 * pad_value (114 / 255).  The host computes new_h, new_w, top, left, Ho, Wo as the reference does. */
int flair_letterbox_nhwc(const float* src, int B, int H, int W, int new_h, int new_w, int top, int left, int Ho, int Wo,
                         float a, float b, float lo, float hi, float s, float pad_value, float* y, int y_ld,
                         hipStream_t stream);

/* ------------------------------------------------------------- SuperSloMo frame interpolation (guided_diffusion/superslomo.py)
 * The per-timestep tail of SuperSloMo.forward around the interpolation UNet; everything else of the network is
 * flair_conv_nhwc (FLAIR_ACT_LRELU01) and flair_resize_nhwc (modes 0 and 3).  Both entries use the reference's back_warp
 * (superslomo.py:225-247), which is NOT flair_flow_warp's convention: x = w + u, gx = 2 (x / W - 0.5), then F.grid_sample with
 * its defaults (bilinear, zeros padding, align_corners=False), i.e. ix = ((gx + 1) W - 1) / 2: the sample sits half a pixel
 * up-left of w + u, and corners outside the frame contribute zero.  f32 arithmetic in the reference's order of operations.
 * Clip tensors [B][H][W][ld] in the activation dtype (F32 / BF16), any H, W >= 1:
 *   pair: the normalised frames ((frame + 1) / 2 - mean), i0 in channels 0-2, i1 in 3-5;
 *   flow: the flow UNet's output, f01 in channels 0-1, f10 in 2-3, each (u, v) in pixels;
 *   strides: every *_ld at least the channels named and a multiple of 16 bytes, every pointer 16-byte aligned (FLAIR_ERR_ARG
 *            naming the argument otherwise); a clip of B H W ld elements spans < 2 GiB.
 *
 * flair_slomo_warp_pack, stage A (:260-270): ft0 = c0 f01 + c1 f10, ft1 = c2 f01 + c3 f10 and
 *   out[p] = (i0, i1, f01, f10, ft1, ft0, back_warp(i1, ft1), back_warp(i0, ft0)), 20 channels in the reference's torch.cat
 *   order, zeros in channels 20 .. out_c - 1 (out_c: 20 .. 32, a multiple of 16 bytes: the padded input of interp.conv1). */
int flair_slomo_warp_pack(const void* pair, int pair_ld, const void* flow, int flow_ld, int dtype, int B, int H, int W,
                          float c0, float c1, float c2, float c3, void* out, int out_ld, int out_c, hipStream_t stream);
/* flair_slomo_blend, stage B (:273-287): io is the interpolation UNet's output (>= 5 channels); ft0 and ft1 are recomputed
 *   from the flows; ft0f = io[0:2] + ft0, ft1f = io[2:4] + ft1, v0 = sigmoid(io[4]), v1 = 1 - v0, g0 = back_warp(i0, ft0f),
 *   g1 = back_warp(i1, ft1f), out = (((1 - t) v0 g0 + t v1 g1) / ((1 - t) v0 + t v1) + mean[c]) * 2 - 1 with 1 - t taken in
 *   double (0 < t < 1).  mean: HOST array of 3 floats.  out: f32 NCHW, frame b at out + b * out_batch_stride (>= 3 H W
 *   floats), so a call fills slot [:, k] of a (B, factor - 1, 3, H, W) tensor. */
int flair_slomo_blend(const void* pair, int pair_ld, const void* flow, int flow_ld, const void* io, int io_ld, int dtype,
                      int B, int H, int W, float c0, float c1, float c2, float c3, double t, const float* mean, float* out,
                      long out_batch_stride, hipStream_t stream);

/* ------------------------------------------------------------- AMT-G frame interpolation (amt.hip)
 * What guided_diffusion/amt.py and amt_blocks/ need beyond convolutions, resizes and flair_flow_warp (border).  All f32.
 *
 * The correlation volume (raft.py:142-163, :201-209).  BidirCorrBlock.corr is fmap1^T fmap2 / sqrt(dim): the product is
 * flair_matmul_f32 on the NHWC feature map of one frame and the NCHW copy of the other (corr), and once more with the two
 * frames swapped (corr_T: no permuted copy), each followed by flair_corr_scale, a true division in place (n floats at x,
 * 16-byte aligned; divisor positive and finite).  A volume is B h w planes of h x w floats, dense; flair_corr_pool makes the
 * next pyramid level, F.avg_pool2d(., 2, stride=2) per plane: dst is planes x (h / 2) x (w / 2), odd sizes floor, h, w >= 2;
 * ((a + b) + c) + d in row-major order, times 1/4.  64-bit offsets; src, dst 4-byte aligned. */
int flair_corr_scale(float* x, long n, float divisor, hipStream_t stream);
int flair_corr_pool(const float* src, long planes, int h, int w, float* dst, hipStream_t stream);
/* BidirCorrBlock.__call__ (raft.py:165-199) on the coordinates of AMT._corr_scale_lookup (amt.py:98-111), radius 3.
 *   corr, corr_t : HOST arrays of `levels` (1 .. 4) device pointers, level l of each direction: B h w planes of
 *                  level_h[l] x level_w[l] floats (HOST int arrays), plane q belonging to query pixel q of the [B][h][w] grid.
 *                  A level is either >= 2 on both sides (sampled) or 1 x 1 (its value goes to all 49 taps, raft.py:186-188);
 *                  FLAIR_ERR_ARG on any other size, where the reference raises.
 *   flow         : [B][h][w] pixels of (flow0.x, flow0.y, flow1.x, flow1.y), flow_ld floats apart.
 *   out          : [B][h][w] pixels, out_ld floats apart; channels [0, 49 levels) receive corr sampled around
 *                  (x, y) + flow1 * scale_corr, channels [49 levels, 98 levels) corr_t around (x, y) + flow0 * scale_corr_t
 *                  (scale_corr = 1 / t, scale_corr_t = 1 / (1 - t) in the reference), level-major, tap 7 a + b of a level at
 *                  centre / 2^l + (a - 3, b - 3): the first tap axis moves x (raft.py:177-184).  Nothing else is written,
 *                  so out may be the 392-channel head of convc1's zero-padded 400-channel input segment.
 *   Bilinear, align_corners=True, zeros outside the plane; each coordinate step rounded to f32 as in the reference; the
 *   pixel -> [-1, 1] -> pixel round trip of bilinear_sampler is the identity and is not repeated (integer coordinates return
 *   volume entries bit for bit).  Coordinates must be finite.
 *   strides: flow_ld >= 4 and a multiple of 4 floats, flow 16-byte aligned; out_ld >= 98 levels, out and the planes 4-byte
 *            aligned (the results leave as 4-byte stores, 49 consecutive ones per wave and level); FLAIR_ERR_ARG naming the
 *            argument otherwise; 64-bit offsets, at most 2^31 workgroups of two queries. */
int flair_corr_lookup(const float* const* corr, const float* const* corr_t, const int* level_h, const int* level_w, int levels,
                      const float* flow, int flow_ld, int B, int h, int w, float scale_corr, float scale_corr_t, float* out,
                      int out_ld, hipStream_t stream);
/* y = prelu(x0 (+ x1), slope[c]) = v > 0 ? v : slope[c] v on P pixels of C channels: nn.PReLU(C) behind a convolution
 * (ifrnet.py:10-14) and ResBlock's prelu(x + out) (:52).  x1 may be NULL; y may be x0 or x1 (each thread reads what it
 * writes).  A separate launch on purpose: the convolution epilogues stay as they are.
 *   strides: C a multiple of 4; x0_ld / x1_ld / y_ld at least C and multiples of 4 floats; x0, x1, y, slope 16-byte aligned. */
int flair_prelu_nhwc(const float* x0, int x0_ld, const float* x1, int x1_ld, const float* slope, int C, long P, float* y,
                     int y_ld, hipStream_t stream);
/* x [F][H][W][4 C] -> y [F][2 H][2 W][C]: y(2 m + py, 2 n + px, c) = x(m, n, (2 py + px) C + c).  With the host-side repack
 * of a ConvTranspose2d(4, 2, 1) weight into a 3 x 3 convolution of 4 C outputs (flair_amd.ops.
 * deconv_as_conv3x3) this is nn.ConvTranspose2d(Cin, C, 4, 2, 1) of ifrnet.py:84, :100 and multi_flow.py:65.
 *   strides: C a multiple of 4; x_ld >= 4 C, y_ld >= C, multiples of 4 floats; x, y 16-byte aligned. */
int flair_depth_to_space2_nhwc(const float* x, int x_ld, int F, int H, int W, int C, float* y, int y_ld, hipStream_t stream);

/* y = a x0 + b x1 on P pixels of C channels (x1 may be NULL: y = a x0), each product rounded before the sum, as ATen does
 * `delta + 2.0 * resize(flow, 2.0)` (ifrnet.py:109-110) and `flow + scale_factor * resize(delta_flow, scale_factor)`
 * (raft.py:138 with amt.py:161-162).  y may be x0 or x1.  strides as flair_prelu_nhwc. */
int flair_axpby_nhwc(const float* x0, int x0_ld, float a, const float* x1, int x1_ld, float b, int C, long P, float* y, int y_ld,
                     hipStream_t stream);
/* The tail of one timestep for num_flows = 5 (multi_flow.py).  flair_amt_multiflow_prepare is MultiFlowDecoder.forward behind
 * its convblock (:73-83): dec holds the 40 channels delta_flow0 (10) | delta_flow1 (10) | mask (5) | img_res (15), up the
 * 4 channels resize(flow0 | flow1, 2.0); out = (delta_flow0 + 2 up[0:2] five times | delta_flow1 + 2 up[2:4] five times |
 * sigmoid(mask) | img_res).  flair_amt_multiflow_combine is multi_flow_combine up to comb_block (:27-54): pair holds the
 * mean-free frames (img0 in channels 0-2, img1 in 3-5), prep the 40 channels above at the frames' size, neg_mean[f *
 * neg_mean_ld] minus the pair's mean (device); per flow i, x[3 i + c] = mask_i warp(img0, flow0_i) + (1 - mask_i)
 * warp(img1, flow1_i) + mean + img_res_i with flow_utils.warp (bilinear, border, align_corners=True), x[15] = 0 (the padded
 * input of comb_block[0]), avg[c] = the mean of x[3 i + c] over i, avg[3] = 0.
 *   strides: every *_ld at least the channels named (pair 6, prep / dec / out 40, up 4, x 16, avg 4) and a multiple of 4
 *            floats, every pointer 16-byte aligned (FLAIR_ERR_ARG naming the argument otherwise); 64-bit offsets. */
int flair_amt_multiflow_prepare(const float* dec, int dec_ld, const float* up, int up_ld, long P, float* out, int out_ld,
                                hipStream_t stream);
int flair_amt_multiflow_combine(const float* pair, int pair_ld, const float* prep, int prep_ld, const float* neg_mean,
                                int neg_mean_ld, int B, int H, int W, float* x, int x_ld, float* avg, int avg_ld,
                                hipStream_t stream);

/* nn.InstanceNorm2d(C) (no affine, biased variance) + activation (FLAIR_ACT_NONE or FLAIR_ACT_RELU) on [F][H][W] pixels of C
 * channels: feat_enc.py:86-114 with norm_fn='instance'.  Two-pass: the mean, then the variance of the centred values, summed
 * in double over fixed pixel ranges in a fixed order (bitwise reproducible), y = act((x - mean) * rstd) in f32.
 * (flair_groupnorm_nhwc with groups = C is the one-pass var = E[x^2] - mean^2 and misses the f32 ATen deviation on planes
 * whose mean is a few standard deviations.)  y must not alias x.
 *   workspace: flair_instnorm_workspace_bytes(F, H, W, C) bytes, 16-byte aligned, contents irrelevant.
 *   strides: C a multiple of 4; x_ld / y_ld at least C and multiples of 4 floats; x, y 16-byte aligned; F <= 65535. */
size_t flair_instnorm_workspace_bytes(int F, int H, int W, int C);
int flair_instnorm_nhwc(const float* x, int x_ld, int F, int H, int W, int C, double eps, int act, float* y, int y_ld,
                        void* workspace, size_t workspace_bytes, hipStream_t stream);
/* ------------------------------------------------------------- multi-GPU start-up
 * The only collective of the path: in-place RCCL broadcast of the kernel-native weight blob (flair_amd.checkpoint.export_packed:
 * bf16 [Cout][taps][Cin] conv weights, batched embedding matrix, f32 biases ...) from `root` to every rank of `rccl_comm`
 * (an ncclComm_t of the host process), enqueued on `stream`.  Replaces dist_util.py:40-79 (pickled-chunk load_state_dict +
 * one broadcast per parameter).  librccl is bound with dlopen at the first call.  Clips are independent after that: no
 * data-path collective exists. */
int flair_bcast_weights(void* blob, size_t bytes, int root, void* rccl_comm, hipStream_t stream);

/* ------------------------------------------------------------- image metrics (python -m flair_amd evaluate)
 * No counterpart in the reference, which ships no scoring tool: squared error and SSIM of two sets of WRITTEN frames.
 * a, b: dense [N][H][W][3] uint8 RGB (what flair_amd.io.decode_frame yields after the HWC transpose and io.to_bytes produces).
 * out: [N][4] doubles per frame n: out[4n] = sum of (a - b)^2 over the 3 H W byte values, the exact integer (32-bit integer
 * partials, summed in double: exact below 2^53); out[4n + 1 .. 4n + 3] = sums of the SSIM map of R, G, B over its
 * (H - 10) x (W - 10) valid region: the restoration definition (Wang et al. 2004, as BasicSR computes it on RGB) on the 0..255
 * scale: 11 x 11 Gaussian window, sigma 1.5, normalised to sum 1, applied separably without padding; mu_x, mu_y,
 * var_x = E[x^2] - mu_x^2, var_y, cov_xy; C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2;
 * ssim = (2 mu_x mu_y + C1)(2 cov_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(var_x + var_y + C2)), moments in f32 on values shifted by
 * -128.  PSNR = 10 log10(255^2 * 3 H W / out[4n]) and the mean SSIM = (out[4n+1] + out[4n+2] + out[4n+3]) / (3 (H-10)(W-10)) are
 * the caller's arithmetic (flair_amd.metrics).  One workgroup per 32 x 64 tile of one (frame, channel) writes one partial into
 * ws; a second launch sums each frame's partials in a fixed order: no floating-point atomics, so a frame's four values are the
 * same bits in every run and for every N.  ws: flair_image_metrics_workspace(N, H, W) bytes (0 for a shape the entry refuses),
 * 8-byte aligned, contents irrelevant.  H, W >= 11, N >= 1; offsets are 64-bit (N H W 3 may exceed 2^31). */
size_t flair_image_metrics_workspace(int N, int H, int W);
int flair_image_metrics(const uint8_t* a, const uint8_t* b, int N, int H, int W, double* out, void* ws, size_t ws_bytes,
                        hipStream_t stream);

/* ------------------------------------------------------------- scene cuts (python -m flair_amd scenes, --scene-cuts auto)
 * No counterpart in the reference, whose script restores one continuous clip: the per-block mean brightness that
 * flair_amd.scenes compares between neighbouring frames to find the cuts of a video.
 * frames: dense [N][H][W][3] uint8 RGB (what flair_amd.io.iter_frame_batches yields), at an address of any alignment.
 * out: [N][64] 64-bit integers; out[64 n + 8 a + b] = the sum of the integer luma Y = (77 R + 150 G + 29 B + 128) >> 8 over the
 * pixels (y, x) of frame n with (a H) / 8 <= y < ((a + 1) H) / 8 and (b W) / 8 <= x < ((b + 1) W) / 8 (integer divisions: an
 * 8 x 8 grid of blocks whose sizes differ by at most one row and one column).  Integer arithmetic only, so the sums are exact
 * and the same in every run, for every N and every position of a frame in the batch.  Every byte of the frames is read once:
 * one workgroup per (block, 32 rows) reads each row segment as an unaligned head, aligned 12-byte pieces and a tail, and adds
 * ONE 64-bit integer atomic to its entry; the entry zeroes `out` on `stream` first.  No allocation, no workspace, asynchronous
 * on `stream`.  H, W >= 8, W <= 2^24, N >= 1, out 8-byte aligned; offsets are 64-bit (N H W 3 may exceed 2^31). */
int flair_block_luma_sums(const uint8_t* frames, int N, int H, int W, long long* out, hipStream_t stream);

/* ------------------------------------------------------------- calibration launches (measurement only)
 * No counterpart in the reference: they exist so that bench.py can print, beside every roofline fraction against the data-sheet
 * peaks, what the device it ran on sustains with nothing in the way (profiles/r04_attainable_peaks.txt).
 * flair_probe_matrix_rate: workgroups_per_cu x CU-count workgroups of four waves, each wave `iters` x 16 independent
 *   v_mfma_f32_32x32x16_bf16 out of registers; *flop_out (host, optional) = FLOPs of the launch; sink: >= 4 bytes of device memory
 *   (never written).  flair_probe_stream_rate: mode 0 reads `bytes` from src, 1 writes `bytes` to dst, 2 copies src -> dst
 *   (16-byte accesses, grid-stride).  The caller times them with events on `stream`. */
int flair_probe_matrix_rate(int iters, int workgroups_per_cu, float* sink, double* flop_out, hipStream_t stream);
int flair_probe_stream_rate(const void* src, void* dst, size_t bytes, int mode, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAIR_HIP_H */
