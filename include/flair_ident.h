/* libflair_hip.so -- the identity part of the C ABI: the kernels behind the `--identity FILE` option of evaluate / restore /
 * interpolate.  flair_abi_version() is 20 from this header on.
 *
 * Same library, same dialect and same conventions as flair_hip.h, flair_eval.h and flair_noref.h (plain device pointers and
 * sizes, FLAIR_OK or a negative flair_status with a thread-local message for flair_last_error(), asynchronous on `stream`,
 * nothing allocated, every argument validated before anything is enqueued).  A header of its own because the three others are
 * closed sets; this one holds what a score of "is it still the same person" needs and the others lack.
 *
 * ArcFace identity similarity ("IDS" of CodeFormer, "Deg." of RestoreFormer, "IDD" of VQFR in its cosine form) of two aligned
 * face crops a, b of H x W RGB bytes, with the ResNet-18 IR network of GFPGAN / VQFR (arcface_resnet18.pth):
 *   1. x = 2 byte / 255 - 1 per channel; gray = 0.2989 R + 0.5870 G + 0.1140 B (GFPGAN's gray_resize_for_identity);
 *   2. bilinear resize to 128 x 128 as F.interpolate(size=128, mode='bilinear', align_corners=False) does it, without
 *      antialias, up or down: for an output index d along an axis of `in` pixels, src = (d + 0.5) (in / 128) - 0.5 clamped
 *      below at 0, i0 = floor(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1; the pixel is
 *      l0h (l0w p00 + l1w p01) + l1h (l0w p10 + l1w p11);
 *   3. the network (flair_conv_nhwc in f32 with the BatchNorms after a convolution folded in, flair_affine_channels_f32 for the
 *      BatchNorm in front of one, flair_prelu_nhwc, flair_maxpool2x2s2_nhwc) up to the 8 x 8 x 512 output of layer4;
 *   4. e = bn5(fc5(flatten(bn4(.)))), 512 numbers: one matrix-vector product per frame once both BatchNorms are folded
 *      into the matrix (flair_ident_embed);
 *   5. ids = <e_a, e_b> / (|e_a| |e_b|) in float64 on the host (flair_amd/identity.py).
 * The scripts of GFPGAN / VQFR make the grey image and the 128 x 128 size with cv2 on bytes (cv2.cvtColor's fixed-point
 * luma, cv2.resize); those are not reproduced.  There is no counterpart in the reference, which ships no scoring tool.
 */
#ifndef FLAIR_IDENT_H
#define FLAIR_IDENT_H

#include "flair_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLAIR_IDENT_SIDE 128          /* the network's input is 1 x 128 x 128 */
#define FLAIR_IDENT_EMBED_KCHUNK 1024 /* inputs per workgroup of flair_ident_embed; its workspace in closed form below */

/* Steps 1 and 2 for one or two frame sets in one launch, so that a batch goes through the network as F frames.
 * a, b: dense [N][H][W][3] uint8 RGB (what flair_amd.io.iter_frame_batches yields), each at an address of ANY alignment (read
 * byte by byte); nothing outside the 3 N H W bytes is read.  b may be NULL: then F = N, else F = 2 N with a's frames first.
 * y: f32 clip tensor [F][128][128] pixels, y_ld floats apart.  Channel 0 of a pixel = the value of step 2, evaluated in double
 * precision throughout and rounded to f32 once (|value| <= 0.9999, so within 2^-24 of exact arithmetic).  Channels 1 .. 15
 * = 0: the first convolution reads input segments in multiples of 16 channels.  Channels 16 .. y_ld-1 are never written.
 * Four lanes write one pixel's 64 bytes.
 *   refuses : null a / y; N, H or W < 1; y_ld < 16 or not a multiple of 4 floats; y not 16-byte aligned; more than
 *             2^31 - 1 workgroups.  Offsets are 64-bit. */
int flair_ident_prepare(const uint8_t* a, const uint8_t* b, int N, int H, int W, float* y, int y_ld, hipStream_t stream);

/* Step 4: out[f][o] = bias[o] + sum_k w[o][k] x[f][k], f = 0 .. F-1, o = 0 .. O-1.
 * x: [F] rows of K floats, x_ld floats apart (the layer4 output as it lies: K = 8 * 8 * 512 = 32768 for the real network);
 * w: dense [O][K] f32 (67 MB there); bias: [O] f32; out: [F] rows of O floats, out_ld floats apart.
 * A workgroup owns 16 output rows and FLAIR_IDENT_EMBED_KCHUNK consecutive inputs (a quarter per wave) for up to 16 frames at
 * a time, so w is streamed from memory once per launch for every 16 frames, in 16-byte loads of whole 128-byte lines.  A
 * product of two f32 is exact in float64, and every sum is float64: a wave accumulates its 16 x 16 tile with
 * v_mfma_f64_16x16x4_f64 over its inputs in ascending order, the workgroup adds its four waves' tiles in wave order and writes
 * one partial per (chunk, f, o) into ws; a second launch adds bias and the chunks' partials in ascending order and rounds to
 * f32 once.  No floating-point atomics: the chunking depends on K alone, so a frame's embedding is the same bits in every
 * run, for every F and every position in the batch.
 * ws: ceil(K / FLAIR_IDENT_EMBED_KCHUNK) * F * O * 8 bytes (the closed form: there is no size query), 8-byte aligned,
 * contents irrelevant.
 *   refuses : null x / w / bias / out / ws; F, K or O < 1; K not a multiple of 4 or above 2^30; x_ld below K or not a multiple
 *             of 4 floats; x or w not 16-byte aligned; out_ld below O; ws not 8-byte aligned; ws_bytes below the closed form;
 *             more than 2^31 - 1 workgroups or more than 65535 * 16 frames.  Offsets are 64-bit. */
int flair_ident_embed(const float* x, int x_ld, int F, int K, const float* w, const float* bias, int O, float* out, int out_ld,
                      void* ws, size_t ws_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FLAIR_IDENT_H */
