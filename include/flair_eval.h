/* libflair_hip.so -- the evaluation-only part of the C ABI: the kernels behind `python -m flair_amd evaluate --lpips`.
 *
 * Same library, same dialect and same conventions as flair_hip.h (plain device pointers and sizes, FLAIR_OK or a negative
 * flair_status with a thread-local message for flair_last_error(), asynchronous on `stream`, nothing allocated, every
 * argument validated before anything is enqueued).  The entries live in a header of their own because nothing of the
 * sampling hot path calls them: flair_hip.h stays the drop-in boundary of the reference's operators, this one is ours.
 *
 * LPIPS (Zhang et al. 2018, the `lpips` package 0.1 with spatial=False in eval mode) of two RGB byte frames a, b:
 *   1. x = 2 byte / 255 - 1;
 *   2. x_c <- (x_c - shift_c) / scale_c, shift = (-.030, -.088, -.188), scale = (.458, .448, .450); the zero padding of the
 *      trunk's first convolution applies AFTER this step, so it is not folded into that layer's bias;
 *   3. five taps of a frozen VGG-16 or AlexNet trunk (flair_conv_nhwc with FLAIR_ACT_RELU, the pools below, AlexNet's stem below);
 *   4. per tap and pixel a^ = a / (sqrt(sum_c a_c^2) + 1e-10), the same for b^, d = sum_c w_c (a^_c - b^_c)^2 with the C weights
 *      of the tap's bias-free 1x1 `lin` layer; an all-zero feature vector normalises to zeros;
 *   5. LPIPS = the sum over the taps of the mean of d over the tap's pixels.
 * There is no counterpart in the reference, which ships no scoring tool.
 */
#ifndef FLAIR_EVAL_H
#define FLAIR_EVAL_H

#include "flair_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Steps 1 and 2 for BOTH frame sets in one launch, so that a batch goes through the trunk as 2 N frames.
 * a, b: dense [N][H][W][3] uint8 RGB (what flair_amd.io.iter_frame_batches yields), each at an address of ANY alignment: a
 * set is read as a head of at most three pixels byte by byte, then aligned 12-byte pieces of four pixels (two dword loads
 * per pixel, never a misaligned one), then a tail byte by byte; nothing outside the 3 N H W bytes is read.
 * y: f32 clip tensor [2 N][H][W] pixels, y_ld floats apart: frames 0 .. N-1 are a's, N .. 2N-1 are b's.  Channels 0 .. 2
 * of a pixel = ((2 byte / 255 - 1) - shift_c) / scale_c, evaluated as ONE double-precision fma A_c byte + B_c with
 * A_c = 2 / (255 scale_c), B_c = -(1 + shift_c) / scale_c and rounded to f32 once: within 1 ulp (f32) of the steps above in
 * exact arithmetic for every byte.  Channels 3 .. 15 = 0: the first convolution reads input segments in multiples of 16
 * channels.  Channels 16 .. y_ld-1 are never written.  Four lanes write one pixel's 64 bytes, so a wave stores 1 KiB
 * contiguously when y_ld = 16.
 *   refuses : null a / b / y; N, H or W < 1; y_ld < 16 or not a multiple of 4 floats; y not 16-byte aligned; more than
 *             2^31 - 1 workgroups.  Offsets are 64-bit (2 N H W y_ld may exceed 2^31). */
int flair_lpips_prepare(const uint8_t* a, const uint8_t* b, int N, int H, int W, float* y, int y_ld, hipStream_t stream);

/* Step 4 and the spatial mean of ONE tap: acc[f] += (1 / HW) sum_p d_p(fa[f], fb[f]), f = 0 .. F-1, so that five calls
 * accumulate a frame's LPIPS in acc (the caller zeroes it before the first).
 * fa, fb: f32 [F][HW] pixels of C channels, pixel strides fa_ld / fb_ld >= C (channel slices and the two halves of one
 * 2F-frame tensor are views); C in {64, 128, 192, 256, 384, 512}; w: [C] f32, the tap's lin weights; acc: [F] doubles.
 * Each feature value is read ONCE, in 16-byte loads: C / 4 float4 of a pixel sit in 16, 32 or 64 lanes (one, two or three
 * float4 per lane: 512 channels are 8 floats per lane of a whole wave) and stay in registers across the two passes, the
 * sums of squares (lane-serial fma, then an xor butterfly, so every lane holds the same sum) and the weighted squared
 * difference of the quotients (true f32 divisions, as the definition reads).  A lane adds its part of d to a DOUBLE
 * accumulator; a frame is cut into FLAIR_LPIPS_TAP_PARTS contiguous runs of ceil(HW / PARTS) pixels, one workgroup each,
 * which writes one partial into ws; a second launch sums a frame's partials in a fixed order, divides by HW and adds to
 * acc[f].  No floating-point atomics: a frame's value is the same bits in every run, for every F and every position in the
 * batch.  ws: F * FLAIR_LPIPS_TAP_PARTS * 8 bytes (the closed form: there is no size query), 8-byte aligned, contents irrelevant.
 *   refuses : null fa / fb / w / acc / ws; F < 1; HW < 1; a C outside the list; fa_ld / fb_ld below C or not multiples of 4
 *             floats; fa, fb or w not 16-byte aligned; acc or ws not 8-byte aligned; ws_bytes below the closed form;
 *             F * PARTS > 2^31 - 1.  Offsets are 64-bit. */
#define FLAIR_LPIPS_TAP_PARTS 1024
int flair_lpips_tap(const float* fa, int fa_ld, const float* fb, int fb_ld, int F, long HW, int C, const float* w, double* acc,
                    void* ws, size_t ws_bytes, hipStream_t stream);

/* nn.MaxPool2d(k, stride 2) WITHOUT padding in floor mode, k = 2 or 3, on an f32 clip tensor:
 * [F][H][W][C] -> [F][(H - k) / 2 + 1][(W - k) / 2 + 1][C]; every window lies inside the frame, so an odd last row or column
 * is dropped.  k = 3 is AlexNet's pool (flair_maxpool3x3s2_nhwc pads by 1), k = 2 VGG's on odd frames
 * (flair_maxpool2x2s2_nhwc is ceil_mode=True and agrees with it on even ones only).  Bit-exact: max of the window.
 *   refuses : null x / y; F < 1; k not 2 or 3; H or W < k; C not a positive multiple of 4; x_ld / y_ld below C or not
 *             multiples of 4 floats; x or y not 16-byte aligned; more than 2^31 - 1 workgroups. */
int flair_maxpool_valid_s2_nhwc(const float* x, int x_ld, int F, int H, int W, int C, int k, float* y, int y_ld,
                                hipStream_t stream);

/* AlexNet's stem, torchvision `features.0` + ReLU: Conv2d(3, 64, kernel 11, stride 4, padding 2) on the prepared frames.
 * x: f32 [F][H][W] pixels, x_ld >= 3 floats apart, channels 0 .. 2 read (flair_lpips_prepare's output); w: [363][64] f32,
 * row (ky * 11 + kx) * 3 + c, column = output channel; bias: [64] f32; y: [F][Ho][Wo] pixels of 64 channels, y_ld apart,
 * Ho = (H + 4 - 11) / 4 + 1, Wo likewise; zeros outside the frame.  A direct kernel: one workgroup stages the 39 x 39 x 3
 * input patch of an 8 x 8 output tile in LDS; a lane owns one output pixel and a wave 16 output channels, whose weights
 * are wave-uniform.  f32 fma in tap order (ky, kx, c), bias first.
 *   refuses : null x / w / bias / y; F < 1; H or W < 7; x_ld < 3; y_ld < 64 or not a multiple of 4 floats; w, bias or y not
 *             16-byte aligned; more than 2^31 - 1 workgroups. */
int flair_alexnet_stem(const float* x, int x_ld, int F, int H, int W, const float* w, const float* bias, float* y, int y_ld,
                       hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FLAIR_EVAL_H */
