/* libflair_hip.so -- the video-stream part of the C ABI: the colour conversion and chroma resampling behind YUV4MPEG2 (.y4m)
 * input and output of every command.  flair_abi_version() is 23 from this header on.
 *
 * Same library, same dialect and same conventions as flair_hip.h, flair_eval.h, flair_noref.h, flair_ident.h, flair_temporal.h
 * and flair_facescore.h (plain device pointers and sizes, FLAIR_OK or a negative flair_status with a thread-local message for
 * flair_last_error(), asynchronous on `stream`, nothing allocated, every argument validated before anything is enqueued).  A
 * header of its own because the six others are closed sets; this one holds what reading and writing a video stream needs and
 * the others lack: the step between the BYTES OF A .y4m FRAME and the RGB bytes every other entry reads and writes.
 *
 * Formats.  All 8-bit; Wc = (W + 1) / 2 and Hc = (H + 1) / 2 where subsampled.
 *   tag (id)                      chroma plane          horizontal   vertical
 *   420jpeg (0; also bare 420)    Hc x Wc               centred      centred
 *   420mpeg2 (1)                  Hc x Wc               co-sited     centred
 *   422 (2)                       H x Wc                co-sited     full
 *   444 (3)                       H x W                 full         full
 *   mono (4)                      none (U = V = 128)    -            -
 * A frame's payload is Y | U | V, dense, W H + 2 wc hc bytes (wc x hc the chroma plane; W H for mono).
 *
 * Matrix and range.  bt601 (id 0; Kr, Kb = 0.299, 0.114) or bt709 (id 1; 0.2126, 0.0722); limited (id 0) or full (id 1).
 * Kg = 1 - Kr - Kb.  limited: sy = 255/219, sc = 255/224, y0 = 16; full: sy = sc = 1, y0 = 0.
 *   decode:  cy = sy, crv = 2 (1 - Kr) sc, cgu = 2 Kb (1 - Kb) / Kg sc, cgv = 2 Kr (1 - Kr) / Kg sc, cbu = 2 (1 - Kb) sc
 *   encode rows over (R, G, B):  ey = (Kr, Kg, Kb) / sy,  eu = (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)) / sc,
 *                                ev = (1 - Kr, -Kg, -Kb) / (2 (1 - Kr)) / sc
 * Every coefficient is round(x 65536) of the float64 value, computed once in Python; the kernels hold this table of INTEGERS
 * (no product comes nearer to a rounding tie than 0.003; tests/test_y4m_cpu.py derives the table again from Kr and Kb):
 *   coefficients bt601 limited : cy 76309 crv 104597 cgu 25675 cgv 53279 cbu 132201 ey 16829 33039 6416 eu -9714 -19071 28784 ev 28784 -24103 -4681
 *   coefficients bt601 full    : cy 65536 crv 91881 cgu 22553 cgv 46802 cbu 116130 ey 19595 38470 7471 eu -11058 -21710 32768 ev 32768 -27439 -5329
 *   coefficients bt709 limited : cy 76309 crv 117489 cgu 13975 cgv 34925 cbu 138438 ey 11966 40254 4064 eu -6596 -22189 28784 ev 28784 -26145 -2639
 *   coefficients bt709 full    : cy 65536 crv 103206 cgu 12276 cgv 30679 cbu 121609 ey 13933 46871 4732 eu -7509 -25259 32768 ev 32768 -29763 -3005
 *
 * Decode, YUV -> RGB at luma pixel (x, y).  Each axis gives two chroma taps with integer weights in quarters that sum to 4;
 * with c = i >> 1 on an axis of n chroma samples:
 *   full:      (i, 4)
 *   centred:   (c, 3) and, for even i, (max(c - 1, 0), 1); for odd i, (min(c + 1, n - 1), 1)
 *   co-sited:  for even i, (c, 4); for odd i, (c, 2) and (min(c + 1, n - 1), 2)
 * U16 = sum of wy wx U[cy][cx], in sixteenths; V16 likewise (mono: 2048 both).  Then
 *   yy = cy 16 (Y - y0),  u = U16 - 2048,  v = V16 - 2048
 *   R = clamp((yy + crv v + 2^19) >> 20, 0, 255)
 *   G = clamp((yy - cgu u - cgv v + 2^19) >> 20, 0, 255)
 *   B = clamp((yy + cbu u + 2^19) >> 20, 0, 255)
 * >> is the floor shift.  Every magnitude stays below 6 10^8, so int32 is exact, and each value is rounded ONCE.
 *
 * Encode, RGB -> YUV.
 *   Y = clamp(((ey . (R, G, B) + 2^15) >> 16) + y0, lo, hiY)
 *   per luma pixel the UNROUNDED cu = eu . (R, G, B) and cv = ev . (R, G, B), at scale 2^16
 *   a chroma sample is the integer-weighted sum S of cu over its footprint, tap indices clamped to the frame (odd sizes
 *   replicate the edge):  centred axis: luma 2c and 2c + 1, weights 1, 1;  co-sited axis: luma 2c - 1, 2c and 2c + 1,
 *   weights 1, 2, 1;  full axis: weight 1.  The total weight is 2^k: k = 0 for 444, 2 for 422, 2 for 420jpeg, 3 for 420mpeg2.
 *   U = clamp(((S + 2^(15 + k)) >> (16 + k)) + 128, lo, hiC);  V likewise from cv
 *   (lo, hiY, hiC) = (16, 235, 240) for limited and (0, 255, 255) for full.  mono writes Y only.
 * All integers, so the order of a sum is free and a file is the same bits in every run.
 * This is the definition computed here.  It is deliberately NOT swscale's path, which uses other tables, rounds twice and
 * uses other chroma filters.  There is no counterpart in the reference, which reads and writes frame files only.
 */
#ifndef FLAIR_YUV_H
#define FLAIR_YUV_H

#include "flair_hip.h"

#define FLAIR_YUV_420JPEG 0
#define FLAIR_YUV_420MPEG2 1
#define FLAIR_YUV_422 2
#define FLAIR_YUV_444 3
#define FLAIR_YUV_MONO 4
#define FLAIR_YUV_BT601 0
#define FLAIR_YUV_BT709 1
#define FLAIR_YUV_LIMITED 0
#define FLAIR_YUV_FULL 1

#ifdef __cplusplus
extern "C" {
#endif

/* N frames of a stream -> RGB bytes, the decode above.
 * payload: dense [N][P] uint8, P = W H + 2 wc hc (W H for mono), exactly the file's bytes, at an address of ANY alignment
 * (payload sizes are odd in general).  out: dense uint8 at any alignment, [N][H][W][3] for planar = 0 and [N][3][H][W] for
 * planar = 1.
 * One thread per 4 x 2 luma pixels, lanes along x, a workgroup owns 16 rows of 128 pixels of one frame: the two luma rows
 * that share a chroma row sit in one thread, and neighbouring threads' chroma taps meet in the cache, so every byte comes
 * from HBM once.  Four bytes move as one word where the address allows and byte by byte where not.  No LDS, no atomics.
 * N = 0 is a no-op: nothing is enqueued, and payload and out are not looked at.
 *   refuses : H or W < 1; N < 0; format, matrix or range not one of the ids above; planar not 0 or 1; and for N > 0: null
 *             payload / out; more than 2^31 - 1 workgroups; out overlapping payload.  Offsets are 64-bit. */
int flair_yuv_to_rgb_u8(const uint8_t* payload, int N, int H, int W, int format, int matrix, int range, int planar, uint8_t* out,
                        hipStream_t stream);

/* N frames of RGB bytes -> the payloads of a stream, the encode above.
 * rgb: dense [N][H][W][3] uint8 at any alignment.  payload_out: dense [N][P] uint8 at any alignment, P as above.
 * The same threads and workgroups as flair_yuv_to_rgb_u8; a thread reads its 4 x 2 pixels and, for the co-sited formats, the
 * pixel to their left.  N = 0 is a no-op.
 *   refuses : H or W < 1; N < 0; format, matrix or range not one of the ids above; and for N > 0: null rgb / payload_out; more
 *             than 2^31 - 1 workgroups; payload_out overlapping rgb.  Offsets are 64-bit. */
int flair_rgb_to_yuv_u8(const uint8_t* rgb, int N, int H, int W, int format, int matrix, int range, uint8_t* payload_out,
                        hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FLAIR_YUV_H */
