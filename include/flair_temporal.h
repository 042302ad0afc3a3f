/* libflair_hip.so -- the temporal part of the C ABI: the kernels behind the `--warp-error FILE` option of evaluate / restore /
 * interpolate and behind the `warp-error` command.  flair_abi_version() is 21 from this header on.
 *
 * Same library, same dialect and same conventions as flair_hip.h, flair_eval.h, flair_noref.h and flair_ident.h (plain device
 * pointers and sizes, FLAIR_OK or a negative flair_status with a thread-local message for flair_last_error(), asynchronous on
 * `stream`, nothing allocated, every argument validated before anything is enqueued).  A header of its own because the four
 * others are closed sets; this one holds what a score of "does the video hold together over time" needs and the others lack.
 *
 * The flow-warping error (E_warp of Lai et al., "Learning Blind Video Temporal Consistency", ECCV 2018, with the occlusion
 * and motion-boundary rule of Ruder et al. 2016) of two consecutive frames a (frame t) and b (frame t + 1), H x W RGB bytes,
 * under two dense f32 flows [H][W][2] of (dx, dy) in pixels: f, the flow a -> b, so that a(p) ~ b(p + f(p)), and g, the flow
 * b -> a.  All arithmetic is float64 on the f32 and byte inputs; every product and every sum is rounded on its own (the file
 * is compiled without contraction), in the order written here, sums from left to right:
 *   1. q = p + f(p).  The pixel is OUTSIDE unless 0 <= q.x <= W - 1 and 0 <= q.y <= H - 1 (a flow that is not a number is
 *      outside by this wording);
 *   2. g~ = bilinear(g, q) and b~_c = bilinear(b_c, q): x0 = floor(q.x), x1 = min(x0 + 1, W - 1), l1x = q.x - x0,
 *      l0x = 1 - l1x, likewise in y; the value is l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), v(row)(column);
 *   3. OCCLUDED if |f + g~|^2 > 0.01 (|f|^2 + |g~|^2) + 0.5, each |v|^2 = v.x v.x + v.y v.y;
 *   4. MOTION BOUNDARY if (|dx f|^2 + |dy f|^2) > 0.01 |f|^2 + 0.002, with forward differences dx f(x, y) = f(x + 1, y) -
 *      f(x, y), 0 in the last column, dy f(x, y) = f(x, y + 1) - f(x, y), 0 in the last row;
 *   5. M(p) = 1 unless the pixel is outside, occluded or on a motion boundary (an outside pixel is neither gathered nor tested);
 *   6. e(p) = (a_0 - b~_0)^2 + (a_1 - b~_1)^2 + (a_2 - b~_2)^2 in byte units;
 *   7. S = sum_p M e, N = sum_p M;
 *   8. warp_err = S / (255^2 N), undefined for N = 0 (the host's division: flair_amd/temporal.py).
 * This is the definition computed here.  It is NOT a reproduction of Lai et al.'s script, which took its flows from FlowNet2
 * and its occlusion mask from code of its own; here the flows are SPyNet's (flair_conv_nhwc in f32).  There is no counterpart
 * in the reference, which ships no scoring tool.
 */
#ifndef FLAIR_TEMPORAL_H
#define FLAIR_TEMPORAL_H

#include "flair_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLAIR_WARP_TILE_H 32 /* a workgroup of flair_warp_error owns a tile of 32 rows ... */
#define FLAIR_WARP_TILE_W 64 /* ... by 64 columns, the tile of flair_image_metrics; its workspace in closed form below */

/* Steps 1 to 5 for P frame pairs: mask[i][y][x] = M of pair i.
 * f, g: dense [P][H][W][2] f32, read as 8-byte pairs; mask: dense [P][H][W] uint8, every byte written with 0 or 1 (ordinary
 * byte stores).  One thread per pixel; the four gathered corners of g are the traffic that is not streamed.
 *   refuses : null f / g / mask; P, H or W < 1; f or g not 8-byte aligned; more than 2^31 - 1 workgroups (256 pixels each).
 *             Offsets are 64-bit. */
int flair_flow_occlusion(const float* f, const float* g, int P, int H, int W, uint8_t* mask, hipStream_t stream);

/* Steps 6 and 7 for P frame pairs of one or two frame sets judged by the SAME flow and mask: out[s][i] = (S, N) of frames i
 * and i + 1 of set s.
 * a: dense [P + 1][H][W][3] uint8 RGB at an address of ANY alignment (read byte by byte); a2: a second frame set of the same
 * shape, or NULL; sets = 1 without it and 2 with it (a is set 0).  f: dense [P][H][W][2] f32 (the flow frame i -> frame i + 1);
 * mask: dense [P][H][W] uint8, non-zero = counted.  A pixel whose mask is non-zero but whose q is outside (a mask that
 * flair_flow_occlusion did not make from this f) is left out like a masked one: nothing outside the frames is ever read.
 * out: [sets][P][2] float64.
 * A workgroup owns one FLAIR_WARP_TILE_H x FLAIR_WARP_TILE_W tile of one pair for both sets: lane = column, a wave owns 8
 * rows.  A lane adds its rows in ascending order, a wave adds its lanes in a fixed tree, the workgroup adds its four waves in
 * wave order, all in float64 (N in integers), and writes one (S, N) partial per (set, pair, tile) into ws; a second launch
 * adds a pair's tiles in ascending order.  No floating-point atomics: the partition depends on H and W alone, so a pair's
 * (S, N) is the same bits in every run, for every P and every position in the batch.
 * ws: sets * P * ceil(H / FLAIR_WARP_TILE_H) * ceil(W / FLAIR_WARP_TILE_W) * 16 bytes (the closed form: there is no size
 * query), 8-byte aligned, contents irrelevant.
 *   refuses : null a / f / mask / out / ws; P, H or W < 1; f, out or ws not 8-byte aligned; ws_bytes below the closed form;
 *             more than 2^31 - 1 workgroups.  Offsets are 64-bit. */
int flair_warp_error(const uint8_t* a, const uint8_t* a2, const float* f, const uint8_t* mask, int P, int H, int W, double* out,
                     void* ws, size_t ws_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FLAIR_TEMPORAL_H */
