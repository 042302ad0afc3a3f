/* libflair_hip.so -- the tiling part of the C ABI: cutting whole frames into overlapping tiles of one size and blending the
 * tiles' results back into whole frames with feathered weights (flair_amd/tiling.py: restore --tile).  flair_abi_version() is 24
 * from this header on.
 *
 * Same library, same dialect and same conventions as flair_hip.h, flair_eval.h, flair_noref.h, flair_ident.h, flair_temporal.h,
 * flair_facescore.h and flair_yuv.h (plain device pointers and sizes, FLAIR_OK or a negative flair_status with a thread-local
 * message for flair_last_error(), asynchronous on `stream`, nothing allocated, every argument validated before anything is
 * enqueued).  A header of its own because the seven others are closed sets.
 *
 * The plan.  A plan is a tensor product: `rows` tile rows with origins oy[0 .. rows) and `cols` tile columns with origins
 * ox[0 .. cols), every tile th x tw pixels; tile k = r cols + c (row-major, "plan order") starts at pixel (oy[r], ox[c]) of an
 * H x W frame.  The origins are int32 arrays IN DEVICE MEMORY (they are the same for every step of a video, so they are uploaded
 * once); the host side (flair_amd/tiling.py, flair_amd/ops.py) checks them before it uploads them, and the kernels do not trust
 * them either: a tile whose origin is negative or reaches beyond the frame is read as zeros by the gather and skipped by the blend,
 * so that no index ever leaves a buffer.  Any number of tiles may cover a pixel (three per axis happen with short frames).
 *
 * Tiles are dense [rows cols N][C][th][tw] f32: the tile index is major, so the tiles of a clip of N frames are rows cols clips of N
 * frames, one after the other.
 *
 * The weights.  Along one axis, for a tile with origin o and side t in a frame of length L, and a pixel p with o <= p < o + t:
 *   dl = p - o + 0.5                dr = o + t - p - 0.5
 *   wl = 1 if o == 0,     else min(1, dl / ramp)
 *   wr = 1 if o + t == L, else min(1, dr / ramp)
 *   w  = min(wl, wr)
 * A tile's weight at a pixel is wy wx, and
 *   out = sum_k w^_k v_k,   w^_k = w_k / sum_j w_j     over the tiles k that cover the pixel, in plan order.
 * Because the plan is a product, sum_j w_j = (sum of wy over the covering rows) (sum of wx over the covering columns), and the
 * kernel normalises per axis: w^_k = (wy / sum wy) (wx / sum wx).  The weights are evaluated in float64 and w^_k is rounded to f32
 * ONCE; the sum is f32, acc = w^_0 v_0, then acc = fma(w^_k, v_k, acc) for k = 1, 2, ... in plan order: one fixed association,
 * the same bits in every run, and at most k + 1 roundings for k covering tiles (|error| <= (k + 1) 2^-24 sum w^ |v| to first
 * order).  A pixel covered by one tile has w^ = w / w = 1 and gets that tile's value bit for bit.  A pixel no tile covers (a plan
 * the host side refuses) is written as 0.
 */
#ifndef FLAIR_TILE_H
#define FLAIR_TILE_H

#include "flair_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frames -> tiles, a plain copy: tiles[(k N + n)][c][y][x] = frame[n][c][oy[r] + y][ox[cc] + x] for k = r cols + cc.
 * frame: dense [N][C][H][W] f32 at any 4-byte alignment (a view into a larger buffer will do); tiles: dense
 * [rows cols N][C][th][tw] f32 at any 4-byte alignment; oy: rows int32 and ox: cols int32 in device memory.
 * One launch for all tiles.  One thread per 4 consecutive pixels of a tile row, lanes along x: 16-byte loads and stores where both
 * addresses allow, element by element where not (odd W or tw, origins that are no multiple of 4, a misaligned base).  64-bit
 * offsets, no LDS, no atomics.
 *   refuses : null frame / tiles / oy / ox; N, C, rows, cols < 1; th, tw < 1; th > H or tw > W; more than 2^31 - 1 workgroups;
 *             tiles overlapping frame. */
int flair_tile_gather_f32(const float* frame, int N, int C, int H, int W, const int* oy, int rows, const int* ox, int cols, int th,
                          int tw, float* tiles, hipStream_t stream);

/* Tiles -> frames, the weighted sum above with ramp = `ramp` pixels on both axes.
 * tiles: dense [rows cols N][C][th][tw] f32; out: dense [N][C][H][W] f32; both at any 4-byte alignment; oy, ox as above.
 * Output-centric: one thread owns 4 consecutive pixels of one row of one frame, for all C channels (the weights do not depend on
 * the channel), finds the covering tile rows and columns from the origin arrays and evaluates the definition; 16-byte loads of a
 * tile row where the four pixels lie inside the tile and the address allows, 16-byte stores where the output address allows,
 * element by element where not.  64-bit offsets, no LDS, no atomics.
 *   refuses : null tiles / out / oy / ox; N, C, rows, cols < 1; th, tw < 1; th > H or tw > W; ramp < 1; more than 2^31 - 1
 *             workgroups; out overlapping tiles. */
int flair_tile_blend_f32(const float* tiles, int N, int C, int H, int W, const int* oy, int rows, const int* ox, int cols, int th,
                         int tw, int ramp, float* out, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FLAIR_TILE_H */
