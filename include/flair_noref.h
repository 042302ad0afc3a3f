/* libflair_hip.so -- the no-reference part of the C ABI: the kernels behind `python -m flair_amd niqe` and the `--niqe FILE`
 * option of evaluate / restore / interpolate.  flair_abi_version() is 19 from this header on.
 *
 * Same library, same dialect and same conventions as flair_hip.h and flair_eval.h (plain device pointers and sizes, FLAIR_OK
 * or a negative flair_status with a thread-local message for flair_last_error(), asynchronous on `stream`, nothing allocated,
 * every argument validated before anything is enqueued).  A header of its own because the two others are closed sets: the
 * sampling path's drop-in boundary and the full-reference scores.  This one holds scores that need no ground truth.
 *
 * NIQE (Mittal, Soundararajan, Bovik 2013) of ONE RGB byte frame of H x W, as BasicSR's calculate_niqe computes it on the Y
 * channel without border crop, with the two differences marked (D1), (D2).  nh = H / 96, nw = W / 96 (floored); a score needs
 * nh nw >= 2.
 *   1. Luma, exact integers: Y = round_half_even((65481 R + 128553 G + 24966 B) / 255000) + 16, in 16 .. 235 (BT.601 "y_only",
 *      then .round()).  (D1) BasicSR reaches this through float32 /255 ... *255 round trips and lands one grey level away on
 *      about 2e-5 of all byte triples, those within its rounding error of a tie; here the value is the exact-arithmetic one.
 *      Crop to the top-left 96 nh x 96 nw.
 *   2. Two scales: scale 1 is the cropped luma; scale 2 is MATLAB imresize(., 0.5) (bicubic, antialiased) of it, which for a
 *      factor of exactly 1/2 on even sizes is the separable 8-tap filter [-3, -9, 29, 111, 111, 29, -9, -3] / 256 on inputs
 *      2i-3 .. 2i+4, indices reflected symmetrically (-1 -> 0, -2 -> 1, n -> n-1).  65536 Y2 is an exact integer below 2^25.
 *   3. MSCN map per scale, window g of 7 x 7 (fspecial('gaussian', 7, 7/6), from the parameter file): mu = g * Y as a 2-D
 *      convolution with replicate borders of the cropped plane, sigma = sqrt(|g * Y^2 - mu^2|), M = (Y - mu) / (sigma + 1).
 *      (D2) evaluated in the shifted form d = Y_tap - Y_centre, mu - Y_centre = sum g d, sigma^2 = sum g d^2 - (sum g d)^2 in
 *      float64: a constant neighbourhood gives M = 0 exactly, where the unshifted sums leave +-1e-14 of rounding noise
 *      to which a distribution is then fitted.
 *   4. Per block (96 x 96 at scale 1, 48 x 48 at scale 2), block index j nh + i (column-major), five maps: M itself and
 *      M roll(M, s) for s = (0,1), (1,0), (1,1), (1,-1), numpy's roll wrapping INSIDE the block; per map five moments:
 *      c- = #{x < 0}, c+ = #{x > 0}, s- = sum of x^2 over x < 0, s+ = the same over x > 0, a = sum |x|.  Zeros count in
 *      neither c- nor c+.
 *   5. and 6. The AGGD fit of every map, the 36 features per block and the distance to the pristine model are float64 work on
 *      the host (flair_amd/niqe.py): 50 numbers per block leave the device.
 * There is no counterpart in the reference, which ships no scoring tool.
 */
#ifndef FLAIR_NOREF_H
#define FLAIR_NOREF_H

#include "flair_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLAIR_NIQE_BLOCK 96 /* block side at scale 1; half of it at scale 2 */

/* Steps 1 and 2 in one launch.  u8: dense [N][H][W][3] uint8 RGB (what flair_amd.io.iter_frame_batches yields) at an address
 * of ANY alignment (read byte by byte); nothing outside the 3 N H W bytes is read, and nothing right of or below the crop.
 * y1: [N][96 nh][96 nw] int32, the cropped luma; y2: [N][48 nh][48 nw] int32 = 65536 x the half-scale plane.
 * Integer arithmetic only: both planes are bit-exact.  One workgroup owns a 32 x 32 tile of y1: its 38 x 38 haloed luma sits
 * in LDS (reflected at the crop's border), the rows are filtered into a 38 x 16 strip, and thread (i, j) writes y2.
 *   refuses : null u8 / y1 / y2; N < 1; H or W < 96 (no block); y1 or y2 not 4-byte aligned; more than 2^31 - 1 workgroups.
 *             Offsets are 64-bit. */
int flair_niqe_luma(const uint8_t* u8, int N, int H, int W, int* y1, int* y2, hipStream_t stream);

/* Steps 3 and 4 of ONE scale.  y: dense [N][Hc][Wc] int32, a pixel's value is y * inv_scale with inv_scale = 1 (y1) or
 * 2^-16 (y2), so that differences of two pixels are exact doubles; block = 96 or 48 divides Hc and Wc.  window: 49 doubles in
 * row-major order, a DEVICE pointer; tap (dy, dx) of the convolution weighs window[3 - dy][3 - dx].
 * out: [N][(Hc / block) (Wc / block)][5 maps][5 moments] doubles in the order of step 4 (c-, c+, s-, s+, a; the counts are
 * exact doubles).  mscn: null, or [N][Hc][Wc] doubles that receive M (for per-element tests; null in production).
 * One workgroup per (frame, block), of 1024 threads at 96 and 256 at 48 (nine pixels per thread): the haloed int32 tile
 * ((block + 6)^2) and the float64 MSCN tile (block^2) sit in LDS, 118 544 bytes at 96; the window's index is uniform, so its 49
 * doubles come through the scalar cache.  A thread accumulates the 25 numbers over its pixels tid, tid + threads, ... in that
 * order, a wave adds its 64 lanes in a shuffle tree and thread q < 25 adds the waves' sums in wave order.  No floating-point
 * atomics: a block's 25 numbers are the same bits in every run, for every N and every position in the batch.  Float64
 * throughout, evaluated product by product (no contraction).
 *   refuses : null y / window / out; N, Hc or Wc < 1; a block other than 96 or 48; Hc or Wc not a multiple of block; an
 *             inv_scale other than 1 or 2^-16; y not 4-byte aligned; window, out or mscn not 8-byte aligned; more than
 *             2^31 - 1 workgroups.  Offsets are 64-bit. */
int flair_niqe_moments(const int* y, int N, int Hc, int Wc, int block, double inv_scale, const double* window, double* out,
                       double* mscn, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FLAIR_NOREF_H */
