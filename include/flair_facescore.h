/* libflair_hip.so -- the face-score part of the C ABI: the crop behind the `--score-faces largest|all` option of evaluate and
 * restore --ground-truth.  flair_abi_version() is 22 from this header on.
 *
 * Same library, same dialect and same conventions as flair_hip.h, flair_eval.h, flair_noref.h, flair_ident.h and
 * flair_temporal.h (plain device pointers and sizes, FLAIR_OK or a negative flair_status with a thread-local message for
 * flair_last_error(), asynchronous on `stream`, nothing allocated, every argument validated before anything is enqueued).  A
 * header of its own because the five others are closed sets; this one holds what a score of "how did the faces of unaligned
 * footage come out" needs and the others lack: a crop that goes from the WRITTEN BYTES of two frame sets to aligned byte crops,
 * which the byte-based entries flair_image_metrics, flair_lpips_prepare and flair_ident_prepare then read unchanged.
 * (flair_warp_affine_cubic works on the sampler's f32 [-1, 1] tensors and rounds in f32; a score describes the files.)
 *
 * The crop.  A bicubic (a = -0.75) affine crop with a constant border, all integers after two roundings.  For destination
 * pixel (x, y) of face k with the dst -> src matrix M = (M0 .. M5) = minv[k]:
 *   1. position, in 1/32 pixel:  X = (rint((M1 y + M2) 2^10) + 16 + rint(M0 x 2^10)) >> 5,  Y likewise from M3, M4, M5.
 *      The products and the one sum are float64 operations, each rounded on its own (the file is compiled without
 *      contraction); rint rounds half to even; >> is the floor shift.  The first of the four taps is (X >> 5) - 1, the row of
 *      the weight table X & 31; likewise in y.  (The position of flair_warp_affine_cubic, without its 16-bit saturation:
 *      that lies beyond +-32 000 source pixels, which the Python wrapper refuses.)
 *   2. weights: the 32 x 4 table of the a = -0.75 cubic at the fractions 0/32 .. 31/32 as INTEGERS num / 2^17; every entry
 *      of that table is a multiple of 2^-17 and every row sums to exactly 2^17.
 *   3. per channel c:  S = sum over the 4 x 4 taps of s num_x num_y  in 64-bit integers, s being the source byte of frame
 *      src_index[k] at the tap, or border[c] for a tap outside the frame.  |S| <= 255 (11/8)^2 2^34, far inside 64 bits.
 *   4. the byte is clamp((S + 2^33) >> 34, 0, 255), >> again the floor shift: floor(v + 1/2) of the exact value v = S / 2^34.
 * Both frame sets are cut with ONE geometry, computed once per pixel.  The arithmetic is exact, so the order of the sum is free
 * and a crop is the same bits in every run, for every K and every position in the batch.
 * This is the definition computed here.  It is deliberately NOT cv2.warpAffine's uint8 path, which multiplies by a 2^15
 * table of rounded weights and rounds twice; it is the exact value of the cubic that flair_warp_affine_cubic evaluates in
 * f32, rounded once.  There is no counterpart in the reference, which ships no scoring tool.
 */
#ifndef FLAIR_FACESCORE_H
#define FLAIR_FACESCORE_H

#include "flair_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K crops of Hd x Wd pixels out of one or two frame sets: out_a[k] (and out_b[k]) is the crop of frame src_index[k] of a (and
 * of b) under minv[k], steps 1 to 4 above.
 * a, b: dense [Nsrc][Hs][Ws][3] uint8 RGB at an address of ANY alignment (read byte by byte); b a second frame set of the
 * same shape, or NULL, and then out_b is NULL too.  minv: DEVICE [K][6] float64, dst -> src.  src_index: DEVICE [K] int32
 * with entries in [0, Nsrc), which the caller guarantees (the Python wrapper checks its host copy); a face whose index
 * lies outside is written as border and nothing outside the frames is ever read.  border: HOST [3] bytes, read before the
 * entry returns.  out_a, out_b: dense [K][Hd][Wd][3] uint8 at any alignment (byte stores).
 * One thread per destination pixel, lanes along x, the three channels and both sets per thread; a gather from L2 without LDS
 * or atomics.  K = 0 is a no-op: nothing is enqueued, and minv, src_index, out_a and out_b are not looked at.
 *   refuses : null a / border; b without out_b or out_b without b; Nsrc, Hs, Ws, Hd or Wd < 1; K < 0; and for K > 0: null
 *             minv / src_index / out_a; minv not 8-byte or src_index not 4-byte aligned; more than 2^31 - 1 workgroups
 *             (4 rows of 64 pixels each); out_a or out_b overlapping a or b.  Offsets are 64-bit. */
int flair_face_crop_u8(const uint8_t* a, const uint8_t* b, int Nsrc, int Hs, int Ws, const double* minv, const int* src_index, int K,
                       int Hd, int Wd, const uint8_t* border /* HOST [3] */, uint8_t* out_a, uint8_t* out_b, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FLAIR_FACESCORE_H */
