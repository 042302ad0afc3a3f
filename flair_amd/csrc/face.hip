// Device-side face crop / inverse paste of the un-aligned auxiliary-prior branch
// (guided_diffusion/gaussian_diffusion.py:476-493, every denoising step with t in [tau, start]):
//   facelib/utils/face_restoration_helper.py:225-254  get_crop_face_from_affine_matrices
//       cv2.warpAffine(img, M, (512, 512), INTER_CUBIC, BORDER_CONSTANT, (135, 133, 132)) on float32 frames
//   facelib/utils/face_restoration_helper.py:264-335  inverse_faces
//       parsing arg-max -> MASK_COLORMAP -> 2 x cv2.GaussianBlur(mask, (101, 101), 26) on a float64 mask
//       -> 10-pixel border zeroed, / 255 -> cv2.warpAffine(face | mask, inverse_affine, INTER_CUBIC)
//   gaussian_diffusion.py:491  x_with_face = x0 * (1 - inv_mask) + inv_face * inv_mask
// flair_warp_affine_cubic_indexed crops several faces out of one frame (:225-254 with a frame index per matrix);
// flair_face_paste runs the two warps of :264-335 and the blend of :491 per output pixel for every face of the frame, in list
// order -- a composition of the reference's per-face operations (the reference itself pastes one face per frame).
// The reference round-trips every frame through numpy / OpenCV on the host, twice per step.  Here the
// frames never leave HBM.  The arithmetic follows OpenCV 4.4's published algorithms (imgwarp.cpp: fixed-point
// coordinates with 10 + 5 fractional bits, 32 x 32 table of a = -0.75 cubic weights held in float, the
// BORDER_CONSTANT edge rule; filter.simd.hpp: RowFilter / SymmColumnFilter summation order, BORDER_REFLECT_101);
// cv2 is not installable here and the reference holds no fixture for it: PARITY UNPINNED (oracle/facewarp.py is the
// same restatement in numpy).  Sums must round like the scalar C code: no product may contract into the sum that follows.
// The pragma below is not enough for that -- the library is compiled with -ffp-contract=fast, and under that flag the
// backend fuses a multiply into an add whatever the front end marked -- so every product that feeds a sum or a
// difference goes through unfused() (tests/test_gpu_face_exact.py compares with numpy, which never contracts).
#include "common.h"

#pragma clang fp contract(off)

namespace {

// The value itself, behind an empty asm statement that the instruction selector cannot look through: the product
// is rounded on its own and the add that consumes it stays an add.  No instruction is emitted for it.
template <typename T>
__device__ __forceinline__ T unfused(T v) {
    asm("" : "+v"(v));
    return v;
}

constexpr int INTER_BITS = 5, INTER_TAB = 1 << INTER_BITS, AB_BITS = 10;

// imgwarp.cpp interpolateCubic (A = -0.75), evaluated in float like initInterTab1D does.  x is a multiple of 1/32, so
// every intermediate below is a dyadic rational of a few bits that f32 holds exactly: contraction cannot change a weight
// (tests/face_ref.py cubic_table asserts it step by step), and the products here need no unfused()
__device__ __forceinline__ void cubic_coeffs(float x, float (&c)[4]) {
#pragma clang fp contract(off)
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// Fixed-point source position of destination pixel (x, y) under the dst -> src matrix M (imgwarp.cpp WarpAffineInvoker):
// (sx, sy) is the first of the 4 x 4 taps, cx / cy the weights of its columns / rows
__device__ __forceinline__ void affine_taps(const double* M, int x, int y, int& sx, int& sy, float (&cx)[4], float (&cy)[4]) {
#pragma clang fp contract(off)
    const double ABS = (double)(1 << AB_BITS);
    const int round_delta = (1 << AB_BITS) / INTER_TAB / 2;
    // cvRound = round-half-to-even, as rint in the default rounding mode
    const int adelta = (int)rint(M[0] * x * ABS), bdelta = (int)rint(M[3] * x * ABS);
    const int X0 = (int)rint((unfused(M[1] * y) + M[2]) * ABS) + round_delta;
    const int Y0 = (int)rint((unfused(M[4] * y) + M[5]) * ABS) + round_delta;
    const int X = (X0 + adelta) >> (AB_BITS - INTER_BITS), Y = (Y0 + bdelta) >> (AB_BITS - INTER_BITS);
    sx = X >> INTER_BITS;
    sy = Y >> INTER_BITS;
    sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);      // saturate_cast<short>
    sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
    sx -= 1;
    sy -= 1;
    cubic_coeffs((float)(X & (INTER_TAB - 1)) * (1.f / INTER_TAB), cx);
    cubic_coeffs((float)(Y & (INTER_TAB - 1)) * (1.f / INTER_TAB), cy);
}

__device__ __forceinline__ bool taps_inner(int sx, int sy, int Hs, int Ws) {
    return (unsigned)sx < (unsigned)(Ws - 3 > 0 ? Ws - 3 : 0) && (unsigned)sy < (unsigned)(Hs - 3 > 0 ? Hs - 3 : 0);
}

__device__ __forceinline__ bool taps_outside(int sx, int sy, int Hs, int Ws) {
    return sx >= Ws || sx + 4 <= 0 || sy >= Hs || sy + 4 <= 0;
}

// One BORDER_CONSTANT cubic sample of the plane P (Hs x Ws) at the taps of affine_taps.  T = element / accumulator type of
// the image (float frames, double masks); weights are float in both cases.  This is the only copy of the tap arithmetic
// and its rounding order: the crop / inverse-warp kernel and the paste kernel both call it.
template <typename T>
__device__ __forceinline__ T cubic_sample(const T* P, int Hs, int Ws, int sx, int sy, const float (&cx)[4],
                                          const float (&cy)[4], T cv, int pre, bool inner, bool outside) {
#pragma clang fp contract(off)
    auto fetch = [&](long off) -> T {
        T v = P[off];
        if (pre) {                                               // VF.normalize(x, [-1]*3, [2]*3).clamp(0, 1) * 255
            float f = ((float)v + 1.f) / 2.f;
            f = unfused(fminf(fmaxf(f, 0.f), 1.f) * 255.f);      // the caller subtracts the border value from it
            v = (T)f;
        }
        return v;
    };
    T sum;
    if (outside) {
        sum = cv;
    } else if (inner) {
        // imgwarp.cpp remapBicubic: the four taps of a row are summed first (left to right), then the row sum is
        // added to the running sum -- sum = row0; sum += row1; ... -- which rounds differently from 16 sequential adds
        sum = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            T row = unfused(fetch((long)(sy + r) * Ws + sx) * (T)(cy[r] * cx[0]));
#pragma unroll
            for (int c = 1; c < 4; ++c) row = row + unfused(fetch((long)(sy + r) * Ws + sx + c) * (T)(cy[r] * cx[c]));
            sum = r == 0 ? row : sum + row;
        }
    } else {
        sum = cv;                                                // cv * ONE, then (S - cv) * w for the taps inside the image
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int yi = sy + r;
            if ((unsigned)yi >= (unsigned)Hs) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int xi = sx + c;
                if ((unsigned)xi < (unsigned)Ws) sum += unfused((fetch((long)yi * Ws + xi) - cv) * (T)(cy[r] * cx[c]));
            }
        }
    }
    return sum;
}

// .astype(np.float32), then / 255 -> VF.normalize(., .5, .5) -> clamp(-1, 1) when post
__device__ __forceinline__ float warp_post(float o, int post) {
#pragma clang fp contract(off)
    if (post) {
        o = ((o / 255.0f) - 0.5f) / 0.5f;
        o = fminf(fmaxf(o, -1.f), 1.f);
    }
    return o;
}

// Output image n is sampled from source image src_index[n] (n itself when src_index is null)
template <typename T>
__global__ __launch_bounds__(256) void warp_affine_cubic_kernel(const T* src, const int* src_index, int Nsrc, int C, int Hs,
                                                                int Ws, const double* minv, int Hd, int Wd, float b0, float b1,
                                                                float b2, float b3, int pre, int post, float* dst, long total) {
#pragma clang fp contract(off)
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % Wd);
    const int y = (int)((i / Wd) % Hd);
    const int n = (int)(i / ((long)Wd * Hd));
    int s = n;
    if (src_index) {                                             // the wrapper checks the range; the clamp keeps a bad list in bounds
        s = src_index[n];
        s = s < 0 ? 0 : (s >= Nsrc ? Nsrc - 1 : s);
    }
    int sx, sy;
    float cx[4], cy[4];
    affine_taps(minv + 6 * n, x, y, sx, sy, cx, cy);
    const float border[4] = {b0, b1, b2, b3};
    const long plane = (long)Hs * Ws;
    const T* S0 = src + (long)s * C * plane;
    const bool inner = taps_inner(sx, sy, Hs, Ws), outside = taps_outside(sx, sy, Hs, Ws);
    for (int k = 0; k < C; ++k) {
        const T sum = cubic_sample<T>(S0 + k * plane, Hs, Ws, sx, sy, cx, cy, (T)border[k & 3], pre, inner, outside);
        dst[((long)n * C + k) * Hd * Wd + (long)y * Wd + x] = warp_post((float)sum, post);
    }
}

// inverse_faces' two warps and the blend of gaussian_diffusion.py:491 per output pixel, for every face of the pixel's frame:
// one thread per pixel, the C channels in registers, faces[frame_start[t] .. frame_start[t + 1]) blended in list order
__global__ __launch_bounds__(256) void face_paste_kernel(const float* x0, int C, int H, int W, const float* faces,
                                                         const double* masks, const double* minv, int K, int h, int w,
                                                         const int* frame_start, float* out, long total) {
#pragma clang fp contract(off)
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const int t = (int)(i / ((long)W * H));
    const long P = (long)H * W, p = (long)y * W + x, fp = (long)h * w;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < C ? x0[((long)t * C + k) * P + p] : 0.f;
    int k0 = frame_start[t], k1 = frame_start[t + 1];           // the wrapper checks the list; the clamp keeps a bad one in bounds
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > K ? K : k1;
    for (int f = k0; f < k1; ++f) {
        int sx, sy;
        float cx[4], cy[4];
        affine_taps(minv + 6 * f, x, y, sx, sy, cx, cy);
        // all 16 taps outside the face: the mask sample is 0 and v * (1 - 0) + face * 0 returns v's bits
        if (taps_outside(sx, sy, h, w)) continue;
        const bool inner = taps_inner(sx, sy, h, w);
        const float m = (float)cubic_sample<double>(masks + f * fp, h, w, sx, sy, cx, cy, 0.0, 0, inner, false);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < C) {
                const float s = cubic_sample<float>(faces + ((long)f * C + k) * fp, h, w, sx, sy, cx, cy, 0.f, 1, inner, false);
                v[k] = unfused(v[k] * (1.f - m)) + unfused(warp_post(s, 1) * m);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < C) out[((long)t * C + k) * P + p] = v[k];
}

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// horizontal pass (filter.simd.hpp RowFilter: sum_k kx[k] * S[i + k], ascending k).  When idx != null the source is the
// parsing map looked up in `lut` (MASK_COLORMAP), else the f64 image `in`.
__global__ __launch_bounds__(256) void blur_row_kernel(const double* in, const int* idx, const double* lut, int nlut,
                                                       const double* kern, int ksize, int H, int W, double* out, long total) {
#pragma clang fp contract(off)
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const long row = i / W;
    const int r = ksize / 2;
    double s = 0;
    for (int k = 0; k < ksize; ++k) {
        const int xi = reflect101(x + k - r, W);
        double v;
        if (idx) {
            int c = idx[row * W + xi];
            c = c < 0 ? 0 : (c >= nlut ? nlut - 1 : c);
            v = lut[c];
        } else {
            v = in[row * W + xi];
        }
        const double t = unfused(kern[k] * v);
        s = k == 0 ? t : s + t;
    }
    out[i] = s;
}

// vertical pass (SymmColumnFilter: ky[0] * S[c] + sum_{k>=1} ky[k] * (S[c + k] + S[c - k])); last pass: zero the
// `edge` outermost pixels and divide by `div`
__global__ __launch_bounds__(256) void blur_col_kernel(const double* in, const double* kern, int ksize, int H, int W, int edge,
                                                       double div, double* out, long total) {
#pragma clang fp contract(off)
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const long base = (i / ((long)W * H)) * (long)W * H;
    const int r = ksize / 2;
    double s = unfused(kern[r] * in[base + (long)y * W + x]);
    for (int k = 1; k <= r; ++k) {
        const double a = in[base + (long)reflect101(y + k, H) * W + x];
        const double b = in[base + (long)reflect101(y - k, H) * W + x];
        s += unfused(kern[r + k] * (a + b));
    }
    if (edge >= 0) {
        if (y < edge || y >= H - edge || x < edge || x >= W - edge) s = 0;
        s = s / div;
    }
    out[i] = s;
}

__global__ __launch_bounds__(256) void face_blend_kernel(const float* x0, const float* face, const float* mask, int C,
                                                         long plane, long total, float* out) {
#pragma clang fp contract(off)
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / (C * plane), p = i % plane;
        const float m = mask[n * plane + p];
        out[i] = unfused(x0[i] * (1.f - m)) + unfused(face[i] * m);
    }
}

}  // namespace

static int launch_warp_affine_cubic(const void* src, int src_is_f64, const int* src_index, int Nsrc, int N, int C, int Hs,
                                    int Ws, const double* minv, int Hd, int Wd, const float* border, int pre, int post,
                                    float* dst, hipStream_t stream) {
    const long total = (long)N * Hd * Wd;
    const int grid = cdiv(total, 256);
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < C; ++k) b[k] = border[k];
    if (src_is_f64)
        hipLaunchKernelGGL(warp_affine_cubic_kernel<double>, dim3(grid), dim3(256), 0, stream, (const double*)src, src_index,
                           Nsrc, C, Hs, Ws, minv, Hd, Wd, b[0], b[1], b[2], b[3], 0, 0, dst, total);
    else
        hipLaunchKernelGGL(warp_affine_cubic_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)src, src_index,
                           Nsrc, C, Hs, Ws, minv, Hd, Wd, b[0], b[1], b[2], b[3], pre, post, dst, total);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_warp_affine_cubic(const void* src, int src_is_f64, int N, int C, int Hs, int Ws, const double* minv,
                                       int Hd, int Wd, const float* border, int pre, int post, float* dst,
                                       hipStream_t stream) {
    FLAIR_CHECK(src && minv && dst && border, "flair_warp_affine_cubic: null argument");
    FLAIR_CHECK(N > 0 && C > 0 && C <= 4 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "flair_warp_affine_cubic: shape");
    FLAIR_CHECK(!src_is_f64 || (!pre && !post), "flair_warp_affine_cubic: the f64 form has no value transforms");
    return launch_warp_affine_cubic(src, src_is_f64, nullptr, N, N, C, Hs, Ws, minv, Hd, Wd, border, pre, post, dst, stream);
}

extern "C" int flair_warp_affine_cubic_indexed(const void* src, int src_is_f64, int Nsrc, const int* src_index, int N, int C,
                                               int Hs, int Ws, const double* minv, int Hd, int Wd, const float* border,
                                               int pre, int post, float* dst, hipStream_t stream) {
    FLAIR_CHECK(src && src_index && minv && dst && border, "flair_warp_affine_cubic_indexed: null argument");
    FLAIR_CHECK(N >= 0 && Nsrc > 0 && C > 0 && C <= 4 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0,
                "flair_warp_affine_cubic_indexed: shape (N = %d >= 0, Nsrc = %d > 0, 0 < C = %d <= 4, sizes > 0)", N, Nsrc, C);
    FLAIR_CHECK(!src_is_f64 || (!pre && !post), "flair_warp_affine_cubic_indexed: the f64 form has no value transforms");
    if (N == 0) return FLAIR_OK;
    return launch_warp_affine_cubic(src, src_is_f64, src_index, Nsrc, N, C, Hs, Ws, minv, Hd, Wd, border, pre, post, dst,
                                    stream);
}

extern "C" int flair_face_paste(const float* x0, int T, int C, int H, int W, const float* faces, const double* masks,
                                const double* minv, int K, int h, int w, const int* frame_start, float* out,
                                hipStream_t stream) {
    FLAIR_CHECK(x0 && out, "flair_face_paste: null x0 / out");
    FLAIR_CHECK(frame_start, "flair_face_paste: null frame_start");
    FLAIR_CHECK(K >= 0 && T > 0 && C > 0 && C <= 4 && H > 0 && W > 0,
                "flair_face_paste: shape (K = %d >= 0, T = %d > 0, 0 < C = %d <= 4, H, W > 0)", K, T, C);
    FLAIR_CHECK(K == 0 || (faces && masks && minv && h > 0 && w > 0),
                "flair_face_paste: K = %d faces need faces, masks, minv and a positive face size", K);
    const long total = (long)T * H * W;
    FLAIR_CHECK(out + total * C <= x0 || x0 + total * C <= out, "flair_face_paste: out may not alias x0");
    hipLaunchKernelGGL(face_paste_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, x0, C, H, W, faces, masks, minv, K,
                       h > 0 ? h : 1, w > 0 ? w : 1, frame_start, out, total);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_face_mask_blur(const int* parse_idx, int N, int H, int W, const double* lut, int nlut,
                                    const double* kern, int ksize, int repeats, int edge, double div, double* tmp,
                                    double* mask, hipStream_t stream) {
    FLAIR_CHECK(parse_idx && lut && kern && tmp && mask, "flair_face_mask_blur: null argument");
    FLAIR_CHECK(N > 0 && H > 1 && W > 1 && nlut > 0 && (ksize & 1) && ksize > 0 && repeats >= 1 && edge >= 0 && div != 0.0,
                "flair_face_mask_blur: shape");
    FLAIR_CHECK(ksize / 2 < 2 * H - 1 && ksize / 2 < 2 * W - 1, "flair_face_mask_blur: kernel wider than two reflections");
    const long total = (long)N * H * W;
    const int grid = cdiv(total, 256);
    for (int r = 0; r < repeats; ++r) {
        hipLaunchKernelGGL(blur_row_kernel, dim3(grid), dim3(256), 0, stream, (const double*)mask, r == 0 ? parse_idx : nullptr,
                           lut, nlut, kern, ksize, H, W, tmp, total);
        FLAIR_LAUNCH_CHECK();
        hipLaunchKernelGGL(blur_col_kernel, dim3(grid), dim3(256), 0, stream, (const double*)tmp, kern, ksize, H, W,
                           r == repeats - 1 ? edge : -1, div, mask, total);
        FLAIR_LAUNCH_CHECK();
    }
    return FLAIR_OK;
}

extern "C" int flair_face_blend(const float* x0, const float* face, const float* mask, int N, int C, int H, int W, float* out,
                                hipStream_t stream) {
    FLAIR_CHECK(x0 && face && mask && out && N > 0 && C > 0 && H > 0 && W > 0, "flair_face_blend: bad argument");
    const long total = (long)N * C * H * W;
    long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(face_blend_kernel, dim3((int)g), dim3(256), 0, stream, x0, face, mask, C, (long)H * W, total, out);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
