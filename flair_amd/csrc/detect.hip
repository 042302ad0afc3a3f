// Bandwidth-bound pieces of the YOLOv5-face detectors (facelib/detection/yolov5face): the StemBlock's ceil-mode 2x2 pool,
// SPP's three stride-1 pools in one launch, ShuffleNetV2's concat + channel_shuffle(2), Detect's inference decode and the
// letterbox pre-processing.  NHWC clip tensors [F][H][W][ld], every access 16 bytes wide along C; no atomics, every output
// element is produced by one thread in a fixed evaluation order, so the pools and the interleave are bit-exact.
#include <math.h>

#include "common.h"

namespace {

// nn.MaxPool2d(2, 2, ceil_mode=True): windows clipped at the bottom / right edge
template <typename E>
__global__ __launch_bounds__(256) void maxpool2s2_kernel(const E* __restrict__ x, int xLd, int F, int H, int W, int C,
                                                                 E* __restrict__ y, int yLd) {
    constexpr int VEC = ET<E>::VEC;
    const int cv = C / VEC, Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const long total = (long)F * Ho * Wo * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cv) * VEC;
        long q = i / cv;
        const int wo = (int)(q % Wo);
        q /= Wo;
        const int ho = (int)(q % Ho), f = (int)(q / Ho);
        float m[VEC];
        Vec16<E>::load(x + (((long)f * H + 2 * ho) * W + 2 * wo) * xLd + c0, m);
#pragma unroll
        for (int t = 1; t < 4; ++t) {
            const int h = 2 * ho + (t >> 1), w = 2 * wo + (t & 1);
            if (h >= H || w >= W) continue;
            float v[VEC];
            Vec16<E>::load(x + (((long)f * H + h) * W + w) * xLd + c0, v);
#pragma unroll
            for (int k = 0; k < VEC; ++k) m[k] = fmaxf(m[k], v[k]);
        }
        Vec16<E>::store(y + (((long)f * Ho + ho) * Wo + wo) * yLd + c0, m);
    }
}

// SPP: slice 0 (channels [0, C)) of buf -> MaxPool2d(k_j, 1, k_j / 2) into slice j + 1, j = 0..2, r_j = k_j / 2 increasing.
// One pass over the largest window; the smaller windows take the maximum over their part of it (a maximum is associative
// and commutative, so the ring order gives the same bits as three separate pools).  Positions outside the frame do not take
// part (-inf padding).  Slice 0 is only read, slices 1..3 only written: no thread reads what another writes.
template <typename E>
__global__ __launch_bounds__(256) void spp_pool_kernel(E* __restrict__ buf, int ld, int F, int H, int W, int C, int r0, int r1,
                                                               int r2) {
    constexpr int VEC = ET<E>::VEC;
    const int cv = C / VEC;
    const long total = (long)F * H * W * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cv) * VEC;
        long q = i / cv;
        const int w = (int)(q % W);
        q /= W;
        const int h = (int)(q % H), f = (int)(q / H);
        float m0[VEC], m1[VEC], m2[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) m0[k] = m1[k] = m2[k] = -INFINITY;
        const int hlo = max(h - r2, 0), hhi = min(h + r2, H - 1), wlo = max(w - r2, 0), whi = min(w + r2, W - 1);
        for (int hh = hlo; hh <= hhi; ++hh) {
            const int dh = abs(hh - h);
            const E* row = buf + ((long)f * H + hh) * W * ld + c0;
            for (int ww = wlo; ww <= whi; ++ww) {
                const int d = max(dh, abs(ww - w));
                float v[VEC];
                Vec16<E>::load(row + (long)ww * ld, v);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    m2[k] = fmaxf(m2[k], v[k]);
                    if (d <= r1) m1[k] = fmaxf(m1[k], v[k]);
                    if (d <= r0) m0[k] = fmaxf(m0[k], v[k]);
                }
            }
        }
        E* o = buf + (((long)f * H + h) * W + w) * ld + c0;
        Vec16<E>::store(o + C, m0);
        Vec16<E>::store(o + 2 * C, m1);
        Vec16<E>::store(o + 3 * C, m2);
    }
}

// y[p][2i] = a[p][i], y[p][2i + 1] = b[p][i]: torch.cat((a, b), 1) + channel_shuffle(., 2).  One thread: VEC channels of
// a and of b -> 2 VEC consecutive channels of y (two 16-byte stores).
template <typename E>
__global__ __launch_bounds__(256) void interleave_kernel(const E* __restrict__ a, int aLd, const E* __restrict__ b, int bLd, int C,
                                                                 long P, E* __restrict__ y, int yLd) {
    constexpr int VEC = ET<E>::VEC;
    const int cv = C / VEC;
    const long total = P * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cv) * VEC;
        const long p = i / cv;
        alignas(16) E va[VEC], vb[VEC], lo[VEC], hi[VEC];
        *reinterpret_cast<uint4*>(va) = *reinterpret_cast<const uint4*>(a + p * aLd + c0);
        *reinterpret_cast<uint4*>(vb) = *reinterpret_cast<const uint4*>(b + p * bLd + c0);
#pragma unroll
        for (int k = 0; k < VEC / 2; ++k) {
            lo[2 * k] = va[k];
            lo[2 * k + 1] = vb[k];
            hi[2 * k] = va[VEC / 2 + k];
            hi[2 * k + 1] = vb[VEC / 2 + k];
        }
        E* o = y + p * yLd + 2 * c0;
        *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(lo);
        *reinterpret_cast<uint4*>(o + VEC) = *reinterpret_cast<const uint4*>(hi);
    }
}

constexpr int DET_MAX_NA = 8;
struct AnchorArgs {
    float w[DET_MAX_NA], h[DET_MAX_NA];
};

__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

// Detect.forward, inference branch, one level (yolo.py:52-86).  One thread: the 16 values of (frame b, anchor a, cell y, x).
__global__ __launch_bounds__(256) void yolo_decode_kernel(const float* __restrict__ x, int xLd, int B, int ny, int nx, int na,
                                                                  float stride, AnchorArgs an, float* __restrict__ z, long N, long row0) {
    const long total = (long)B * na * ny * nx;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int gx = (int)(i % nx);
        long q = i / nx;
        const int gy = (int)(q % ny);
        q /= ny;
        const int a = (int)(q % na), b = (int)(q / na);
        const float* src = x + (((long)b * ny + gy) * nx + gx) * xLd + a * 16;
        float v[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) Vec16<float>::load(src + 4 * k, v + 4 * k);
        const float aw = an.w[a], ah = an.h[a], fx = (float)gx, fy = (float)gy;
        float o[16];
        o[0] = (sigmoid_f(v[0]) * 2.0f - 0.5f + fx) * stride;
        o[1] = (sigmoid_f(v[1]) * 2.0f - 0.5f + fy) * stride;
        const float sw = sigmoid_f(v[2]) * 2.f, sh = sigmoid_f(v[3]) * 2.f;
        o[2] = sw * sw * aw;
        o[3] = sh * sh * ah;
        o[4] = sigmoid_f(v[4]);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            o[5 + 2 * k] = v[5 + 2 * k] * aw + fx * stride;
            o[6 + 2 * k] = v[6 + 2 * k] * ah + fy * stride;
        }
        o[15] = sigmoid_f(v[15]);
        float* dst = z + ((long)b * N + row0 + ((long)a * ny + gy) * nx + gx) * 16;
#pragma unroll
        for (int k = 0; k < 4; ++k) Vec16<float>::store(dst + 4 * k, o + 4 * k);
    }
}

struct LetterboxArgs {
    int B, H, W, nh, nw, top, left, Ho, Wo, yLd;
    float a, b, lo, hi, s, pad;
};

// One thread: one output pixel, 16 channels (3 image channels, 13 zeros).
__global__ __launch_bounds__(256) void letterbox_kernel(const float* __restrict__ src, LetterboxArgs p, float* __restrict__ y) {
    const long total = (long)p.B * p.Ho * p.Wo, plane = (long)p.H * p.W;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ox = (int)(i % p.Wo);
        const long q = i / p.Wo;
        const int oy = (int)(q % p.Ho), b = (int)(q / p.Ho);
        const int iy = oy - p.top, ix = ox - p.left;
        float c[4] = {p.pad, p.pad, p.pad, 0.f};
        if (iy >= 0 && iy < p.nh && ix >= 0 && ix < p.nw) {
            const float* im = src + (long)b * 3 * plane;
            if (p.nh == p.H && p.nw == p.W) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    c[ch] = fminf(fmaxf(p.a * im[ch * plane + (long)iy * p.W + ix] + p.b, p.lo), p.hi) * p.s;
            } else {
                // half-pixel centres, clamped edges; the source coordinate in double so that the blend weights carry no
                // rounding of a coordinate in the hundreds
                const double sy = fmax(((double)iy + 0.5) * ((double)p.H / (double)p.nh) - 0.5, 0.0);
                const double sx = fmax(((double)ix + 0.5) * ((double)p.W / (double)p.nw) - 0.5, 0.0);
                const int y0 = min((int)sy, p.H - 1), x0 = min((int)sx, p.W - 1);
                const int y1 = min(y0 + 1, p.H - 1), x1 = min(x0 + 1, p.W - 1);
                const float ly = (float)(sy - (double)y0), lx = (float)(sx - (double)x0);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float* pl = im + ch * plane;
                    const float v00 = fminf(fmaxf(p.a * pl[(long)y0 * p.W + x0] + p.b, p.lo), p.hi);
                    const float v01 = fminf(fmaxf(p.a * pl[(long)y0 * p.W + x1] + p.b, p.lo), p.hi);
                    const float v10 = fminf(fmaxf(p.a * pl[(long)y1 * p.W + x0] + p.b, p.lo), p.hi);
                    const float v11 = fminf(fmaxf(p.a * pl[(long)y1 * p.W + x1] + p.b, p.lo), p.hi);
                    const float top = v00 + lx * (v01 - v00), bot = v10 + lx * (v11 - v10);
                    c[ch] = (top + ly * (bot - top)) * p.s;
                }
            }
        }
        float* o = y + i * p.yLd;
        const float zero[4] = {0.f, 0.f, 0.f, 0.f};
        Vec16<float>::store(o, c);
        Vec16<float>::store(o + 4, zero);
        Vec16<float>::store(o + 8, zero);
        Vec16<float>::store(o + 12, zero);
    }
}

}  // namespace

extern "C" int flair_maxpool2x2s2_nhwc(const void* x, int x_ld, int dtype, int F, int H, int W, int C, void* y, int y_ld,
                                       hipStream_t stream) {
    FLAIR_CHECK(x && y, "flair_maxpool2x2s2_nhwc: x / y is null");
    FLAIR_CHECK(F > 0 && H > 0 && W > 0, "flair_maxpool2x2s2_nhwc: F = %d, H = %d, W = %d must be positive", F, H, W);
    return flair_by_dtype("flair_maxpool2x2s2_nhwc", dtype, [&](auto e) -> int {
        using E = decltype(e);
        constexpr int VEC = ET<E>::VEC;
        FLAIR_CHECK(C > 0 && C % VEC == 0, "flair_maxpool2x2s2_nhwc: C = %d is not a positive multiple of %d", C, VEC);
        FLAIR_CHECK_VIEW("flair_maxpool2x2s2_nhwc", "x", x, x_ld, C, VEC);
        FLAIR_CHECK_VIEW("flair_maxpool2x2s2_nhwc", "y", y, y_ld, C, VEC);
        const long n = (long)F * ((H + 1) / 2) * ((W + 1) / 2) * (C / VEC);
        hipLaunchKernelGGL(maxpool2s2_kernel<E>, dim3(grid_for(n, 256, 4096)), dim3(256), 0, stream, (const E*)x, x_ld, F, H, W, C,
                           (E*)y, y_ld);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}

extern "C" int flair_spp_maxpool_nhwc(void* buf, int ld, int dtype, int F, int H, int W, int C, int k0, int k1, int k2,
                                      hipStream_t stream) {
    FLAIR_CHECK(buf, "flair_spp_maxpool_nhwc: buf is null");
    FLAIR_CHECK(F > 0 && H > 0 && W > 0, "flair_spp_maxpool_nhwc: F = %d, H = %d, W = %d must be positive", F, H, W);
    return flair_by_dtype("flair_spp_maxpool_nhwc", dtype, [&](auto e) -> int {
        using E = decltype(e);
        constexpr int VEC = ET<E>::VEC;
        FLAIR_CHECK(C > 0 && C % VEC == 0, "flair_spp_maxpool_nhwc: C = %d is not a positive multiple of %d", C, VEC);
        FLAIR_CHECK(k0 % 2 == 1 && k1 % 2 == 1 && k2 % 2 == 1 && 3 <= k0 && k0 < k1 && k1 < k2 && k2 <= 13,
                    "flair_spp_maxpool_nhwc: k = (%d, %d, %d) must be odd, strictly increasing, from 3 to 13", k0, k1, k2);
        // not FLAIR_CHECK_VIEW: the buffer holds the input and the three pooled copies side by side, ld >= 4 C (in long: 4 C may overflow)
        FLAIR_CHECK((long)ld >= 4L * C && ld % VEC == 0 && reinterpret_cast<uintptr_t>(buf) % 16 == 0,
                    "flair_spp_maxpool_nhwc: buf stride/alignment: ld = %d must be >= 4 C = %ld and a multiple of %d elements, buf = %p "
                    "16-byte aligned", ld, 4L * C, VEC, (const void*)buf);
        const long n = (long)F * H * W * (C / VEC);
        hipLaunchKernelGGL(spp_pool_kernel<E>, dim3(grid_for(n, 256, 4096)), dim3(256), 0, stream, (E*)buf, ld, F, H, W, C, k0 / 2,
                           k1 / 2, k2 / 2);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}

extern "C" int flair_channel_interleave_nhwc(const void* a, int a_ld, const void* b, int b_ld, int dtype, int C, long P, void* y,
                                             int y_ld, hipStream_t stream) {
    FLAIR_CHECK(a && b && y, "flair_channel_interleave_nhwc: a / b / y is null");
    FLAIR_CHECK(P > 0, "flair_channel_interleave_nhwc: P = %ld must be positive", P);
    return flair_by_dtype("flair_channel_interleave_nhwc", dtype, [&](auto e) -> int {
        using E = decltype(e);
        constexpr int VEC = ET<E>::VEC;
        FLAIR_CHECK(C > 0 && C % VEC == 0, "flair_channel_interleave_nhwc: C = %d is not a positive multiple of %d", C, VEC);
        FLAIR_CHECK_VIEW("flair_channel_interleave_nhwc", "a", a, a_ld, C, VEC);
        FLAIR_CHECK_VIEW("flair_channel_interleave_nhwc", "b", b, b_ld, C, VEC);
        FLAIR_CHECK_VIEW("flair_channel_interleave_nhwc", "y", y, y_ld, 2 * C, VEC);
        hipLaunchKernelGGL(interleave_kernel<E>, dim3(grid_for(P * (C / VEC), 256, 4096)), dim3(256), 0, stream, (const E*)a, a_ld,
                           (const E*)b, b_ld, C, P, (E*)y, y_ld);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}

extern "C" int flair_yolo_face_decode(const float* x, int x_ld, int B, int ny, int nx, int na, int no, float stride,
                                      const float* anchor_grid, float* z, long N, long row0, hipStream_t stream) {
    FLAIR_CHECK(x && z && anchor_grid, "flair_yolo_face_decode: x / z / anchor_grid is null");
    FLAIR_CHECK(no == 16, "flair_yolo_face_decode: no = %d (16 only: box 4, objectness, 5 landmarks, nc = 1)", no);
    FLAIR_CHECK(na >= 1 && na <= DET_MAX_NA, "flair_yolo_face_decode: na = %d (1 to %d)", na, DET_MAX_NA);
    FLAIR_CHECK(B > 0 && ny > 0 && nx > 0, "flair_yolo_face_decode: B = %d, ny = %d, nx = %d must be positive", B, ny, nx);
    FLAIR_CHECK(stride > 0.f, "flair_yolo_face_decode: stride = %g must be positive", (double)stride);
    FLAIR_CHECK_VIEW("flair_yolo_face_decode", "x", x, x_ld, na * 16, 4);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(z) % 16 == 0, "flair_yolo_face_decode: z = %p must be 16-byte aligned", (const void*)z);
    FLAIR_CHECK(row0 >= 0 && row0 + (long)na * ny * nx <= N, "flair_yolo_face_decode: row0 = %ld + na ny nx = %ld rows do not fit N = %ld",
                row0, (long)na * ny * nx, N);
    AnchorArgs an = {};
    for (int a = 0; a < na; ++a) {
        an.w[a] = anchor_grid[2 * a];
        an.h[a] = anchor_grid[2 * a + 1];
    }
    hipLaunchKernelGGL(yolo_decode_kernel, dim3(grid_for((long)B * na * ny * nx, 256, 4096)), dim3(256), 0, stream, x, x_ld, B, ny,
                       nx, na, stride, an, z, N, row0);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_letterbox_nhwc(const float* src, int B, int H, int W, int new_h, int new_w, int top, int left, int Ho, int Wo,
                                    float a, float b, float lo, float hi, float s, float pad_value, float* y, int y_ld,
                                    hipStream_t stream) {
    FLAIR_CHECK(src && y, "flair_letterbox_nhwc: src / y is null");
    FLAIR_CHECK(B > 0 && H > 0 && W > 0, "flair_letterbox_nhwc: B = %d, H = %d, W = %d must be positive", B, H, W);
    FLAIR_CHECK(new_h > 0 && new_w > 0, "flair_letterbox_nhwc: new_h = %d, new_w = %d must be positive", new_h, new_w);
    FLAIR_CHECK(top >= 0 && left >= 0, "flair_letterbox_nhwc: top = %d, left = %d must not be negative", top, left);
    FLAIR_CHECK(Ho >= top + new_h && Wo >= left + new_w, "flair_letterbox_nhwc: Ho = %d, Wo = %d do not hold top + new_h = %d, left + new_w = %d",
                Ho, Wo, top + new_h, left + new_w);
    FLAIR_CHECK(lo <= hi, "flair_letterbox_nhwc: lo = %g > hi = %g", (double)lo, (double)hi);
    FLAIR_CHECK_VIEW("flair_letterbox_nhwc", "y", y, y_ld, 16, 4);
    LetterboxArgs p = {B, H, W, new_h, new_w, top, left, Ho, Wo, y_ld, a, b, lo, hi, s, pad_value};
    hipLaunchKernelGGL(letterbox_kernel, dim3(grid_for((long)B * Ho * Wo, 256, 4096)), dim3(256), 0, stream, src, p, y);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
