// Depthwise 7x7 convolution of VQFR's TextureWarpingModule (vqfr.py:388-396: `nn.Conv2d(c, c, groups=c, kernel_size=7,
// padding=3)` between two GroupNorm + SiLU, which stay on flair_groupnorm_nhwc).  NHWC clip tensors, f32 or bf16, f32
// accumulation, every access 16 bytes wide along C.
//
// A thread owns one 16-byte channel chunk of DW7_R consecutive output pixels of one row: per kernel row it loads the
// DW7_R + 6 input chunks of that row once and the 7 weight chunks once, so one input chunk feeds up to 7 outputs from
// registers (10 loads per kernel row for 4 outputs instead of 28).  Consecutive threads take consecutive chunks of one
// pixel strip, so a wave's loads are contiguous runs along C.
#include "common.h"

namespace {

constexpr int DW7_R = 4;          // output pixels per thread (along W)

template <typename E>
__global__ __launch_bounds__(256) void dw7_kernel(const E* __restrict__ x, int xLd, int H, int W, int C,
                                                  const float* __restrict__ w, const float* __restrict__ bias, long strips,
                                                  E* __restrict__ y, int yLd) {
    constexpr int VEC = ET<E>::VEC;
    const int cv = C / VEC;
    const int ws = (W + DW7_R - 1) / DW7_R;                  // strips per row
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < strips * cv; i += (long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cv) * VEC;
        const long s = i / cv;
        const int w0 = (int)(s % ws) * DW7_R;
        const long r = s / ws;                                // t * H + h
        const int h = (int)(r % H);
        const long f = r / H;
        float acc[DW7_R][VEC];
        {
            float b[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) b[e] = 0.f;
            if (bias) {
#pragma unroll
                for (int e = 0; e < VEC; e += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(bias + c0 + e);
                    b[e] = v.x; b[e + 1] = v.y; b[e + 2] = v.z; b[e + 3] = v.w;
                }
            }
#pragma unroll
            for (int o = 0; o < DW7_R; ++o)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[o][e] = b[e];
        }
        for (int kh = 0; kh < 7; ++kh) {
            const int hh = h + kh - 3;
            if ((unsigned)hh >= (unsigned)H) continue;
            const E* row = x + ((f * H + hh) * W) * (long)xLd + c0;
            float wk[7][VEC];
#pragma unroll
            for (int kw = 0; kw < 7; ++kw)
#pragma unroll
                for (int e = 0; e < VEC; e += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(w + (kh * 7 + kw) * C + c0 + e);
                    wk[kw][e] = v.x; wk[kw][e + 1] = v.y; wk[kw][e + 2] = v.z; wk[kw][e + 3] = v.w;
                }
#pragma unroll
            for (int j = 0; j < DW7_R + 6; ++j) {             // input column w0 - 3 + j
                const int ww = w0 - 3 + j;
                if ((unsigned)ww >= (unsigned)W) continue;
                float v[VEC];
                Vec16<E>::load(row + (long)ww * xLd, v);
#pragma unroll
                for (int o = 0; o < DW7_R; ++o) {
                    const int kw = j - o;
                    if (kw < 0 || kw > 6) continue;           // compile time after unrolling
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[o][e] = fmaf(wk[kw][e], v[e], acc[o][e]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < DW7_R; ++o)
            if (w0 + o < W) Vec16<E>::store(y + ((f * H + h) * W + w0 + o) * (long)yLd + c0, acc[o]);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int flair_dwconv7_nhwc(const void* x, int x_ld, int dtype, int T, int H, int W, int C, const float* w,
                                  const float* bias, void* y, int y_ld, hipStream_t stream) {
    FLAIR_CHECK(x && y && w && T > 0 && H > 0 && W > 0 && C > 0, "flair_dwconv7_nhwc: bad argument (x, y, w, T, H, W, C)");
    FLAIR_CHECK(aligned16(w) && aligned16(bias), "flair_dwconv7_nhwc: w / bias must be 16-byte aligned");
    return flair_by_dtype("flair_dwconv7_nhwc", dtype, [&](auto e) -> int {
        using E = decltype(e);
        constexpr int VEC = ET<E>::VEC;
        FLAIR_CHECK(C % VEC == 0, "flair_dwconv7_nhwc: C = %d is not a multiple of %d", C, VEC);
        FLAIR_CHECK_VIEW("flair_dwconv7_nhwc", "x", x, x_ld, C, VEC);
        FLAIR_CHECK_VIEW("flair_dwconv7_nhwc", "y", y, y_ld, C, VEC);
        const long strips = (long)T * H * ((W + DW7_R - 1) / DW7_R);
        hipLaunchKernelGGL(dw7_kernel<E>, dim3(grid_for(strips * (C / VEC), 256, 8192)), dim3(256), 0, stream, (const E*)x, x_ld, H,
                           W, C, w, bias, strips, (E*)y, y_ld);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}
