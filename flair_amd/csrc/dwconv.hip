// Depthwise-separable block of the RetinaFace MobileNet-0.25 body (facelib/detection/retinaface/retinaface_net.py:25-33,
// `conv_dw`): a per-channel 3x3 convolution (groups = C, stride 1 or 2, zero padding 1) + folded BatchNorm + activation,
// then -- in the same launch -- the 1x1 convolution C -> Cout + folded BatchNorm + activation.  f32 clip tensors
// [T][H][W][ld], channels innermost, every access 16 bytes wide along C.
//
// Fused form: a workgroup owns TP consecutive output pixels.  Stage 1 computes their depthwise result (TP x C) into LDS;
// stage 2 reads it back as the K operand of the 1x1 product (FMAs: f32-input MFMA runs at the f32 vector rate on gfx950,
// so there is nothing to gain from the matrix cores at these widths).  With w_pw == NULL the depthwise result is written
// straight to y by a plain elementwise launch.  The detector's body uses that form followed by the 1x1 on flair_conv_nhwc:
// at the 512^2 shapes the pair takes 512 us for the 13 blocks of a 10-frame window against 852 us fused
// (profiles/retinaface_mobile_detect.txt; the fused 1x1 loop waits on its weight loads with few workgroups in flight).
#include "common.h"

namespace {

constexpr int DW_THREADS = 256;
constexpr int DW_PP = 4;          // output pixels per thread in the 1x1 stage (x 4 output channels)

// depthwise 3x3 + bias + act of output pixel q (linear over T x Ho x Wo), channels c0 .. c0+3
__device__ __forceinline__ float4 dw_pixel(const float* __restrict__ x, int xLd, int H, int W, int Ho, int Wo, int C, int stride,
                                           const float* __restrict__ wdw, const float* __restrict__ bdw, int act, long q, int c0) {
    const int wo = (int)(q % Wo);
    const long r = q / Wo;
    const int ho = (int)(r % Ho);
    const long f = r / Ho;
    float4 acc = bdw ? *reinterpret_cast<const float4*>(bdw + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int h = ho * stride - 1 + kh;
        if ((unsigned)h >= (unsigned)H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int w = wo * stride - 1 + kw;
            if ((unsigned)w >= (unsigned)W) continue;
            const float4 v = *reinterpret_cast<const float4*>(x + ((f * H + h) * W + w) * xLd + c0);
            const float4 k = *reinterpret_cast<const float4*>(wdw + (kh * 3 + kw) * C + c0);
            acc.x += v.x * k.x;
            acc.y += v.y * k.y;
            acc.z += v.z * k.z;
            acc.w += v.w * k.w;
        }
    }
    acc.x = apply_act(acc.x, act);
    acc.y = apply_act(acc.y, act);
    acc.z = apply_act(acc.z, act);
    acc.w = apply_act(acc.w, act);
    return acc;
}

__global__ __launch_bounds__(DW_THREADS) void dw3x3_kernel(const float* __restrict__ x, int xLd, int H, int W, int Ho, int Wo, int C,
                                                          int stride, const float* __restrict__ wdw, const float* __restrict__ bdw,
                                                          int act, long total, float* __restrict__ y, int yLd) {
    const int c4 = C / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total * c4; i += (long)gridDim.x * blockDim.x) {
        const long q = i / c4;
        const int c0 = (int)(i % c4) * 4;
        *reinterpret_cast<float4*>(y + q * yLd + c0) = dw_pixel(x, xLd, H, W, Ho, Wo, C, stride, wdw, bdw, act, q, c0);
    }
}

// One workgroup: output pixels [blockIdx.x * TP, + TP) of the T x Ho x Wo grid.  LDS: TP rows of C + 4 floats (the pad keeps
// the 16-byte rows of neighbouring pixels off the same banks).
__global__ __launch_bounds__(DW_THREADS) void dwpw_kernel(const float* __restrict__ x, int xLd, int H, int W, int Ho, int Wo, int C,
                                                         int stride, const float* __restrict__ wdw, const float* __restrict__ bdw,
                                                         const float* __restrict__ wpw, const float* __restrict__ bpw, int Cout,
                                                         int act, long total, int TP, float* __restrict__ y, int yLd) {
    extern __shared__ float4 dw_smem[];
    float* sdw = reinterpret_cast<float*>(dw_smem);
    const int pitch = C + 4, c4 = C / 4;
    const long p0 = (long)blockIdx.x * TP;
    for (int i = threadIdx.x; i < TP * c4; i += DW_THREADS) {
        const int p = i / c4, c0 = (i % c4) * 4;
        const long q = p0 + p;
        const float4 v = q < total ? dw_pixel(x, xLd, H, W, Ho, Wo, C, stride, wdw, bdw, act, q, c0) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(sdw + p * pitch + c0) = v;
    }
    __syncthreads();
    const int o4 = Cout / 4;
    for (int i = threadIdx.x; i < (TP / DW_PP) * o4; i += DW_THREADS) {
        const int co = (i % o4) * 4, pg = (i / o4) * DW_PP;     // consecutive lanes: consecutive output channels, one pixel group
        const float4 b = bpw ? *reinterpret_cast<const float4*>(bpw + co) : make_float4(0.f, 0.f, 0.f, 0.f);
        float acc[DW_PP][4];
#pragma unroll
        for (int j = 0; j < DW_PP; ++j) {
            acc[j][0] = b.x;
            acc[j][1] = b.y;
            acc[j][2] = b.z;
            acc[j][3] = b.w;
        }
        const float* wrow = wpw + (long)co * C;
#pragma unroll 2
        for (int c = 0; c < C; c += 4) {
            float4 wk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) wk[k] = *reinterpret_cast<const float4*>(wrow + k * C + c);
#pragma unroll
            for (int j = 0; j < DW_PP; ++j) {
                const float4 d = *reinterpret_cast<const float4*>(sdw + (pg + j) * pitch + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[j][k] += d.x * wk[k].x + d.y * wk[k].y + d.z * wk[k].z + d.w * wk[k].w;
            }
        }
#pragma unroll
        for (int j = 0; j < DW_PP; ++j) {
            const long q = p0 + pg + j;
            if (q < total)
                *reinterpret_cast<float4*>(y + q * yLd + co) =
                    make_float4(apply_act(acc[j][0], act), apply_act(acc[j][1], act), apply_act(acc[j][2], act), apply_act(acc[j][3], act));
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int flair_dwconv_nhwc(const float* x, int x_ld, int T, int H, int W, int C, int stride, const float* w_dw, const float* b_dw,
                                 const float* w_pw, const float* b_pw, int Cout, int act, float* y, int y_ld, hipStream_t stream) {
    FLAIR_CHECK(x && y && w_dw && T > 0 && H > 0 && W > 0 && C > 0, "flair_dwconv_nhwc: bad argument (x, y, w_dw, T, H, W, C)");
    FLAIR_CHECK(stride == 1 || stride == 2, "flair_dwconv_nhwc: stride %d (1 or 2)", stride);
    FLAIR_CHECK(C % 4 == 0, "flair_dwconv_nhwc: C = %d is not a multiple of 4", C);
    FLAIR_CHECK(act >= FLAIR_ACT_NONE && act <= FLAIR_ACT_GELU && act != FLAIR_ACT_DCN_OFFSETS, "flair_dwconv_nhwc: activation %d", act);
    const int cy = w_pw ? Cout : C;
    if (w_pw) {
        FLAIR_CHECK(Cout > 0 && Cout % 4 == 0, "flair_dwconv_nhwc: Cout = %d is not a positive multiple of 4", Cout);
        FLAIR_CHECK(C <= 512, "flair_dwconv_nhwc: C = %d > 512 with the 1x1 stage", C);
    }
    FLAIR_CHECK_VIEW("flair_dwconv_nhwc", "x", x, x_ld, C, 4);
    FLAIR_CHECK_VIEW("flair_dwconv_nhwc", "y", y, y_ld, cy, 4);
    FLAIR_CHECK(aligned16(w_dw) && aligned16(b_dw) && aligned16(w_pw) && aligned16(b_pw),
                "flair_dwconv_nhwc: weights and biases must be 16-byte aligned");
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const long total = (long)T * Ho * Wo;
    if (!w_pw) {
        hipLaunchKernelGGL(dw3x3_kernel, dim3(grid_for(total * (C / 4), DW_THREADS, 4096)), dim3(DW_THREADS), 0, stream, x, x_ld, H, W, Ho, Wo,
                           C, stride, w_dw, b_dw, act, total, y, y_ld);
    } else {
        int tp = 256;                                            // pixels per workgroup: LDS of at most ~33 KiB
        while (tp > 16 && tp * C > 8192) tp /= 2;
        const size_t lds = (size_t)tp * (C + 4) * sizeof(float);
        hipLaunchKernelGGL(dwpw_kernel, dim3((unsigned)((total + tp - 1) / tp)), dim3(DW_THREADS), lds, stream, x, x_ld, H, W, Ho, Wo, C,
                           stride, w_dw, b_dw, w_pw, b_pw, Cout, act, total, tp, y, y_ld);
    }
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
