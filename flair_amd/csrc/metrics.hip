// PSNR / SSIM of written frames: flair_image_metrics (include/flair_hip.h, "image metrics").
//
// One workgroup of 256 threads owns a TH x TW = 32 x 64 tile of the SSIM map of one (frame, channel):
//   1. stage    the haloed 42 x 74 byte tiles of a and b into LDS (bytes, 80-byte rows); every thread squares the differences of
//               the bytes its workgroup OWNS (the tile's 32 x 64 pixels, plus the halo where the tile is the frame's last in a
//               direction, so that every byte of the frame is counted once) in integers;
//   2. rows     the horizontal 11-tap pass of the five moment planes x, y, x^2, y^2, xy (x and y shifted by -128: variances and the
//               covariance do not depend on the shift, the products stay exact integers below 2^14 and the cancellation in
//               E[x^2] - mu^2 shrinks) into LDS, four adjacent outputs per thread from four dwords of each byte row;
//   3. columns  the vertical pass, eight rows of one column per thread (lane = column: conflict-free), then the SSIM of each;
//   4. reduce   shuffles inside a wave, LDS across the four waves, ONE partial (SSIM sum, squared error) per workgroup into ws.
// A second launch sums each frame's partials in a fixed order in double: no floating-point atomic anywhere, so two runs give
// the same bits and a frame's result does not depend on how many frames the call holds.
#include "common.h"

namespace {
constexpr int MT_TW = 64, MT_TH = 32, MT_HALO = 10;
constexpr int MT_IW = MT_TW + MT_HALO, MT_IH = MT_TH + MT_HALO;      // 74 x 42 staged bytes per image
constexpr int MT_PITCH = 80;                                          // bytes per staged row: 20 dwords
constexpr int MT_THREADS = 256;
constexpr int MT_ROWS = MT_TH / (MT_THREADS / MT_TW);                 // 8 map rows per thread in the vertical pass
static_assert(MT_THREADS % MT_TW == 0 && MT_TH % (MT_THREADS / MT_TW) == 0 && MT_TW % 4 == 0, "tile / thread mapping");
static_assert(MT_PITCH % 4 == 0 && MT_PITCH >= MT_TW + 12, "a thread of the row pass reads dwords g .. g + 3 of a byte row");
// The frame's bytes a workgroup may own are at most 42 x 74 x 255^2 = 2.03e8: a 32-bit sum is exact.

// exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, normalised in double and rounded to float (their sum is 1 - 1.4e-9)
constexpr float MT_G[11] = {0.00102838008447911f, 0.007598758135239185f, 0.03600077212843083f, 0.10936068950970002f,
                            0.2130055377112537f,  0.26601172486179436f,  0.2130055377112537f,  0.10936068950970002f,
                            0.03600077212843083f, 0.007598758135239185f, 0.00102838008447911f};
constexpr float MT_C1 = 6.5025f, MT_C2 = 58.5225f;                    // (0.01 * 255)^2, (0.03 * 255)^2

__device__ __forceinline__ float byte_of(const uint32_t (&w)[4], int j) {
    return (float)((w[j >> 2] >> (8 * (j & 3))) & 0xffu) - 128.f;
}

__global__ __launch_bounds__(MT_THREADS) void image_metrics_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                         int H, int W, int tilesX, int tiles,
                                                                         double* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) uint8_t sa[MT_IH * MT_PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t sb[MT_IH * MT_PITCH];
    __shared__ __attribute__((aligned(16))) float hm[5][MT_IH][MT_TW];
    __shared__ double red_ssim[MT_THREADS / FLAIR_WAVE];
    __shared__ unsigned red_sse[MT_THREADS / FLAIR_WAVE];

    const int tid = threadIdx.x;
    const unsigned bid = blockIdx.x;                       // = (n * 3 + c) * tiles + t: the partial's index in ws
    const int t = (int)(bid % (unsigned)tiles);
    const int c = (int)(bid / (unsigned)tiles % 3u);
    const size_t n = bid / (unsigned)tiles / 3u;
    const int ty = t / tilesX, tx = t - ty * tilesX;
    const int y0 = ty * MT_TH, x0 = tx * MT_TW;
    const int mh = H - MT_HALO, mw = W - MT_HALO;          // the SSIM map
    const bool lastRow = y0 + MT_TH >= mh, lastCol = x0 + MT_TW >= mw;

    // 1. stage + squared error of the owned bytes
    unsigned sse = 0;
    for (int e = tid; e < MT_IH * MT_IW; e += MT_THREADS) {
        const int r = e / MT_IW, col = e - r * MT_IW;
        const int gy = y0 + r, gx = x0 + col;
        int va = 0, vb = 0;
        if (gy < H && gx < W) {
            const size_t idx = ((n * (size_t)H + (size_t)gy) * (size_t)W + (size_t)gx) * 3u + (size_t)c;
            va = a[idx];
            vb = b[idx];
            if ((r < MT_TH || lastRow) && (col < MT_TW || lastCol)) sse += (unsigned)((va - vb) * (va - vb));
        }
        sa[r * MT_PITCH + col] = (uint8_t)va;
        sb[r * MT_PITCH + col] = (uint8_t)vb;
    }
    __syncthreads();

    // 2. horizontal pass: item = (row, group of four adjacent outputs)
    for (int item = tid; item < MT_IH * (MT_TW / 4); item += MT_THREADS) {
        const int r = item / (MT_TW / 4), g = item - r * (MT_TW / 4);
        const uint32_t* pa = reinterpret_cast<const uint32_t*>(sa + r * MT_PITCH) + g;
        const uint32_t* pb = reinterpret_cast<const uint32_t*>(sb + r * MT_PITCH) + g;
        const uint32_t wa[4] = {pa[0], pa[1], pa[2], pa[3]}, wb[4] = {pb[0], pb[1], pb[2], pb[3]};
        float x[14], y[14], xx[14], yy[14], xy[14];
#pragma unroll
        for (int j = 0; j < 14; ++j) {
            x[j] = byte_of(wa, j);
            y[j] = byte_of(wb, j);
            xx[j] = x[j] * x[j];
            yy[j] = y[j] * y[j];
            xy[j] = x[j] * y[j];
        }
        float o[5][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                s0 = fmaf(MT_G[k], x[q + k], s0);
                s1 = fmaf(MT_G[k], y[q + k], s1);
                s2 = fmaf(MT_G[k], xx[q + k], s2);
                s3 = fmaf(MT_G[k], yy[q + k], s3);
                s4 = fmaf(MT_G[k], xy[q + k], s4);
            }
            o[0][q] = s0; o[1][q] = s1; o[2][q] = s2; o[3][q] = s3; o[4][q] = s4;
        }
#pragma unroll
        for (int p = 0; p < 5; ++p)
            *reinterpret_cast<float4*>(&hm[p][r][4 * g]) = make_float4(o[p][0], o[p][1], o[p][2], o[p][3]);
    }
    __syncthreads();

    // 3. vertical pass: map rows r0 .. r0 + 7 of column col, from rows r0 .. r0 + 17 of the horizontal planes
    const int col = tid % MT_TW, r0 = tid / MT_TW * MT_ROWS;
    float acc[5][MT_ROWS];
#pragma unroll
    for (int p = 0; p < 5; ++p)
#pragma unroll
        for (int i = 0; i < MT_ROWS; ++i) acc[p][i] = 0.f;
#pragma unroll
    for (int k = 0; k < MT_ROWS + MT_HALO; ++k) {
        float v[5];
#pragma unroll
        for (int p = 0; p < 5; ++p) v[p] = hm[p][r0 + k][col];
#pragma unroll
        for (int i = 0; i < MT_ROWS; ++i) {
            const int tap = k - i;
            if (tap >= 0 && tap <= MT_HALO) {
#pragma unroll
                for (int p = 0; p < 5; ++p) acc[p][i] = fmaf(MT_G[tap], v[p], acc[p][i]);
            }
        }
    }
    float tile_sum = 0.f;
#pragma unroll
    for (int i = 0; i < MT_ROWS; ++i) {
        const float hx = acc[0][i], hy = acc[1][i];
        const float mux = hx + 128.f, muy = hy + 128.f;
        const float vx = fmaf(-hx, hx, acc[2][i]), vy = fmaf(-hy, hy, acc[3][i]), cxy = fmaf(-hx, hy, acc[4][i]);
        const float num = (2.f * (mux * muy) + MT_C1) * (2.f * cxy + MT_C2);
        const float den = (mux * mux + muy * muy + MT_C1) * (vx + vy + MT_C2);
        const float s = num / den;
        tile_sum += (y0 + r0 + i < mh && x0 + col < mw) ? s : 0.f;
    }

    // 4. one partial per workgroup
    double ds = (double)tile_sum;
#pragma unroll
    for (int off = FLAIR_WAVE / 2; off > 0; off >>= 1) {
        ds += __shfl_down(ds, off, FLAIR_WAVE);
        sse += __shfl_down(sse, off, FLAIR_WAVE);
    }
    if ((tid & (FLAIR_WAVE - 1)) == 0) {
        red_ssim[tid / FLAIR_WAVE] = ds;
        red_sse[tid / FLAIR_WAVE] = sse;
    }
    __syncthreads();
    if (tid == 0) {
        double s = red_ssim[0];
        unsigned e = red_sse[0];
#pragma unroll
        for (int w = 1; w < MT_THREADS / FLAIR_WAVE; ++w) {
            s += red_ssim[w];
            e += red_sse[w];
        }
        ws[2 * (size_t)bid] = s;
        ws[2 * (size_t)bid + 1] = (double)e;
    }
}

// Frame n: out[4n] = sum of the 3 * tiles squared-error partials (integers: exact in double below 2^53),
// out[4n + 1 + c] = sum of channel c's SSIM partials.  Thread i adds partials i, i + 256, ... in that order, then a fixed tree.
__global__ __launch_bounds__(MT_THREADS) void image_metrics_sum_kernel(const double* __restrict__ ws, int tiles,
                                                                        double* __restrict__ out) {
    __shared__ double sh[4][MT_THREADS];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < 3; ++c)
        for (int t = tid; t < tiles; t += MT_THREADS) {
            const double* p = ws + 2 * ((n * 3 + (size_t)c) * (size_t)tiles + (size_t)t);
            s[1 + c] += p[0];
            s[0] += p[1];
        }
    for (int q = 0; q < 4; ++q) sh[q][tid] = s[q];
    for (int off = MT_THREADS / 2; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off)
            for (int q = 0; q < 4; ++q) sh[q][tid] += sh[q][tid + off];
    }
    __syncthreads();
    if (tid < 4) out[4 * n + tid] = sh[tid][0];
}

inline long metrics_tiles(int H, int W) {
    return (long)cdiv(H - MT_HALO, MT_TH) * (long)cdiv(W - MT_HALO, MT_TW);
}
}  // namespace

extern "C" size_t flair_image_metrics_workspace(int N, int H, int W) {
    if (N <= 0 || H <= MT_HALO || W <= MT_HALO) return 0;
    return (size_t)N * 3u * (size_t)metrics_tiles(H, W) * 2u * sizeof(double);
}

extern "C" int flair_image_metrics(const uint8_t* a, const uint8_t* b, int N, int H, int W, double* out, void* ws,
                                   size_t ws_bytes, hipStream_t stream) {
    FLAIR_CHECK(a && b && out && ws, "flair_image_metrics: null pointer (a = %p, b = %p, out = %p, ws = %p)", (const void*)a,
                (const void*)b, (const void*)out, ws);
    FLAIR_CHECK(N > 0, "flair_image_metrics: N = %d frames, need at least one", N);
    FLAIR_CHECK(H > MT_HALO && W > MT_HALO, "flair_image_metrics: frames of %dx%d are smaller than the 11x11 SSIM window", H, W);
    const long tiles = metrics_tiles(H, W);
    const long groups = (long)N * 3 * tiles;
    FLAIR_CHECK(tiles <= 0x7fffffffL && groups <= 0x7fffffffL, "flair_image_metrics: %ld workgroups (N = %d, %dx%d) exceed one launch",
                groups, N, H, W);
    const size_t need = flair_image_metrics_workspace(N, H, W);
    FLAIR_CHECK(ws_bytes >= need, "flair_image_metrics: ws_bytes = %zu, flair_image_metrics_workspace(%d, %d, %d) = %zu", ws_bytes,
                N, H, W, need);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(ws) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0,
                "flair_image_metrics: ws = %p and out = %p hold doubles and must be 8-byte aligned", ws, (const void*)out);
    hipLaunchKernelGGL(image_metrics_tile_kernel, dim3((unsigned)groups), dim3(MT_THREADS), 0, stream, a, b, H, W,
                       cdiv(W - MT_HALO, MT_TW), (int)tiles, reinterpret_cast<double*>(ws));
    FLAIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(image_metrics_sum_kernel, dim3((unsigned)N), dim3(MT_THREADS), 0, stream,
                       reinterpret_cast<const double*>(ws), (int)tiles, out);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
