// The flow-warping error, the two kernels of its own: flair_flow_occlusion, flair_warp_error (include/flair_temporal.h, which
// holds the definition and both entries' contracts).  The flows are SPyNet's, made by entries of flair_hip.h; f32 and bytes
// in, float64 inside.  Compiled with -ffp-contract=off (Makefile): every product and sum of the definition is rounded on its own.
//
//   occlusion   one thread per pixel: q = p + f, the four corners of g around q, both tests, one byte out.
//   warp error  a workgroup owns a 32 x 64 tile of one pair for both frame sets: lane = column, a wave owns 8 rows.  Lane,
//               wave, workgroup sums in a fixed order; one (S, N) partial per (set, pair, tile); a second launch adds a
//               pair's tiles in ascending order: no atomics.
#include "common.h"

#include "../../include/flair_temporal.h"

namespace {
constexpr int TP_THREADS = 256;
constexpr int TP_TH = FLAIR_WARP_TILE_H, TP_TW = FLAIR_WARP_TILE_W;
constexpr int TP_WAVES = TP_THREADS / FLAIR_WAVE;
constexpr int TP_ROWS = TP_TH / TP_WAVES;                               // 8 rows per lane
static_assert(TP_TW == FLAIR_WAVE && TP_TH % TP_WAVES == 0, "lane = column, a wave owns whole rows");

// Steps 1 and 2 up to the weights: false for an outside pixel (or a flow that is not a number), else the corners and weights.
struct Tap {
    int x0, x1, y0, y1;
    double l0x, l1x, l0y, l1y;
};
__device__ __forceinline__ bool tap_of(int x, int y, float2 fv, int H, int W, Tap& t) {
    const double qx = (double)x + (double)fv.x, qy = (double)y + (double)fv.y;
    if (!(qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1))) return false;
    t.x0 = (int)qx;                                                       // q >= 0: truncation is floor; x0 <= W - 1
    t.y0 = (int)qy;
    t.x1 = t.x0 + 1 < W ? t.x0 + 1 : W - 1;
    t.y1 = t.y0 + 1 < H ? t.y0 + 1 : H - 1;
    t.l1x = qx - (double)t.x0;
    t.l1y = qy - (double)t.y0;
    t.l0x = 1.0 - t.l1x;
    t.l0y = 1.0 - t.l1y;
    return true;
}
__device__ __forceinline__ double blend(const Tap& t, double v00, double v01, double v10, double v11) {
    return t.l0y * (t.l0x * v00 + t.l1x * v01) + t.l1y * (t.l0x * v10 + t.l1x * v11);
}

// ---- occlusion ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TP_THREADS) void flow_occlusion_kernel(const float2* __restrict__ f, const float2* __restrict__ g, long total,
                                                                     int H, int W, uint8_t* __restrict__ mask) {
    const long i = (long)blockIdx.x * TP_THREADS + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const float2 fv = f[i];
    Tap t;
    bool keep = tap_of(x, y, fv, H, W, t);
    if (keep) {
        const float2* gp = g + (i - ((long)y * W + x));                   // this pair's plane
        const float2 g00 = gp[(size_t)t.y0 * W + t.x0], g01 = gp[(size_t)t.y0 * W + t.x1];
        const float2 g10 = gp[(size_t)t.y1 * W + t.x0], g11 = gp[(size_t)t.y1 * W + t.x1];
        const double gx = blend(t, (double)g00.x, (double)g01.x, (double)g10.x, (double)g11.x);
        const double gy = blend(t, (double)g00.y, (double)g01.y, (double)g10.y, (double)g11.y);
        const double fx = (double)fv.x, fy = (double)fv.y;
        const double sx = fx + gx, sy = fy + gy;
        const double ff = fx * fx + fy * fy, gg = gx * gx + gy * gy;
        const bool occluded = sx * sx + sy * sy > 0.01 * (ff + gg) + 0.5;
        double dxx = 0.0, dxy = 0.0, dyx = 0.0, dyy = 0.0;
        if (x + 1 < W) {
            const float2 n = f[i + 1];
            dxx = (double)n.x - fx;
            dxy = (double)n.y - fy;
        }
        if (y + 1 < H) {
            const float2 n = f[i + W];
            dyx = (double)n.x - fx;
            dyy = (double)n.y - fy;
        }
        const bool boundary = (dxx * dxx + dxy * dxy) + (dyx * dyx + dyy * dyy) > 0.01 * ff + 0.002;
        keep = !occluded && !boundary;
    }
    mask[i] = keep ? 1 : 0;
}

// ---- warp error ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double squared_error(const Tap& t, const uint8_t* __restrict__ pa, const uint8_t* __restrict__ pb, int W) {
    const uint8_t* b00 = pb + ((size_t)t.y0 * W + t.x0) * 3;
    const uint8_t* b01 = pb + ((size_t)t.y0 * W + t.x1) * 3;
    const uint8_t* b10 = pb + ((size_t)t.y1 * W + t.x0) * 3;
    const uint8_t* b11 = pb + ((size_t)t.y1 * W + t.x1) * 3;
    double e = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double d = (double)pa[c] - blend(t, (double)b00[c], (double)b01[c], (double)b10[c], (double)b11[c]);
        e = c == 0 ? d * d : e + d * d;
    }
    return e;
}

// ws: [sets][P][tiles][2]; block = (pair, tile)
__global__ __launch_bounds__(TP_THREADS) void warp_error_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ a2,
                                                                      const float2* __restrict__ f, const uint8_t* __restrict__ mask, int P,
                                                                      int H, int W, int tilesX, int tiles, double* __restrict__ ws) {
    __shared__ double red_s[2][TP_WAVES];
    __shared__ unsigned red_n[TP_WAVES];
    const int tid = threadIdx.x, lane = tid & (FLAIR_WAVE - 1), wave = tid / FLAIR_WAVE;
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const size_t pair = blockIdx.x / (unsigned)tiles;
    const int x = (tile % tilesX) * TP_TW + lane, yTop = (tile / tilesX) * TP_TH + wave * TP_ROWS;
    const size_t plane = (size_t)H * (size_t)W;
    const float2* fp = f + pair * plane;
    const uint8_t* mp = mask + pair * plane;
    const uint8_t* pa = a + pair * plane * 3;
    const uint8_t* pa2 = a2 ? a2 + pair * plane * 3 : nullptr;

    double s0 = 0.0, s1 = 0.0;
    unsigned n = 0;
    if (x < W) {
        for (int r = 0; r < TP_ROWS; ++r) {
            const int y = yTop + r;
            if (y >= H) break;
            const size_t p = (size_t)y * W + x;
            Tap t;
            if (!mp[p] || !tap_of(x, y, fp[p], H, W, t)) continue;
            n += 1;
            s0 += squared_error(t, pa + p * 3, pa + plane * 3, W);
            if (pa2) s1 += squared_error(t, pa2 + p * 3, pa2 + plane * 3, W);
        }
    }
#pragma unroll
    for (int off = FLAIR_WAVE / 2; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, FLAIR_WAVE);
        s1 += __shfl_down(s1, off, FLAIR_WAVE);
        n += __shfl_down(n, off, FLAIR_WAVE);
    }
    if (lane == 0) {
        red_s[0][wave] = s0;
        red_s[1][wave] = s1;
        red_n[wave] = n;
    }
    __syncthreads();
    if (tid < 2 && (tid == 0 || a2)) {
        double s = red_s[tid][0];
        unsigned c = red_n[0];
#pragma unroll
        for (int w = 1; w < TP_WAVES; ++w) {
            s += red_s[tid][w];
            c += red_n[w];
        }
        double* o = ws + 2 * (((size_t)tid * (size_t)P + pair) * (size_t)tiles + (size_t)tile);
        o[0] = s;
        o[1] = (double)c;
    }
}

// out[cell] = (S, N) of cell = set * P + pair: its tiles' partials added in ascending order, eight loads in flight
__global__ __launch_bounds__(FLAIR_WAVE) void warp_error_sum_kernel(const double* __restrict__ ws, long cells, int tiles, double* __restrict__ out) {
    const long cell = (long)blockIdx.x * FLAIR_WAVE + threadIdx.x;
    if (cell >= cells) return;
    const double2* p = reinterpret_cast<const double2*>(ws) + (size_t)cell * (size_t)tiles;
    double s = 0.0, n = 0.0;
    int t = 0;
    for (; t + 8 <= tiles; t += 8) {
        double2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[t + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s += v[j].x;
            n += v[j].y;
        }
    }
    for (; t < tiles; ++t) {
        s += p[t].x;
        n += p[t].y;
    }
    out[2 * cell] = s;
    out[2 * cell + 1] = n;
}
}  // namespace

extern "C" int flair_flow_occlusion(const float* f, const float* g, int P, int H, int W, uint8_t* mask, hipStream_t stream) {
    FLAIR_CHECK(f && g && mask, "flair_flow_occlusion: null pointer (f = %p, g = %p, mask = %p)", (const void*)f, (const void*)g, (const void*)mask);
    FLAIR_CHECK(P >= 1 && H >= 1 && W >= 1, "flair_flow_occlusion: P = %d, H = %d, W = %d must be positive", P, H, W);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(f) % 8 == 0 && reinterpret_cast<uintptr_t>(g) % 8 == 0,
                "flair_flow_occlusion: f = %p and g = %p hold (dx, dy) pairs and must be 8-byte aligned", (const void*)f, (const void*)g);
    FLAIR_CHECK((double)P * (double)H * (double)W <= (double)0x7fffffffL * TP_THREADS,      // in double first: three ints can pass 2^63
                "flair_flow_occlusion: P = %d pairs of %d x %d pixels exceed one launch of 2^31 - 1 workgroups", P, H, W);
    const long total = (long)P * (long)H * (long)W;
    hipLaunchKernelGGL(flow_occlusion_kernel, dim3((unsigned)grid_for(total, TP_THREADS, GRID_NO_CAP)), dim3(TP_THREADS), 0, stream,
                       reinterpret_cast<const float2*>(f), reinterpret_cast<const float2*>(g), total, H, W, mask);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_warp_error(const uint8_t* a, const uint8_t* a2, const float* f, const uint8_t* mask, int P, int H, int W, double* out,
                                void* ws, size_t ws_bytes, hipStream_t stream) {
    FLAIR_CHECK(a && f && mask && out && ws, "flair_warp_error: null pointer (a = %p, f = %p, mask = %p, out = %p, ws = %p; a2 may be null)",
                (const void*)a, (const void*)f, (const void*)mask, (const void*)out, ws);
    FLAIR_CHECK(P >= 1 && H >= 1 && W >= 1, "flair_warp_error: P = %d, H = %d, W = %d must be positive", P, H, W);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(f) % 8 == 0, "flair_warp_error: f = %p holds (dx, dy) pairs and must be 8-byte aligned", (const void*)f);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(out) % 8 == 0, "flair_warp_error: out = %p holds doubles and must be 8-byte aligned", (const void*)out);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(ws) % 8 == 0, "flair_warp_error: ws = %p holds doubles and must be 8-byte aligned", ws);
    const int tilesX = cdiv(W, TP_TW);
    const long tiles = (long)cdiv(H, TP_TH) * (long)tilesX;               // at most 2^26 * 2^25
    const long sets = a2 ? 2 : 1;
    const double need_d = (double)sets * (double)P * (double)tiles * 16.0;
    FLAIR_CHECK(need_d < 9.0e18 && ws_bytes >= (size_t)sets * (size_t)P * (size_t)tiles * 16,
                "flair_warp_error: ws_bytes = %zu, sets * P * ceil(H / FLAIR_WARP_TILE_H) * ceil(W / FLAIR_WARP_TILE_W) * 16 = %.0f", ws_bytes, need_d);
    FLAIR_CHECK(tiles <= 0x7fffffffL && (long)P * tiles <= 0x7fffffffL,
                "flair_warp_error: %d pairs of %ld tiles (H = %d, W = %d) exceed one launch of 2^31 - 1 workgroups", P, tiles, H, W);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(warp_error_tile_kernel, dim3((unsigned)((long)P * tiles)), dim3(TP_THREADS), 0, stream, a, a2,
                       reinterpret_cast<const float2*>(f), mask, P, H, W, tilesX, (int)tiles, part);
    FLAIR_LAUNCH_CHECK();
    const long cells = sets * P;
    hipLaunchKernelGGL(warp_error_sum_kernel, dim3((unsigned)grid_for(cells, FLAIR_WAVE, GRID_NO_CAP)), dim3(FLAIR_WAVE), 0, stream, part, cells,
                       (int)tiles, out);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
