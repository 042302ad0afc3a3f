// Tiled denoising's two kernels: flair_tile_gather_f32 cuts whole frames into overlapping tiles of one size and
// flair_tile_blend_f32 sums the tiles' results back into whole frames with feathered weights (include/flair_tile.h, which holds
// the plan, the weights' definition and the entries' contracts; flair_amd/tiling.py is the caller).
//
//   Both are streaming kernels on NCHW f32: one thread per 4 consecutive pixels of a row, lanes along x, so a wave moves 1 KiB
//   of a row per instruction where rows and origins are 16-byte aligned; where an address is not (odd widths, origins that are
//   no multiple of 4, a misaligned base) that thread moves its pixels one by one.  A workgroup stays inside one plane (gather)
//   or one frame (blend), so every index below the plane is 32-bit and only the plane's offset is 64-bit.  No LDS, no atomics.
//   The origins come from device memory and are not trusted: a tile that does not lie inside the frame is read as zeros by the
//   gather and skipped by the blend.
//
//   The blend's weights are evaluated in float64 (a handful of operations per pixel and covering tile, shared by all channels)
//   and rounded to f32 once; the sum itself is f32 fused multiply-adds in plan order (flair_tile.h has the error count).
#include "common.h"

#include "../../include/flair_tile.h"

namespace {
constexpr int TL_THREADS = 256;
constexpr int TL_CH = 8;                                               // channels a blend thread holds in registers at a time

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ bool inside(int o, int t, int L) { return o >= 0 && o <= L - t; }

// flair_tile.h, "The weights": pixel p of a tile with origin o and side t in a frame of length L (o <= p < o + t)
__device__ __forceinline__ double axis_weight(int p, int o, int t, int L, double ramp) {
    const double dl = (double)(p - o) + 0.5, dr = (double)(o + t - p) - 0.5;
    const double wl = o == 0 ? 1.0 : fmin(1.0, dl / ramp);
    const double wr = o + t == L ? 1.0 : fmin(1.0, dr / ramp);
    return fmin(wl, wr);
}

// block = (tile plane, group of 256 threads of that plane), groups fastest; a plane is one channel of one frame of one tile
__global__ __launch_bounds__(TL_THREADS) void tile_gather_kernel(const float* __restrict__ frame, int N, int C, int H, int W, const int* __restrict__ oy,
                                                                 const int* __restrict__ ox, int cols, int th, int tw, int quads, unsigned blocksPerPlane,
                                                                 float* __restrict__ tiles) {
    const unsigned plane = blockIdx.x / blocksPerPlane;               // (k N + n) C + c
    const unsigned j = (blockIdx.x % blocksPerPlane) * TL_THREADS + threadIdx.x;
    if (j >= (unsigned)th * (unsigned)quads) return;
    const int y = (int)(j / (unsigned)quads), x = (int)(j % (unsigned)quads) * 4;
    const int nx = tw - x < 4 ? tw - x : 4;
    const unsigned c = plane % (unsigned)C, kn = plane / (unsigned)C;
    const unsigned n = kn % (unsigned)N, k = kn / (unsigned)N;
    const int o_y = oy[k / (unsigned)cols], o_x = ox[k % (unsigned)cols];
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (inside(o_y, th, H) && inside(o_x, tw, W)) {
        const float* src = frame + (((size_t)n * C + c) * H + (size_t)(o_y + y)) * (size_t)W + (size_t)(o_x + x);
        if (nx == 4 && aligned16(src)) {
            const float4 q = *reinterpret_cast<const float4*>(src);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < nx) v[e] = src[e];
        }
    }
    float* dst = tiles + ((size_t)plane * th + (size_t)y) * (size_t)tw + (size_t)x;
    if (nx == 4 && aligned16(dst)) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < nx) dst[e] = v[e];
    }
}

// block = (frame, group of 256 threads of that frame), groups fastest; a thread owns 4 pixels of one row, all channels
__global__ __launch_bounds__(TL_THREADS) void tile_blend_kernel(const float* __restrict__ tiles, int N, int C, int H, int W, const int* __restrict__ oy, int rows,
                                                                const int* __restrict__ ox, int cols, int th, int tw, double ramp, int quads,
                                                                unsigned blocksPerFrame, float* __restrict__ out) {
    const unsigned n = blockIdx.x / blocksPerFrame;
    const unsigned j = (blockIdx.x % blocksPerFrame) * TL_THREADS + threadIdx.x;
    if (j >= (unsigned)H * (unsigned)quads) return;
    const int y = (int)(j / (unsigned)quads), x0 = (int)(j % (unsigned)quads) * 4;
    const int nx = W - x0 < 4 ? W - x0 : 4;

    // the denominators: the sum of the covering rows' weights, and per pixel of the covering columns'
    double sy = 0.0, sx[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < rows; ++r) {
        const int o = oy[r];
        if (inside(o, th, H) && y >= o && y < o + th) sy += axis_weight(y, o, th, H, ramp);
    }
    for (int c = 0; c < cols; ++c) {
        const int o = ox[c];
        if (!inside(o, tw, W) || x0 + nx <= o || x0 >= o + tw) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int p = x0 + e;
            if (e < nx && p >= o && p < o + tw) sx[e] += axis_weight(p, o, tw, W, ramp);
        }
    }

    const size_t plane = (size_t)th * (size_t)tw;
    for (int c0 = 0; c0 < C; c0 += TL_CH) {
        // -0 is the sum's neutral element: fma(w, v, -0) is the rounded product w v, also where that is a zero of either sign
        float acc[TL_CH][4];
#pragma unroll
        for (int cc = 0; cc < TL_CH; ++cc)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[cc][e] = -0.f;
        for (int r = 0; r < rows; ++r) {
            const int o_y = oy[r];
            if (!inside(o_y, th, H) || y < o_y || y >= o_y + th) continue;
            const double wy = axis_weight(y, o_y, th, H, ramp) / sy;
            for (int c = 0; c < cols; ++c) {
                const int o_x = ox[c];
                if (!inside(o_x, tw, W) || x0 + nx <= o_x || x0 >= o_x + tw) continue;
                bool in[4];
                float w[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int p = x0 + e;
                    in[e] = e < nx && p >= o_x && p < o_x + tw;
                    w[e] = in[e] ? (float)(wy * (axis_weight(p, o_x, tw, W, ramp) / sx[e])) : 0.f;      // rounded to f32 once
                }
                const bool all4 = in[0] && in[1] && in[2] && in[3];
                const size_t k = (size_t)r * (size_t)cols + (size_t)c;
                const float* t0 = tiles + ((k * N + n) * C + (size_t)c0) * plane + (size_t)(y - o_y) * (size_t)tw;
                const int xo = x0 - o_x;                                   // of the thread's first pixel in the tile's row; negative left of the tile
#pragma unroll
                for (int cc = 0; cc < TL_CH; ++cc) {
                    if (c0 + cc >= C) break;
                    const float* row = t0 + (size_t)cc * plane;
                    float v[4] = {0.f, 0.f, 0.f, 0.f};
                    if (all4 && aligned16(row + xo)) {
                        const float4 q = *reinterpret_cast<const float4*>(row + xo);
                        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (in[e]) v[e] = row[xo + e];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (in[e]) acc[cc][e] = fmaf(w[e], v[e], acc[cc][e]);
                }
            }
        }
#pragma unroll
        for (int cc = 0; cc < TL_CH; ++cc) {
            if (c0 + cc >= C) break;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = sy > 0.0 && sx[e] > 0.0 ? acc[cc][e] : 0.f;              // no tile covers the pixel: 0
            float* dst = out + (((size_t)n * C + (size_t)(c0 + cc)) * H + (size_t)y) * (size_t)W + (size_t)x0;
            if (nx == 4 && aligned16(dst)) {
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nx) dst[e] = v[e];
            }
        }
    }
}

bool overlaps(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}

struct Sizes {
    size_t frame_bytes, tile_bytes;
};

// The refusals both entries share.  `frame` is the whole-frame tensor (the gather's input, the blend's output).
int check_plan(const char* fn, const void* frame, const char* frame_name, const void* tiles, const int* oy, const int* ox, int N, int C, int H, int W, int rows,
               int cols, int th, int tw, Sizes& sz) {
    FLAIR_CHECK(frame && tiles && oy && ox, "%s: null pointer (%s = %p, tiles = %p, oy = %p, ox = %p)", fn, frame_name, frame, tiles, (const void*)oy,
                (const void*)ox);
    FLAIR_CHECK(N >= 1 && C >= 1 && rows >= 1 && cols >= 1, "%s: N = %d, C = %d, rows = %d, cols = %d must be positive", fn, N, C, rows, cols);
    FLAIR_CHECK(th >= 1 && tw >= 1 && th <= H && tw <= W, "%s: tiles of %d x %d pixels must be positive and fit the %d x %d frame", fn, th, tw, H, W);
    const double tile_elems = (double)rows * (double)cols * (double)N * (double)C * (double)th * (double)tw;       // in double first: six ints can pass 2^63
    FLAIR_CHECK(tile_elems * 4.0 < 9.0e18 && (double)N * (double)C * (double)H * (double)W * 4.0 < 9.0e18, "%s: %d x %d tiles of N = %d, C = %d exceed 64-bit offsets", fn,
                rows, cols, N, C);
    sz.frame_bytes = (size_t)N * (size_t)C * (size_t)H * (size_t)W * 4;
    sz.tile_bytes = (size_t)rows * (size_t)cols * (size_t)N * (size_t)C * (size_t)th * (size_t)tw * 4;
    FLAIR_CHECK(!overlaps(frame, sz.frame_bytes, tiles, sz.tile_bytes), "%s: %s overlaps tiles (%s = %p, %zu bytes; tiles = %p, %zu bytes)", fn, frame_name,
                frame_name, frame, sz.frame_bytes, tiles, sz.tile_bytes);
    return FLAIR_OK;
}
}  // namespace

extern "C" int flair_tile_gather_f32(const float* frame, int N, int C, int H, int W, const int* oy, int rows, const int* ox, int cols, int th, int tw,
                                     float* tiles, hipStream_t stream) {
    Sizes sz;
    const int st = check_plan("flair_tile_gather_f32", frame, "frame", tiles, oy, ox, N, C, H, W, rows, cols, th, tw, sz);
    if (st != FLAIR_OK) return st;
    const int quads = cdiv(tw, 4);
    const long per_plane = cdiv((long)th * quads, TL_THREADS);
    const double blocks = (double)rows * (double)cols * (double)N * (double)C * (double)per_plane;
    FLAIR_CHECK((long)th * quads <= 0x7fffffffL && blocks <= (double)0x7fffffffL,
                "flair_tile_gather_f32: %d x %d tiles of %d x %d pixels, N = %d, C = %d exceed one launch of 2^31 - 1 workgroups", rows, cols, th, tw, N, C);
    hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)blocks), dim3(TL_THREADS), 0, stream, frame, N, C, H, W, oy, ox, cols, th, tw, quads,
                       (unsigned)per_plane, tiles);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_tile_blend_f32(const float* tiles, int N, int C, int H, int W, const int* oy, int rows, const int* ox, int cols, int th, int tw,
                                    int ramp, float* out, hipStream_t stream) {
    Sizes sz;
    const int st = check_plan("flair_tile_blend_f32", out, "out", tiles, oy, ox, N, C, H, W, rows, cols, th, tw, sz);
    if (st != FLAIR_OK) return st;
    FLAIR_CHECK(ramp >= 1, "flair_tile_blend_f32: ramp = %d pixels must be at least 1", ramp);
    const int quads = cdiv(W, 4);
    const long per_frame = cdiv((long)H * quads, TL_THREADS);
    const double blocks = (double)N * (double)per_frame;
    FLAIR_CHECK((long)H * quads <= 0x7fffffffL && blocks <= (double)0x7fffffffL,
                "flair_tile_blend_f32: N = %d frames of %d x %d pixels exceed one launch of 2^31 - 1 workgroups", N, H, W);
    hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)blocks), dim3(TL_THREADS), 0, stream, tiles, N, C, H, W, oy, rows, ox, cols, th, tw, (double)ramp,
                       quads, (unsigned)per_frame, out);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
