// The three launches BiSeNet face parsing needs beyond the shared convolution / resize entries (reference
// guided_diffusion/facelib/parsing/bisenet.py): the global average pool of the attention modules (:45, :70, :100), the
// per-channel gate that applies their attention (:74-75, :79-80, :105-106), and the tail of forward() folded into the
// consumer of its result -- bilinear align_corners=True enlargement of the 1/8-resolution class logits (:127) and the
// arg-max over the classes the face helper takes next (facelib/utils/face_restoration_helper.py:279-281), without the
// enlarged logits ever existing in memory.  No float atomics: every sum has a fixed order, so replays are bit-stable.
#include "common.h"

namespace {

// ---- global average pool: [F][HW][C] -> f32 [F][C].  One workgroup = one frame x POOL_CHUNKS 16-byte channel chunks;
// its 256 threads are POOL_CHUNKS chunk lanes x POOL_LANES pixel lanes (a wave reads 8 pixels x 128 contiguous bytes per
// load).  Every thread sums its pixels i = lane, lane + 32, ... in that order, then one thread per channel adds the 32
// partial sums in lane order: the order depends on HW alone.
constexpr int POOL_CHUNKS = 8;
constexpr int POOL_LANES = 32;

template <typename E>
__global__ __launch_bounds__(256) void global_avgpool_kernel(const E* x, int ld, int HW, int C, float* y, int yLd) {
    constexpr int VEC = ET<E>::VEC;
    constexpr int CB = POOL_CHUNKS * VEC;                   // channels per workgroup
    __shared__ float red[POOL_LANES][CB + 1];
    const int tid = threadIdx.x;
    const int ck = tid % POOL_CHUNKS, pl = tid / POOL_CHUNKS;
    const int c = (blockIdx.x * POOL_CHUNKS + ck) * VEC;
    const int f = blockIdx.y;
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    if (c < C) {
        const E* p = x + (size_t)f * HW * ld + c;
#pragma unroll 4
        for (int i = pl; i < HW; i += POOL_LANES) {
            float v[VEC];
            Vec16<E>::load(p + (size_t)i * ld, v);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] += v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) red[pl][ck * VEC + k] = acc[k];
    __syncthreads();
    const int co = blockIdx.x * CB + tid;
    if (tid < CB && co < C) {
        float s = 0.f;
        for (int l = 0; l < POOL_LANES; ++l) s += red[l][tid];
        y[(size_t)f * yLd + co] = s / (float)HW;
    }
}

// ---- per-channel gate: y = x * g[f][c] (+ x) (+ b[f][c]) (+ a), 16 bytes per thread.  A thread's channel chunk stays
// the same along its grid-stride walk whenever the chunk count divides the stride (every width BiSeNet uses), so the
// sigmoid of a gate logit is evaluated once per thread, not once per element.
template <typename E>
__global__ __launch_bounds__(256) void channel_gate_kernel(const E* x, int xLd, const float* g, int gLd, int gateIsLogit,
                                                           int addX, const float* b, int bLd, const E* a, int aLd, int HW,
                                                           int C, E* y, int yLd) {
    constexpr int VEC = ET<E>::VEC;
    const int cv = C / VEC;
    const int f = blockIdx.y;
    const long total = (long)HW * cv;
    const long stride = (long)gridDim.x * 256;
    float gv[VEC], bv[VEC];
    int cc = -1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += stride) {
        const int c = (int)(i % cv) * VEC;
        const size_t p = (size_t)f * HW + (size_t)(i / cv);
        if (c != cc) {
            cc = c;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float v = g[(size_t)f * gLd + c + k];
                gv[k] = gateIsLogit ? 1.f / (1.f + expf(-v)) : v;
                bv[k] = b ? b[(size_t)f * bLd + c + k] : 0.f;
            }
        }
        float xv[VEC], r[VEC];
        Vec16<E>::load(x + p * xLd + c, xv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            r[k] = xv[k] * gv[k];
            if (addX) r[k] += xv[k];
            r[k] += bv[k];
        }
        if (a) {
            float av[VEC];
            Vec16<E>::load(a + p * aLd + c, av);
#pragma unroll
            for (int k = 0; k < VEC; ++k) r[k] += av[k];
        }
        Vec16<E>::store(y + p * yLd + c, r);
    }
}

// ---- bilinear (align_corners=True) enlargement + arg-max over the classes.  One thread owns one output column of a strip
// of UA_ROWS output rows; lanes are consecutive columns, so the index stores are dense.  The enlargement ratio is
// (h - 1) / (H - 1) (63 / 511 for a 512 x 512 face), not 1 / 8: an output strip does not sit on a source cell, so the thread
// keeps the horizontally blended class vectors of its current pair of source rows in registers (2 x NP floats) and
// reloads them when the strip crosses into the next source row -- about twice per eight output rows at 8x, where the
// literal form loads 4 x N logits per output pixel.  Arithmetic as ATen's upsample_bilinear2d: source = dst * scale in
// float, weights (1 - t, t), value = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11), evaluated without
// contraction into FMAs.
constexpr int UA_ROWS = 8;

// The N class logits of one source pixel as floats.  nload > 0: 16-byte loads of the first nload elements (N rounded up
// to a whole chunk, which the entry has checked to lie inside the pixel stride); nload == 0: element loads.
template <typename E, int NP>
__device__ __forceinline__ void load_classes(const E* p, int N, int nload, float (&v)[NP]) {
    constexpr int VEC = ET<E>::VEC;
    if (nload) {
#pragma unroll
        for (int k = 0; k < NP; k += VEC) {
            if (k < nload) {
                Vec16<E>::load(p + k, &v[k]);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[k + e] = 0.f;
            }
        }
    } else {
#pragma unroll
        for (int n = 0; n < NP; ++n) v[n] = n < N ? ET<E>::ld(p + n) : 0.f;
    }
}

template <typename E, int NP>
__global__ __launch_bounds__(256) void upsample_argmax_kernel(const E* logits, int ld, int h, int w, int N, int nload,
                                                              int H, int W, float sy, float sx, const float* table, int D,
                                                              int* idx, float* y, int yLd) {
#pragma clang fp contract(off)
    const int wo = blockIdx.x * 256 + threadIdx.x;
    if (wo >= W) return;
    const int f = blockIdx.z;
    const int ho0 = blockIdx.y * UA_ROWS;
    const float rx = sx * (float)wo;
    int x0 = (int)rx;
    x0 = x0 > w - 1 ? w - 1 : x0;
    const int x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ax = fminf(fmaxf(rx - (float)x0, 0.f), 1.f), bx = 1.f - ax;
    const E* fb = logits + (size_t)f * h * w * ld;
    float top[NP], bot[NP];
    int cy = -1;
    for (int r = 0; r < UA_ROWS; ++r) {
        const int ho = ho0 + r;
        if (ho >= H) break;
        const float ry = sy * (float)ho;
        int y0 = (int)ry;
        y0 = y0 > h - 1 ? h - 1 : y0;
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0);
        const float ay = fminf(fmaxf(ry - (float)y0, 0.f), 1.f), by = 1.f - ay;
        if (y0 != cy) {                   // the same decision in every lane: it depends on the output row alone
            cy = y0;
            float v0[NP], v1[NP];
            load_classes<E, NP>(fb + ((size_t)y0 * w + x0) * ld, N, nload, v0);
            load_classes<E, NP>(fb + ((size_t)y0 * w + x1) * ld, N, nload, v1);
#pragma unroll
            for (int n = 0; n < NP; ++n) top[n] = bx * v0[n] + ax * v1[n];
            load_classes<E, NP>(fb + ((size_t)y1 * w + x0) * ld, N, nload, v0);
            load_classes<E, NP>(fb + ((size_t)y1 * w + x1) * ld, N, nload, v1);
#pragma unroll
            for (int n = 0; n < NP; ++n) bot[n] = bx * v0[n] + ax * v1[n];
        }
        float best_v = -INFINITY;
        int best = 0;
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            const float v = by * top[n] + ay * bot[n];
            if (n < N && v > best_v) {    // n ascends: a later equal value never replaces (torch.argmax: first index)
                best_v = v;
                best = n;
            }
        }
        const size_t row = ((size_t)f * H + ho) * W + wo;
        if (idx) idx[row] = best;
        if (y)
            for (int c = 0; c < D; ++c) y[row * yLd + c] = table[(size_t)best * D + c];
    }
}

template <typename E>
int launch_upsample_argmax(int np, dim3 grid, hipStream_t stream, const E* logits, int ld, int h, int w, int N, int nload,
                           int H, int W, float sy, float sx, const float* table, int D, int* idx, float* y, int yLd) {
#define FLAIR_UA_CASE(NPV)                                                                                              \
    case NPV:                                                                                                           \
        hipLaunchKernelGGL((upsample_argmax_kernel<E, NPV>), grid, dim3(256), 0, stream, logits, ld, h, w, N, nload, H, W, \
                           sy, sx, table, D, idx, y, yLd);                                                              \
        break;
    switch (np) {
        FLAIR_UA_CASE(8)
        FLAIR_UA_CASE(16)
        FLAIR_UA_CASE(24)
        FLAIR_UA_CASE(32)
        default:
            return -1;
    }
#undef FLAIR_UA_CASE
    return 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int flair_global_avgpool_nhwc(const void* x, int dtype, int x_ld, int F, int H, int W, int C, float* y, int y_ld,
                                         hipStream_t stream) {
    FLAIR_CHECK(x && y, "flair_global_avgpool_nhwc: null argument");
    FLAIR_CHECK(F > 0 && F <= 65535 && H > 0 && W > 0 && C > 0 && (long)H * W <= 0x7fffffffL,
                "flair_global_avgpool_nhwc: bad shape F=%d H=%d W=%d C=%d", F, H, W, C);
    return flair_by_dtype("flair_global_avgpool_nhwc", dtype, [&](auto e) -> int {
        using E = decltype(e);
        constexpr int VEC = ET<E>::VEC;
        FLAIR_CHECK(C % VEC == 0, "flair_global_avgpool_nhwc: C = %d must be a multiple of %d", C, VEC);
        FLAIR_CHECK_VIEW("flair_global_avgpool_nhwc", "x", x, x_ld, C, VEC);
        FLAIR_CHECK(y_ld >= C, "flair_global_avgpool_nhwc: y_ld = %d below C = %d", y_ld, C);      // y: f32 scalars, no pieces
        const dim3 grid(cdiv(C / VEC, POOL_CHUNKS), F);
        hipLaunchKernelGGL(global_avgpool_kernel<E>, grid, dim3(256), 0, stream, (const E*)x, x_ld, H * W, C, y, y_ld);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}

extern "C" int flair_channel_gate_nhwc(const void* x, int x_ld, int dtype, int F, long HW, int C, const float* gate, int gate_ld,
                                       int gate_is_logit, int add_x, const float* bias, int bias_ld, const void* a, int a_ld,
                                       void* y, int y_ld, hipStream_t stream) {
    FLAIR_CHECK(x && gate && y, "flair_channel_gate_nhwc: null argument");
    FLAIR_CHECK(F > 0 && F <= 65535 && HW > 0 && HW <= 0x7fffffffL && C > 0, "flair_channel_gate_nhwc: bad shape F=%d HW=%ld C=%d",
                F, HW, C);
    return flair_by_dtype("flair_channel_gate_nhwc", dtype, [&](auto e) -> int {
        using E = decltype(e);
        constexpr int VEC = ET<E>::VEC;
        FLAIR_CHECK(C % VEC == 0, "flair_channel_gate_nhwc: C = %d must be a multiple of %d", C, VEC);
        FLAIR_CHECK_VIEW("flair_channel_gate_nhwc", "x", x, x_ld, C, VEC);
        FLAIR_CHECK_VIEW("flair_channel_gate_nhwc", "y", y, y_ld, C, VEC);
        if (a) FLAIR_CHECK_VIEW("flair_channel_gate_nhwc", "a", a, a_ld, C, VEC);
        FLAIR_CHECK(gate_ld >= C && (!bias || bias_ld >= C), "flair_channel_gate_nhwc: gate_ld = %d / bias_ld = %d below C = %d",
                    gate_ld, bias_ld, C);
        const dim3 grid(grid_for(HW * (C / VEC), 256, 1024), F);
        hipLaunchKernelGGL(channel_gate_kernel<E>, grid, dim3(256), 0, stream, (const E*)x, x_ld, gate, gate_ld, gate_is_logit, add_x,
                           bias, bias_ld, (const E*)a, a_ld, (int)HW, C, (E*)y, y_ld);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}

extern "C" int flair_upsample_argmax_nhwc(const void* logits, int dtype, int ld, int F, int h, int w, int N, int H, int W,
                                          const float* table, int D, int* idx, float* y, int y_ld, hipStream_t stream) {
    FLAIR_CHECK(logits && (idx || y), "flair_upsample_argmax_nhwc: null argument");
    FLAIR_CHECK(F > 0 && F <= 65535 && h > 0 && w > 0 && H > 0 && W > 0 && (H + UA_ROWS - 1) / UA_ROWS <= 65535,
                "flair_upsample_argmax_nhwc: bad shape F=%d h=%d w=%d H=%d W=%d", F, h, w, H, W);
    FLAIR_CHECK(N >= 1 && N <= 32, "flair_upsample_argmax_nhwc: N = %d classes (1 .. 32)", N);
    FLAIR_CHECK(ld >= N, "flair_upsample_argmax_nhwc: ld = %d below N = %d", ld, N);
    FLAIR_CHECK(!y || (table && D > 0 && y_ld >= D), "flair_upsample_argmax_nhwc: y needs a table, D = %d > 0 and y_ld = %d >= D",
                D, y_ld);
    return flair_by_dtype("flair_upsample_argmax_nhwc", dtype, [&](auto e) -> int {
        using E = decltype(e);
        constexpr int VEC = ET<E>::VEC;
        const int np = (N + 7) / 8 * 8;
        // 16-byte loads when every pixel's class vector starts on a 16-byte boundary and its last chunk stays inside the
        // pixel stride; element loads otherwise (same arithmetic)
        int nload = (N + VEC - 1) / VEC * VEC;
        if (!(ld % VEC == 0 && nload <= ld && aligned16(logits))) nload = 0;
        const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
        const float sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
        const dim3 grid(cdiv(W, 256), cdiv(H, UA_ROWS), F);
        const int rc = launch_upsample_argmax<E>(np, grid, stream, (const E*)logits, ld, h, w, N, nload, H, W, sy, sx, table, D, idx,
                                                 y, y_ld);
        FLAIR_CHECK(rc == 0, "flair_upsample_argmax_nhwc: no kernel for %d classes", N);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}
