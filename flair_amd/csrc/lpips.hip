// LPIPS, the evaluation-only kernels: flair_lpips_prepare, flair_lpips_tap, flair_maxpool_valid_s2_nhwc, flair_alexnet_stem
// (include/flair_eval.h, which holds the definition and every entry's contract).  The trunks' 3x3 / 5x5 convolutions are
// flair_conv_nhwc's; f32 only.
//
//   prepare   16 lanes own one item of a frame set's pixel stream: the head (pixels before the first one whose 3 bytes start
//             on a dword), four pixels in three aligned dwords, or the tail.  Lane 4 k of an item reads pixel k (two aligned
//             dwords and a funnel shift, or three bytes) and maps each byte with one double fma; lanes 4 k + 1 .. 4 k + 3
//             write the pixel's zero channels, so a wave stores 16 pixels x 64 bytes in one piece.
//   tap       LANES lanes hold the C / 4 float4 of a pixel of both frames in registers (V float4 each): sums of squares
//             (xor butterfly: every lane ends with the same bits), quotients, weighted squared difference into a per-lane
//             double.  256 / LANES pixels per workgroup and step, two steps' loads in flight.  One partial per workgroup,
//             a second launch adds a frame's FLAIR_LPIPS_TAP_PARTS partials in a fixed order: no floating-point atomics.
//   pool      one float4 of one output pixel per thread.
//   stem      see the entry.
#include "common.h"

#include "../../include/flair_eval.h"

namespace {
constexpr int LP_THREADS = 256;
constexpr int LP_PARTS = FLAIR_LPIPS_TAP_PARTS;
static_assert(LP_PARTS % LP_THREADS == 0, "the sum kernel's thread i adds partials i, i + 256, ...");

// ---- prepare ------------------------------------------------------------------------------------------------------------
// ((2 v / 255 - 1) - shift) / scale = A v + B in double
constexpr double LP_SHIFT[3] = {-0.030, -0.088, -0.188}, LP_SCALE[3] = {0.458, 0.448, 0.450};
constexpr double LP_A0 = 2.0 / (255.0 * LP_SCALE[0]), LP_A1 = 2.0 / (255.0 * LP_SCALE[1]), LP_A2 = 2.0 / (255.0 * LP_SCALE[2]);
constexpr double LP_B0 = -(1.0 + LP_SHIFT[0]) / LP_SCALE[0], LP_B1 = -(1.0 + LP_SHIFT[1]) / LP_SCALE[1],
                 LP_B2 = -(1.0 + LP_SHIFT[2]) / LP_SCALE[2];
constexpr int LP_ITEM_LANES = 16, LP_ITEMS = LP_THREADS / LP_ITEM_LANES;

__global__ __launch_bounds__(LP_THREADS) void lpips_prepare_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                    long P, float* __restrict__ y, int y_ld) {
    const int tid = threadIdx.x;
    const int set = blockIdx.y;
    const uint8_t* src = set ? b : a;
    const int c = (int)(reinterpret_cast<uintptr_t>(src) & 3u);      // pixel c is the first whose bytes start on a dword
    const long item = (long)blockIdx.x * LP_ITEMS + tid / LP_ITEM_LANES;
    const int k = (tid % LP_ITEM_LANES) >> 2, q = tid & 3;
    const long first = item == 0 ? 0 : c + 4 * (item - 1);
    const long count = item == 0 ? (c < P ? c : P) : (P - first < 4 ? P - first : 4);       // <= 0 past the end
    if (k >= count) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q == 0) {
        unsigned r, g, bl;
        if (item != 0 && count == 4) {
            const uint32_t* d = reinterpret_cast<const uint32_t*>(src + 3 * first);         // dword aligned (see above)
            const int bo = 3 * k;
            const uint32_t w0 = d[bo >> 2], w1 = d[(bo + 2) >> 2];
            const unsigned long long both = (((unsigned long long)w1 << 32) | w0) >> (8 * (bo & 3));
            r = (unsigned)both & 0xffu;
            g = (unsigned)(both >> 8) & 0xffu;
            bl = (unsigned)(both >> 16) & 0xffu;
        } else {
            const uint8_t* e = src + 3 * (first + k);
            r = e[0];
            g = e[1];
            bl = e[2];
        }
        v.x = (float)fma(LP_A0, (double)r, LP_B0);
        v.y = (float)fma(LP_A1, (double)g, LP_B1);
        v.z = (float)fma(LP_A2, (double)bl, LP_B2);
    }
    *reinterpret_cast<float4*>(y + ((size_t)set * (size_t)P + (size_t)(first + k)) * (size_t)y_ld + 4 * q) = v;
}

// ---- tap ----------------------------------------------------------------------------------------------------------------
template <int LANES>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, FLAIR_WAVE);
    return v;
}

template <int LANES, int V>
struct TapPixel {
    float4 a[V], b[V];
    __device__ __forceinline__ void load(const float* __restrict__ pa, const float* __restrict__ pb, int sub) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            a[v] = *reinterpret_cast<const float4*>(pa + 4 * (sub + LANES * v));
            b[v] = *reinterpret_cast<const float4*>(pb + 4 * (sub + LANES * v));
        }
    }
    // this lane's part of d = sum_c w_c (a_c / (|a| + eps) - b_c / (|b| + eps))^2
    __device__ __forceinline__ float distance(const float4 (&w)[V]) const {
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            sa = fmaf(a[v].x, a[v].x, sa); sa = fmaf(a[v].y, a[v].y, sa); sa = fmaf(a[v].z, a[v].z, sa); sa = fmaf(a[v].w, a[v].w, sa);
            sb = fmaf(b[v].x, b[v].x, sb); sb = fmaf(b[v].y, b[v].y, sb); sb = fmaf(b[v].z, b[v].z, sb); sb = fmaf(b[v].w, b[v].w, sb);
        }
        const float da = sqrtf(group_sum<LANES>(sa)) + 1e-10f, db = sqrtf(group_sum<LANES>(sb)) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float ex = a[v].x / da - b[v].x / db, ey = a[v].y / da - b[v].y / db;
            const float ez = a[v].z / da - b[v].z / db, ew = a[v].w / da - b[v].w / db;
            d = fmaf(w[v].x, ex * ex, d);
            d = fmaf(w[v].y, ey * ey, d);
            d = fmaf(w[v].z, ez * ez, d);
            d = fmaf(w[v].w, ew * ew, d);
        }
        return d;
    }
};

template <int LANES, int V>
__global__ __launch_bounds__(LP_THREADS) void lpips_tap_kernel(const float* __restrict__ fa, int fa_ld, const float* __restrict__ fb,
                                                                int fb_ld, long HW, const float* __restrict__ w,
                                                                double* __restrict__ ws) {
    constexpr int SLOTS = LP_THREADS / LANES;              // pixels per workgroup and step
    __shared__ double red[LP_THREADS / FLAIR_WAVE];
    const int tid = threadIdx.x;
    const int sub = tid % LANES, slot = tid / LANES;
    const size_t f = blockIdx.x / (unsigned)LP_PARTS;
    const long part = blockIdx.x % (unsigned)LP_PARTS;
    const long chunk = (HW + LP_PARTS - 1) / LP_PARTS;
    const long p0 = part * chunk, p1 = p0 + chunk < HW ? p0 + chunk : HW;      // this workgroup's pixels (none when p0 >= HW)

    float4 wv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) wv[v] = *reinterpret_cast<const float4*>(w + 4 * (sub + LANES * v));
    const float* base_a = fa + f * (size_t)HW * (size_t)fa_ld;
    const float* base_b = fb + f * (size_t)HW * (size_t)fb_ld;

    // The loop is uniform over the workgroup (the butterflies need whole groups); a slot past the end re-reads the run's last
    // pixel and adds nothing.
    double acc = 0.0;
    for (long s = p0; s < p1; s += 2 * SLOTS) {
        const long q0 = s + slot, q1 = s + SLOTS + slot;
        const long r0 = q0 < p1 ? q0 : p1 - 1, r1 = q1 < p1 ? q1 : p1 - 1;
        TapPixel<LANES, V> x0, x1;
        x0.load(base_a + (size_t)r0 * (size_t)fa_ld, base_b + (size_t)r0 * (size_t)fb_ld, sub);
        x1.load(base_a + (size_t)r1 * (size_t)fa_ld, base_b + (size_t)r1 * (size_t)fb_ld, sub);
        const float d0 = x0.distance(wv), d1 = x1.distance(wv);
        acc += q0 < p1 ? (double)d0 : 0.0;
        acc += q1 < p1 ? (double)d1 : 0.0;
    }

#pragma unroll
    for (int off = FLAIR_WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, FLAIR_WAVE);
    if ((tid & (FLAIR_WAVE - 1)) == 0) red[tid / FLAIR_WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = red[0];
#pragma unroll
        for (int i = 1; i < LP_THREADS / FLAIR_WAVE; ++i) t += red[i];
        ws[blockIdx.x] = t;
    }
}

// acc[f] += (partials of frame f, thread i adding i, i + 256, ... in that order, then a fixed tree) / HW
__global__ __launch_bounds__(LP_THREADS) void lpips_tap_sum_kernel(const double* __restrict__ ws, long HW, double* __restrict__ acc) {
    __shared__ double sh[LP_THREADS];
    const int tid = threadIdx.x;
    const double* p = ws + (size_t)blockIdx.x * LP_PARTS;
    double s = 0.0;
    for (int i = tid; i < LP_PARTS; i += LP_THREADS) s += p[i];
    sh[tid] = s;
    for (int off = LP_THREADS / 2; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off) sh[tid] += sh[tid + off];
    }
    __syncthreads();
    if (tid == 0) acc[blockIdx.x] += sh[0] / (double)HW;
}

// ---- valid max pool -----------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(LP_THREADS) void maxpool_valid_kernel(const float* __restrict__ x, int x_ld, int H, int W, int C4,
                                                                    int Ho, int Wo, long n, float* __restrict__ y, int y_ld) {
    const long i = (long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= n) return;
    const int c4 = (int)(i % C4);
    long r = i / C4;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho);
    const size_t f = (size_t)(r / Ho);
    const float* px = x + ((f * (size_t)H + (size_t)(2 * oy)) * (size_t)W + (size_t)(2 * ox)) * (size_t)x_ld + 4 * c4;
    float4 m = *reinterpret_cast<const float4*>(px);
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const float4 v = *reinterpret_cast<const float4*>(px + ((size_t)dy * (size_t)W + (size_t)dx) * (size_t)x_ld);
            m.x = fmaxf(m.x, v.x);
            m.y = fmaxf(m.y, v.y);
            m.z = fmaxf(m.z, v.z);
            m.w = fmaxf(m.w, v.w);
        }
    *reinterpret_cast<float4*>(y + ((f * (size_t)Ho + (size_t)oy) * (size_t)Wo + (size_t)ox) * (size_t)y_ld + 4 * c4) = m;
}

// ---- AlexNet's stem -----------------------------------------------------------------------------------------------------
constexpr int ST_K = 11, ST_S = 4, ST_PAD = 2, ST_COUT = 64;
constexpr int ST_TILE = 8;                                           // 8 x 8 output pixels: one per lane
constexpr int ST_PATCH = (ST_TILE - 1) * ST_S + ST_K;                // 39 input rows / columns
constexpr int ST_CPW = ST_COUT / (LP_THREADS / FLAIR_WAVE);          // 16 output channels per wave
static_assert(ST_TILE * ST_TILE == FLAIR_WAVE && ST_CPW % 4 == 0, "lane = output pixel, float4 stores");

__global__ __launch_bounds__(LP_THREADS) void alexnet_stem_kernel(const float* __restrict__ x, int x_ld, int H, int W,
                                                                   const float* __restrict__ w, const float* __restrict__ bias,
                                                                   int Ho, int Wo, int tilesX, int tiles, float* __restrict__ y,
                                                                   int y_ld) {
    __shared__ float patch[ST_PATCH * ST_PATCH * 3];
    const int tid = threadIdx.x;
    const int t = (int)(blockIdx.x % (unsigned)tiles);
    const size_t f = blockIdx.x / (unsigned)tiles;
    const int ty = t / tilesX, tx = t - ty * tilesX;
    const int iy0 = ty * ST_TILE * ST_S - ST_PAD, ix0 = tx * ST_TILE * ST_S - ST_PAD;
    for (int e = tid; e < ST_PATCH * ST_PATCH * 3; e += LP_THREADS) {
        const int r = e / (ST_PATCH * 3), rem = e - r * (ST_PATCH * 3);
        const int col = rem / 3, c = rem - col * 3;
        const int gy = iy0 + r, gx = ix0 + col;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = x[((f * (size_t)H + (size_t)gy) * (size_t)W + (size_t)gx) * (size_t)x_ld + c];
        patch[e] = v;
    }
    __syncthreads();

    const int lane = tid & (FLAIR_WAVE - 1);
    const int co0 = __builtin_amdgcn_readfirstlane(tid / FLAIR_WAVE) * ST_CPW;
    const int ly = lane / ST_TILE, lx = lane % ST_TILE;
    float acc[ST_CPW];
#pragma unroll
    for (int j = 0; j < ST_CPW; ++j) acc[j] = bias[co0 + j];
    const float* pin = patch + (ly * ST_S * ST_PATCH + lx * ST_S) * 3;
    for (int ky = 0; ky < ST_K; ++ky)
        for (int kx = 0; kx < ST_K; ++kx) {
            const float* pv = pin + (ky * ST_PATCH + kx) * 3;
            const float* pw = w + (size_t)((ky * ST_K + kx) * 3) * ST_COUT + co0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = pv[c];
#pragma unroll
                for (int j = 0; j < ST_CPW; ++j) acc[j] = fmaf(v, pw[c * ST_COUT + j], acc[j]);
            }
        }
    const int oy = ty * ST_TILE + ly, ox = tx * ST_TILE + lx;
    if (oy < Ho && ox < Wo) {
        float* py = y + ((f * (size_t)Ho + (size_t)oy) * (size_t)Wo + (size_t)ox) * (size_t)y_ld + co0;
#pragma unroll
        for (int j = 0; j < ST_CPW; j += 4)
            *reinterpret_cast<float4*>(py + j) = make_float4(fmaxf(acc[j], 0.f), fmaxf(acc[j + 1], 0.f), fmaxf(acc[j + 2], 0.f),
                                                             fmaxf(acc[j + 3], 0.f));
    }
}

template <int LANES, int V>
void launch_tap(unsigned groups, hipStream_t stream, const float* fa, int fa_ld, const float* fb, int fb_ld, long HW, const float* w,
                double* ws) {
    static_assert(LANES * V * 4 >= 64 && LP_THREADS % LANES == 0 && LANES <= FLAIR_WAVE, "a pixel's float4 over LANES lanes");
    hipLaunchKernelGGL((lpips_tap_kernel<LANES, V>), dim3(groups), dim3(LP_THREADS), 0, stream, fa, fa_ld, fb, fb_ld, HW, w, ws);
}
}  // namespace

extern "C" int flair_lpips_prepare(const uint8_t* a, const uint8_t* b, int N, int H, int W, float* y, int y_ld, hipStream_t stream) {
    FLAIR_CHECK(a && b && y, "flair_lpips_prepare: null pointer (a = %p, b = %p, y = %p)", (const void*)a, (const void*)b, (const void*)y);
    FLAIR_CHECK(N >= 1 && H >= 1 && W >= 1, "flair_lpips_prepare: N = %d, H = %d, W = %d must be positive", N, H, W);
    FLAIR_CHECK_VIEW("flair_lpips_prepare", "y", y, y_ld, 16, 4);
    const long P = (long)N * H * W;
    const long groups = cdiv(1 + (P + 3) / 4, LP_ITEMS);             // the head and at most ceil(P / 4) pieces per set
    FLAIR_CHECK(1 + (P + 3) / 4 <= 0x7fffffffL * (long)LP_ITEMS, "flair_lpips_prepare: %ld pixels per set (N = %d, %dx%d) exceed one launch",
                P, N, H, W);
    hipLaunchKernelGGL(lpips_prepare_kernel, dim3((unsigned)groups, 2), dim3(LP_THREADS), 0, stream, a, b, P, y, y_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_lpips_tap(const float* fa, int fa_ld, const float* fb, int fb_ld, int F, long HW, int C, const float* w,
                               double* acc, void* ws, size_t ws_bytes, hipStream_t stream) {
    FLAIR_CHECK(fa && fb && w && acc && ws, "flair_lpips_tap: null pointer (fa = %p, fb = %p, w = %p, acc = %p, ws = %p)",
                (const void*)fa, (const void*)fb, (const void*)w, (const void*)acc, ws);
    FLAIR_CHECK(F >= 1, "flair_lpips_tap: F = %d frames, need at least one", F);
    FLAIR_CHECK(HW >= 1, "flair_lpips_tap: HW = %ld pixels, need at least one", HW);
    FLAIR_CHECK(C == 64 || C == 128 || C == 192 || C == 256 || C == 384 || C == 512,
                "flair_lpips_tap: C = %d is not a tap width of VGG-16 or AlexNet (64, 128, 192, 256, 384, 512)", C);
    FLAIR_CHECK_VIEW("flair_lpips_tap", "fa", fa, fa_ld, C, 4);
    FLAIR_CHECK_VIEW("flair_lpips_tap", "fb", fb, fb_ld, C, 4);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(w) % 16 == 0, "flair_lpips_tap: w = %p must be 16-byte aligned", (const void*)w);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(acc) % 8 == 0 && reinterpret_cast<uintptr_t>(ws) % 8 == 0,
                "flair_lpips_tap: acc = %p and ws = %p hold doubles and must be 8-byte aligned", (const void*)acc, ws);
    const long groups = (long)F * LP_PARTS;
    FLAIR_CHECK(groups <= 0x7fffffffL, "flair_lpips_tap: %ld workgroups (F = %d) exceed one launch", groups, F);
    const size_t need = (size_t)groups * sizeof(double);
    FLAIR_CHECK(ws_bytes >= need, "flair_lpips_tap: ws_bytes = %zu, F * FLAIR_LPIPS_TAP_PARTS * 8 = %zu", ws_bytes, need);
    double* part = reinterpret_cast<double*>(ws);
    switch (C) {
        case 64: launch_tap<16, 1>((unsigned)groups, stream, fa, fa_ld, fb, fb_ld, HW, w, part); break;
        case 128: launch_tap<32, 1>((unsigned)groups, stream, fa, fa_ld, fb, fb_ld, HW, w, part); break;
        case 192: launch_tap<16, 3>((unsigned)groups, stream, fa, fa_ld, fb, fb_ld, HW, w, part); break;
        case 256: launch_tap<64, 1>((unsigned)groups, stream, fa, fa_ld, fb, fb_ld, HW, w, part); break;
        case 384: launch_tap<32, 3>((unsigned)groups, stream, fa, fa_ld, fb, fb_ld, HW, w, part); break;
        default: launch_tap<64, 2>((unsigned)groups, stream, fa, fa_ld, fb, fb_ld, HW, w, part); break;
    }
    FLAIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(lpips_tap_sum_kernel, dim3((unsigned)F), dim3(LP_THREADS), 0, stream, part, HW, acc);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_maxpool_valid_s2_nhwc(const float* x, int x_ld, int F, int H, int W, int C, int k, float* y, int y_ld,
                                           hipStream_t stream) {
    FLAIR_CHECK(x && y, "flair_maxpool_valid_s2_nhwc: x / y is null");
    FLAIR_CHECK(F >= 1, "flair_maxpool_valid_s2_nhwc: F = %d frames, need at least one", F);
    FLAIR_CHECK(k == 2 || k == 3, "flair_maxpool_valid_s2_nhwc: k = %d, the window is 2 or 3 pixels wide", k);
    FLAIR_CHECK(H >= k && W >= k, "flair_maxpool_valid_s2_nhwc: frames of %dx%d hold no %dx%d window", H, W, k, k);
    FLAIR_CHECK(C > 0 && C % 4 == 0, "flair_maxpool_valid_s2_nhwc: C = %d is not a positive multiple of 4", C);
    FLAIR_CHECK_VIEW("flair_maxpool_valid_s2_nhwc", "x", x, x_ld, C, 4);
    FLAIR_CHECK_VIEW("flair_maxpool_valid_s2_nhwc", "y", y, y_ld, C, 4);
    const int Ho = (H - k) / 2 + 1, Wo = (W - k) / 2 + 1;
    const long n = (long)F * Ho * Wo * (C / 4);
    FLAIR_CHECK(n <= 0x7fffffffL * (long)LP_THREADS, "flair_maxpool_valid_s2_nhwc: %ld items (F = %d, %dx%d, C = %d) exceed one launch", n,
                F, H, W, C);
    const dim3 grid((unsigned)grid_for(n, LP_THREADS, GRID_NO_CAP));
    if (k == 2)
        hipLaunchKernelGGL(maxpool_valid_kernel<2>, grid, dim3(LP_THREADS), 0, stream, x, x_ld, H, W, C / 4, Ho, Wo, n, y, y_ld);
    else
        hipLaunchKernelGGL(maxpool_valid_kernel<3>, grid, dim3(LP_THREADS), 0, stream, x, x_ld, H, W, C / 4, Ho, Wo, n, y, y_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_alexnet_stem(const float* x, int x_ld, int F, int H, int W, const float* w, const float* bias, float* y,
                                  int y_ld, hipStream_t stream) {
    FLAIR_CHECK(x && w && bias && y, "flair_alexnet_stem: null pointer (x = %p, w = %p, bias = %p, y = %p)", (const void*)x,
                (const void*)w, (const void*)bias, (const void*)y);
    FLAIR_CHECK(F >= 1, "flair_alexnet_stem: F = %d frames, need at least one", F);
    FLAIR_CHECK(H >= ST_K - 2 * ST_PAD && W >= ST_K - 2 * ST_PAD, "flair_alexnet_stem: frames of %dx%d are smaller than the 11x11 kernel less its padding of 2",
                H, W);
    FLAIR_CHECK(x_ld >= 3, "flair_alexnet_stem: x_ld = %d must hold the 3 channels", x_ld);
    FLAIR_CHECK_VIEW("flair_alexnet_stem", "y", y, y_ld, ST_COUT, 4);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(w) % 16 == 0 && reinterpret_cast<uintptr_t>(bias) % 16 == 0,
                "flair_alexnet_stem: w = %p and bias = %p must be 16-byte aligned", (const void*)w, (const void*)bias);
    const int Ho = (H + 2 * ST_PAD - ST_K) / ST_S + 1, Wo = (W + 2 * ST_PAD - ST_K) / ST_S + 1;
    const long tilesX = cdiv(Wo, ST_TILE), tiles = tilesX * cdiv(Ho, ST_TILE);
    const long groups = (long)F * tiles;
    FLAIR_CHECK(groups <= 0x7fffffffL, "flair_alexnet_stem: %ld workgroups (F = %d, %dx%d) exceed one launch", groups, F, H, W);
    hipLaunchKernelGGL(alexnet_stem_kernel, dim3((unsigned)groups), dim3(LP_THREADS), 0, stream, x, x_ld, H, W, w, bias, Ho, Wo,
                       (int)tilesX, (int)tiles, y, y_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
