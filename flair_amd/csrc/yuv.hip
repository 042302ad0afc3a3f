// The video streams' colour conversion and chroma resampling: flair_yuv_to_rgb_u8 and flair_rgb_to_yuv_u8 (include/flair_yuv.h,
// which holds the definition, the coefficient table and the entries' contracts).  The bytes of .y4m frames in, RGB bytes out, and
// back; integers throughout, every value rounded once.
//
//   one thread per 4 x 2 luma pixels, lanes along x, a workgroup owns 16 rows of 128 pixels of one frame.  The two luma rows
//   that share a chroma row sit in one thread; the chroma bytes that neighbouring threads share (the taps of the centred and
//   co-sited filters reach one sample to either side) meet in the cache, so every byte comes from HBM once.  Payloads start at
//   any byte (a frame is W H + 2 wc hc bytes after a text header), so four bytes move as one word where the address allows
//   and byte by byte where not; lanes stay consecutive along x either way.  No LDS, no atomics; the format is a template
//   argument, so a thread's chroma patch lives in registers under constant indices.
#include "common.h"

#include "../../include/flair_yuv.h"

namespace {
constexpr int YT_TX = 32, YT_TY = 8, YT_THREADS = YT_TX * YT_TY;       // threads of a workgroup along x and y
constexpr int YT_W = YT_TX * 4, YT_H = YT_TY * 2;                     // its pixels

enum { AX_FULL = 0, AX_CENTRED = 1, AX_COSITED = 2 };                  // how an axis of the chroma planes is sampled

struct Coef {
    int cy, crv, cgu, cgv, cbu;
    int ey[3], eu[3], ev[3];
    int y0, lo, hiY, hiC;
};

// round(x 65536) of the float64 coefficients of include/flair_yuv.h, rows bt601 limited, bt601 full, bt709 limited, bt709 full
// (tests/test_y4m_cpu.py derives them again from Kr and Kb and compares with this table and the header's).
const int YUV_TAB[4][14] = {
    {76309, 104597, 25675, 53279, 132201, 16829, 33039, 6416, -9714, -19071, 28784, 28784, -24103, -4681},
    {65536, 91881, 22553, 46802, 116130, 19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329},
    {76309, 117489, 13975, 34925, 138438, 11966, 40254, 4064, -6596, -22189, 28784, 28784, -26145, -2639},
    {65536, 103206, 12276, 30679, 121609, 13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005},
};

Coef coef_of(int matrix, int range) {
    const int* t = YUV_TAB[matrix * 2 + range];
    Coef k;
    k.cy = t[0], k.crv = t[1], k.cgu = t[2], k.cgv = t[3], k.cbu = t[4];
    for (int i = 0; i < 3; ++i) k.ey[i] = t[5 + i], k.eu[i] = t[8 + i], k.ev[i] = t[11 + i];
    const bool full = range == FLAIR_YUV_FULL;
    k.y0 = full ? 0 : 16, k.lo = full ? 0 : 16, k.hiY = full ? 255 : 235, k.hiC = full ? 255 : 240;
    return k;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// four consecutive bytes, `valid` (1..4) of which exist: one word where all four do and the address allows
__device__ __forceinline__ void load4(const uint8_t* p, int valid, int (&v)[4]) {
    if (valid == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
        v[0] = w & 255, v[1] = (w >> 8) & 255, v[2] = (w >> 16) & 255, v[3] = w >> 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < valid ? (int)p[j] : 0;
    }
}
__device__ __forceinline__ void store4(uint8_t* p, int valid, const int (&v)[4]) {
    if (valid == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < valid) p[j] = (uint8_t)v[j];
    }
}

// The two taps of one axis (flair_yuv.h, Decode) over a patch line p whose entry 0 is chroma sample base - 1 (base = the chroma
// index of the thread's first luma sample; entry 0 is that sample itself on a full axis).  j: the luma sample within the
// thread, a constant after unrolling.  Weights in quarters.
template <int M>
__device__ __forceinline__ int axis_taps(const int* p, int j) {
    if constexpr (M == AX_FULL) return 4 * p[j];
    const int c = (j >> 1) + 1;
    if constexpr (M == AX_CENTRED) return 3 * p[c] + p[(j & 1) ? c + 1 : c - 1];
    return (j & 1) ? 2 * p[c] + 2 * p[c + 1] : 4 * p[c];
}

__device__ __forceinline__ void block_of(int tilesX, int tilesY, size_t& n, int& x0, int& y0) {
    const unsigned tx = blockIdx.x % (unsigned)tilesX, rest = blockIdx.x / (unsigned)tilesX;
    const unsigned ty = rest % (unsigned)tilesY;
    n = rest / (unsigned)tilesY;
    x0 = ((int)tx * YT_TX + (int)(threadIdx.x % YT_TX)) * 4;
    y0 = ((int)ty * YT_TY + (int)(threadIdx.x / YT_TX)) * 2;
}

// block = (frame, row group, column group), column groups fastest
template <int HM, int VM, bool MONO, bool PLANAR>
__global__ __launch_bounds__(YT_THREADS) void yuv_to_rgb_kernel(const uint8_t* __restrict__ payload, int H, int W, int wc, int hc, size_t P,
                                                                int tilesX, int tilesY, Coef k, uint8_t* __restrict__ out) {
    size_t n;
    int x0, y0;
    block_of(tilesX, tilesY, n, x0, y0);
    if (x0 >= W || y0 >= H) return;
    const int nx = W - x0 < 4 ? W - x0 : 4, ny = H - y0 < 2 ? H - y0 : 2;
    const uint8_t* Yp = payload + n * P;

    // U16 - 2048 and V16 - 2048 of the thread's 2 x 4 pixels
    int u[2][4], v[2][4];
    if constexpr (MONO) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) u[i][j] = v[i][j] = 0;
    } else {
        constexpr int PR = VM == AX_FULL ? 2 : 3;
        const uint8_t* Up = Yp + (size_t)H * (size_t)W;
        const uint8_t* Vp = Up + (size_t)wc * (size_t)hc;
        const int rb = VM == AX_FULL ? y0 : (y0 >> 1) - 1, cb = HM == AX_FULL ? x0 : (x0 >> 1) - 1;
        int hu[PR][4], hv[PR][4];                                   // the patch's rows after the horizontal taps
#pragma unroll
        for (int r = 0; r < PR; ++r) {
            const size_t row = (size_t)clampi(rb + r, 0, hc - 1) * (size_t)wc;       // the clamps of the taps: indices stay in the plane
            int pu[4], pv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const size_t o = row + (size_t)clampi(cb + c, 0, wc - 1);
                pu[c] = Up[o], pv[c] = Vp[o];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) hu[r][j] = axis_taps<HM>(pu, j), hv[r][j] = axis_taps<HM>(pv, j);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int cu[PR], cv[PR];
#pragma unroll
            for (int r = 0; r < PR; ++r) cu[r] = hu[r][j], cv[r] = hv[r][j];
#pragma unroll
            for (int i = 0; i < 2; ++i) u[i][j] = axis_taps<VM>(cu, i) - 2048, v[i][j] = axis_taps<VM>(cv, i) - 2048;
        }
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (i >= ny) break;
        const size_t y = (size_t)(y0 + i);
        int Y[4], R[4], G[4], B[4];
        load4(Yp + y * (size_t)W + (size_t)x0, nx, Y);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = k.cy * 16 * (Y[j] - k.y0);
            R[j] = clampi((yy + k.crv * v[i][j] + (1 << 19)) >> 20, 0, 255);
            G[j] = clampi((yy - k.cgu * u[i][j] - k.cgv * v[i][j] + (1 << 19)) >> 20, 0, 255);
            B[j] = clampi((yy + k.cbu * u[i][j] + (1 << 19)) >> 20, 0, 255);
        }
        if constexpr (PLANAR) {
            const size_t HW = (size_t)H * (size_t)W;
            uint8_t* o = out + n * 3 * HW + y * (size_t)W + (size_t)x0;
            store4(o, nx, R);
            store4(o + HW, nx, G);
            store4(o + 2 * HW, nx, B);
        } else {
            uint8_t* o = out + ((n * (size_t)H + y) * (size_t)W + (size_t)x0) * 3;
            const int a[4] = {R[0], G[0], B[0], R[1]}, b[4] = {G[1], B[1], R[2], G[2]}, c[4] = {B[2], R[3], G[3], B[3]};
            if (nx == 4) {
                store4(o, 4, a);
                store4(o + 4, 4, b);
                store4(o + 8, 4, c);
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j < nx) o[3 * j] = (uint8_t)R[j], o[3 * j + 1] = (uint8_t)G[j], o[3 * j + 2] = (uint8_t)B[j];
            }
        }
    }
}

template <int HM, int VM, bool MONO>
__global__ __launch_bounds__(YT_THREADS) void rgb_to_yuv_kernel(const uint8_t* __restrict__ rgb, int H, int W, int wc, int hc, size_t P, int tilesX,
                                                                int tilesY, Coef k, uint8_t* __restrict__ payload) {
    size_t n;
    int x0, y0;
    block_of(tilesX, tilesY, n, x0, y0);
    if (x0 >= W || y0 >= H) return;
    const int nx = W - x0 < 4 ? W - x0 : 4, ny = H - y0 < 2 ? H - y0 : 2;
    uint8_t* Yp = payload + n * P;

    // the thread's 2 x 4 pixels and the one to their left, coordinates clamped to the frame (the footprints' edge rule);
    // entry jj is luma x0 + jj - 1
    int cu[2][5], cv[2][5];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const size_t y = (size_t)(y0 + i < H ? y0 + i : H - 1);
        const uint8_t* row = rgb + (n * (size_t)H + y) * (size_t)W * 3;
        int p[5][3];
        if (nx == 4) {
            int a[4], b[4], c[4];
            const uint8_t* q = row + (size_t)x0 * 3;
            load4(q, 4, a);
            load4(q + 4, 4, b);
            load4(q + 8, 4, c);
            p[1][0] = a[0], p[1][1] = a[1], p[1][2] = a[2], p[2][0] = a[3], p[2][1] = b[0], p[2][2] = b[1];
            p[3][0] = b[2], p[3][1] = b[3], p[3][2] = c[0], p[4][0] = c[1], p[4][1] = c[2], p[4][2] = c[3];
        } else {
#pragma unroll
            for (int jj = 1; jj < 5; ++jj) {
                const uint8_t* q = row + (size_t)(x0 + jj - 1 < W ? x0 + jj - 1 : W - 1) * 3;
                p[jj][0] = q[0], p[jj][1] = q[1], p[jj][2] = q[2];
            }
        }
        if constexpr (HM == AX_COSITED) {
            const uint8_t* q = row + (size_t)(x0 > 0 ? x0 - 1 : 0) * 3;
            p[0][0] = q[0], p[0][1] = q[1], p[0][2] = q[2];
        } else {
            p[0][0] = p[0][1] = p[0][2] = 0;
        }
        int Y[4];
#pragma unroll
        for (int jj = 0; jj < 5; ++jj) {
            cu[i][jj] = k.eu[0] * p[jj][0] + k.eu[1] * p[jj][1] + k.eu[2] * p[jj][2];
            cv[i][jj] = k.ev[0] * p[jj][0] + k.ev[1] * p[jj][1] + k.ev[2] * p[jj][2];
            if (jj > 0) Y[jj - 1] = clampi(((k.ey[0] * p[jj][0] + k.ey[1] * p[jj][1] + k.ey[2] * p[jj][2] + (1 << 15)) >> 16) + k.y0, k.lo, k.hiY);
        }
        if (i < ny) store4(Yp + y * (size_t)W + (size_t)x0, nx, Y);
    }
    if constexpr (MONO) return;

    constexpr int NC = HM == AX_FULL ? 4 : 2, NR = VM == AX_FULL ? 2 : 1;
    constexpr int SHIFT = (HM == AX_CENTRED ? 1 : (HM == AX_COSITED ? 2 : 0)) + (VM == AX_CENTRED ? 1 : 0);
    uint8_t* Up = Yp + (size_t)H * (size_t)W;
    uint8_t* Vp = Up + (size_t)wc * (size_t)hc;
    const int ccb = HM == AX_FULL ? x0 : x0 >> 1, ncx = wc - ccb < NC ? wc - ccb : NC;
    int su[2][4], sv[2][4];                                         // per luma row, the horizontal footprints
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            if constexpr (HM == AX_FULL) su[i][m] = cu[i][m + 1], sv[i][m] = cv[i][m + 1];
            if constexpr (HM == AX_CENTRED) su[i][m] = cu[i][2 * m + 1] + cu[i][2 * m + 2], sv[i][m] = cv[i][2 * m + 1] + cv[i][2 * m + 2];
            if constexpr (HM == AX_COSITED) {
                su[i][m] = cu[i][2 * m] + 2 * cu[i][2 * m + 1] + cu[i][2 * m + 2];
                sv[i][m] = cv[i][2 * m] + 2 * cv[i][2 * m + 1] + cv[i][2 * m + 2];
            }
        }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int crow = VM == AX_FULL ? y0 + r : y0 >> 1;
        if (crow >= hc) break;
        int U[4] = {0, 0, 0, 0}, V[4] = {0, 0, 0, 0};
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            const int a = VM == AX_FULL ? su[r][m] : su[0][m] + su[1][m], b = VM == AX_FULL ? sv[r][m] : sv[0][m] + sv[1][m];
            U[m] = clampi(((a + (1 << (15 + SHIFT))) >> (16 + SHIFT)) + 128, k.lo, k.hiC);
            V[m] = clampi(((b + (1 << (15 + SHIFT))) >> (16 + SHIFT)) + 128, k.lo, k.hiC);
        }
        const size_t o = (size_t)crow * (size_t)wc + (size_t)ccb;
        if constexpr (NC == 4) {
            store4(Up + o, ncx, U);
            store4(Vp + o, ncx, V);
        } else {
#pragma unroll
            for (int m = 0; m < NC; ++m)
                if (m < ncx) Up[o + m] = (uint8_t)U[m], Vp[o + m] = (uint8_t)V[m];
        }
    }
}

bool overlaps(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}

struct Plan {
    int wc, hc, tilesX, tilesY;
    size_t P, payload_bytes, rgb_bytes;
    unsigned grid;
    Coef k;
};

// The refusals both entries share, and the sizes they launch with.  `in` and `out`: the entry's input and output.
int plan_of(const char* fn, const void* in, const char* in_name, const void* out, const char* out_name, bool in_is_payload, int N, int H, int W, int format,
            int matrix, int range, Plan& pl) {
    FLAIR_CHECK(H >= 1 && W >= 1, "%s: H = %d, W = %d must be positive", fn, H, W);
    FLAIR_CHECK(N >= 0, "%s: N = %d frames must not be negative", fn, N);
    FLAIR_CHECK(format >= FLAIR_YUV_420JPEG && format <= FLAIR_YUV_MONO, "%s: unknown format = %d (420jpeg 0, 420mpeg2 1, 422 2, 444 3, mono 4)", fn, format);
    FLAIR_CHECK(matrix == FLAIR_YUV_BT601 || matrix == FLAIR_YUV_BT709, "%s: unknown matrix = %d (bt601 0, bt709 1)", fn, matrix);
    FLAIR_CHECK(range == FLAIR_YUV_LIMITED || range == FLAIR_YUV_FULL, "%s: unknown range = %d (limited 0, full 1)", fn, range);
    if (N == 0) return FLAIR_OK;
    FLAIR_CHECK(in && out, "%s: null pointer (%s = %p, %s = %p)", fn, in_name, in, out_name, out);
    const bool sub_x = format != FLAIR_YUV_444, sub_y = format == FLAIR_YUV_420JPEG || format == FLAIR_YUV_420MPEG2;
    pl.wc = format == FLAIR_YUV_MONO ? 0 : (sub_x ? (int)(((long)W + 1) / 2) : W);
    pl.hc = format == FLAIR_YUV_MONO ? 0 : (sub_y ? (int)(((long)H + 1) / 2) : H);
    pl.tilesX = cdiv(W, YT_W), pl.tilesY = cdiv(H, YT_H);
    FLAIR_CHECK((double)N * (double)pl.tilesX * (double)pl.tilesY <= (double)0x7fffffffL,            // in double first: three ints can pass 2^63
                "%s: N = %d frames of %d x %d pixels exceed one launch of 2^31 - 1 workgroups", fn, N, H, W);
    FLAIR_CHECK((double)N * (double)H * (double)W * 3.0 < 9.0e18, "%s: N = %d frames of %d x %d pixels exceed 64-bit offsets", fn, N, H, W);
    pl.P = (size_t)H * (size_t)W + 2 * (size_t)pl.wc * (size_t)pl.hc;
    pl.payload_bytes = (size_t)N * pl.P, pl.rgb_bytes = (size_t)N * (size_t)H * (size_t)W * 3;
    const size_t in_bytes = in_is_payload ? pl.payload_bytes : pl.rgb_bytes, out_bytes = in_is_payload ? pl.rgb_bytes : pl.payload_bytes;
    FLAIR_CHECK(!overlaps(out, out_bytes, in, in_bytes), "%s: %s overlaps %s (%s = %p, %zu bytes; %s = %p, %zu bytes)", fn, out_name, in_name, in_name, in,
                in_bytes, out_name, out, out_bytes);
    pl.grid = (unsigned)((long)N * pl.tilesX * pl.tilesY);
    pl.k = coef_of(matrix, range);
    return FLAIR_OK;
}

template <bool PLANAR>
void launch_decode(int format, const Plan& pl, const uint8_t* payload, int H, int W, uint8_t* out, hipStream_t stream) {
#define FLAIR_YUV_DECODE(HM, VM, MONO)                                                                                                                   \
    hipLaunchKernelGGL((yuv_to_rgb_kernel<HM, VM, MONO, PLANAR>), dim3(pl.grid), dim3(YT_THREADS), 0, stream, payload, H, W, pl.wc, pl.hc, pl.P, pl.tilesX, \
                       pl.tilesY, pl.k, out)
    switch (format) {
        case FLAIR_YUV_420JPEG: FLAIR_YUV_DECODE(AX_CENTRED, AX_CENTRED, false); break;
        case FLAIR_YUV_420MPEG2: FLAIR_YUV_DECODE(AX_COSITED, AX_CENTRED, false); break;
        case FLAIR_YUV_422: FLAIR_YUV_DECODE(AX_COSITED, AX_FULL, false); break;
        case FLAIR_YUV_444: FLAIR_YUV_DECODE(AX_FULL, AX_FULL, false); break;
        default: FLAIR_YUV_DECODE(AX_FULL, AX_FULL, true); break;
    }
#undef FLAIR_YUV_DECODE
}
}  // namespace

extern "C" int flair_yuv_to_rgb_u8(const uint8_t* payload, int N, int H, int W, int format, int matrix, int range, int planar, uint8_t* out,
                                   hipStream_t stream) {
    FLAIR_CHECK(planar == 0 || planar == 1, "flair_yuv_to_rgb_u8: planar = %d is 0 ([N][H][W][3]) or 1 ([N][3][H][W])", planar);
    Plan pl;
    const int st = plan_of("flair_yuv_to_rgb_u8", payload, "payload", out, "out", true, N, H, W, format, matrix, range, pl);
    if (st != FLAIR_OK || N == 0) return st;
    if (planar)
        launch_decode<true>(format, pl, payload, H, W, out, stream);
    else
        launch_decode<false>(format, pl, payload, H, W, out, stream);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_rgb_to_yuv_u8(const uint8_t* rgb, int N, int H, int W, int format, int matrix, int range, uint8_t* payload_out, hipStream_t stream) {
    Plan pl;
    const int st = plan_of("flair_rgb_to_yuv_u8", rgb, "rgb", payload_out, "payload_out", false, N, H, W, format, matrix, range, pl);
    if (st != FLAIR_OK || N == 0) return st;
#define FLAIR_YUV_ENCODE(HM, VM, MONO)                                                                                                              \
    hipLaunchKernelGGL((rgb_to_yuv_kernel<HM, VM, MONO>), dim3(pl.grid), dim3(YT_THREADS), 0, stream, rgb, H, W, pl.wc, pl.hc, pl.P, pl.tilesX, pl.tilesY, \
                       pl.k, payload_out)
    switch (format) {
        case FLAIR_YUV_420JPEG: FLAIR_YUV_ENCODE(AX_CENTRED, AX_CENTRED, false); break;
        case FLAIR_YUV_420MPEG2: FLAIR_YUV_ENCODE(AX_COSITED, AX_CENTRED, false); break;
        case FLAIR_YUV_422: FLAIR_YUV_ENCODE(AX_COSITED, AX_FULL, false); break;
        case FLAIR_YUV_444: FLAIR_YUV_ENCODE(AX_FULL, AX_FULL, false); break;
        default: FLAIR_YUV_ENCODE(AX_FULL, AX_FULL, true); break;
    }
#undef FLAIR_YUV_ENCODE
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
