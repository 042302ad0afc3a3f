// The face score's crop: flair_face_crop_u8 (include/flair_facescore.h, which holds the definition and the entry's contract).
// Written bytes of one or two frame sets in, aligned byte crops out; two float64 roundings in the position, integers after that.
// Compiled with -ffp-contract=off (Makefile): the products and the sum of the position are rounded on their own.
//
//   one thread per destination pixel, lane = column, a workgroup owns 4 rows of 64 pixels of one face.  A thread computes the
//   position once, then gathers the 4 x 4 taps of both sets byte by byte (a gather from L2: neighbouring lanes read
//   neighbouring pixels under the similarity transforms of face alignment) and stores 3 or 6 bytes.  No LDS, no atomics.
#include "common.h"

#include "../../include/flair_facescore.h"

namespace {
constexpr int FC_ROWS = 4;                                               // rows of a workgroup, one wave each
constexpr int FC_THREADS = FC_ROWS * FLAIR_WAVE;
constexpr int FC_TAB_BITS = 17;

// The a = -0.75 cubic at the fractions i / 32, times 2^17: exact integers, every row sums to 2^17 (tests/test_facecrop_cpu.py
// compares this table with the rational evaluation of tests/face_ref.py).
__constant__ int FC_TAB[32][4] = {
    {0, 131072, 0, 0},
    {-2883, 130789, 3259, -93},
    {-5400, 129960, 6872, -360},
    {-7569, 128615, 10809, -783},
    {-9408, 126784, 15040, -1344},
    {-10935, 124497, 19535, -2025},
    {-12168, 121784, 24264, -2808},
    {-13125, 118675, 29197, -3675},
    {-13824, 115200, 34304, -4608},
    {-14283, 111389, 39555, -5589},
    {-14520, 107272, 44920, -6600},
    {-14553, 102879, 50369, -7623},
    {-14400, 98240, 55872, -8640},
    {-14079, 93385, 61399, -9633},
    {-13608, 88344, 66920, -10584},
    {-13005, 83147, 72405, -11475},
    {-12288, 77824, 77824, -12288},
    {-11475, 72405, 83147, -13005},
    {-10584, 66920, 88344, -13608},
    {-9633, 61399, 93385, -14079},
    {-8640, 55872, 98240, -14400},
    {-7623, 50369, 102879, -14553},
    {-6600, 44920, 107272, -14520},
    {-5589, 39555, 111389, -14283},
    {-4608, 34304, 115200, -13824},
    {-3675, 29197, 118675, -13125},
    {-2808, 24264, 121784, -12168},
    {-2025, 19535, 124497, -10935},
    {-1344, 15040, 126784, -9408},
    {-783, 10809, 128615, -7569},
    {-360, 6872, 129960, -5400},
    {-93, 3259, 130789, -2883},
};

struct Border {
    int v[3];
};

// Step 1 for one axis: (m0 x, m1 y + m2) -> the position in 1/32 pixel.  Beyond 2^40 in magnitude (no frame is that large; the
// wrapper refuses far earlier) the value is pinned, so that the conversion to an integer is defined and the taps lie outside.
__device__ __forceinline__ long long position(double m0, double m1, double m2, int x, int y) {
    const double LIM = 1099511627776.0;
    double a = rint(m0 * (double)x * 1024.0);
    double b = rint((m1 * (double)y + m2) * 1024.0);
    a = a > -LIM ? (a < LIM ? a : LIM) : -LIM;                           // not-a-number compares false: -LIM
    b = b > -LIM ? (b < LIM ? b : LIM) : -LIM;
    return ((long long)b + 16 + (long long)a) >> 5;
}

__device__ __forceinline__ uint8_t to_byte(long long S) {
    const long long v = (S + (1ll << (2 * FC_TAB_BITS - 1))) >> (2 * FC_TAB_BITS);
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// block = (face, row group, column group), column groups fastest
__global__ __launch_bounds__(FC_THREADS) void face_crop_u8_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int Nsrc, int Hs,
                                                                   int Ws, const double* __restrict__ minv, const int* __restrict__ src_index,
                                                                   int Hd, int Wd, int tilesX, int tilesY, Border border,
                                                                   uint8_t* __restrict__ out_a, uint8_t* __restrict__ out_b) {
    const int lane = threadIdx.x & (FLAIR_WAVE - 1), wave = threadIdx.x / FLAIR_WAVE;
    const unsigned tx = blockIdx.x % (unsigned)tilesX, rest = blockIdx.x / (unsigned)tilesX;
    const unsigned ty = rest % (unsigned)tilesY;
    const size_t k = rest / (unsigned)tilesY;
    const int x = (int)tx * FLAIR_WAVE + lane, y = (int)ty * FC_ROWS + wave;
    if (x >= Wd || y >= Hd) return;

    const double* M = minv + k * 6;
    const long long X = position(M[0], M[1], M[2], x, y), Y = position(M[3], M[4], M[5], x, y);
    const long long sx = (X >> 5) - 1, sy = (Y >> 5) - 1;
    const int* wx = FC_TAB[(int)(X & 31)];
    const int* wy = FC_TAB[(int)(Y & 31)];
    const int frame = src_index[k];
    const bool have = frame >= 0 && frame < Nsrc;                        // the caller's promise; a broken one reads nothing
    const size_t plane = (size_t)Hs * (size_t)Ws * 3;
    const uint8_t* pa = a + (have ? (size_t)frame : 0) * plane;
    const uint8_t* pb = b ? b + (have ? (size_t)frame : 0) * plane : nullptr;

    // exact integers: the order of the sum is free, so a row's four taps are added in 32 bits (|t| <= 255 (11/8) 2^17 < 2^26)
    // and only the four row sums meet the 64-bit product
    long long Sa[3] = {0, 0, 0}, Sb[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long yi = sy + r;
        const bool rowIn = have && yi >= 0 && yi < Hs;
        int ta[3] = {0, 0, 0}, tb[3] = {0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long xi = sx + c;
            const bool in = rowIn && xi >= 0 && xi < Ws;
            const size_t off = in ? ((size_t)yi * (size_t)Ws + (size_t)xi) * 3 : 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                ta[ch] += (in ? (int)pa[off + ch] : border.v[ch]) * wx[c];
                if (pb) tb[ch] += (in ? (int)pb[off + ch] : border.v[ch]) * wx[c];
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            Sa[ch] += (long long)ta[ch] * (long long)wy[r];
            Sb[ch] += (long long)tb[ch] * (long long)wy[r];
        }
    }
    const size_t o = ((k * (size_t)Hd + (size_t)y) * (size_t)Wd + (size_t)x) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out_a[o + ch] = to_byte(Sa[ch]);
    if (pb) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out_b[o + ch] = to_byte(Sb[ch]);
    }
}

bool overlaps(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}
}  // namespace

extern "C" int flair_face_crop_u8(const uint8_t* a, const uint8_t* b, int Nsrc, int Hs, int Ws, const double* minv, const int* src_index,
                                  int K, int Hd, int Wd, const uint8_t* border, uint8_t* out_a, uint8_t* out_b, hipStream_t stream) {
    FLAIR_CHECK(a && border, "flair_face_crop_u8: null pointer (a = %p, border = %p; b and out_b may be null together)", (const void*)a,
                (const void*)border);
    FLAIR_CHECK((b != nullptr) == (out_b != nullptr),
                "flair_face_crop_u8: b = %p and out_b = %p: a second frame set and its crops come together or not at all", (const void*)b,
                (const void*)out_b);
    FLAIR_CHECK(Nsrc >= 1 && Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1, "flair_face_crop_u8: Nsrc = %d, Hs = %d, Ws = %d, Hd = %d, Wd = %d must be positive",
                Nsrc, Hs, Ws, Hd, Wd);
    FLAIR_CHECK(K >= 0, "flair_face_crop_u8: K = %d faces must not be negative", K);
    if (K == 0) return FLAIR_OK;
    FLAIR_CHECK(minv && src_index && out_a, "flair_face_crop_u8: null pointer (minv = %p, src_index = %p, out_a = %p)", (const void*)minv,
                (const void*)src_index, (const void*)out_a);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(minv) % 8 == 0 && reinterpret_cast<uintptr_t>(src_index) % 4 == 0,
                "flair_face_crop_u8: minv = %p holds doubles and must be 8-byte aligned, src_index = %p ints and 4-byte aligned", (const void*)minv,
                (const void*)src_index);
    const int tilesX = cdiv(Wd, FLAIR_WAVE), tilesY = cdiv(Hd, FC_ROWS);
    FLAIR_CHECK((double)K * (double)tilesX * (double)tilesY <= (double)0x7fffffffL,       // in double first: three ints can pass 2^63
                "flair_face_crop_u8: K = %d faces of %d x %d pixels exceed one launch of 2^31 - 1 workgroups", K, Hd, Wd);
    const double src_d = (double)Nsrc * (double)Hs * (double)Ws * 3.0, out_d = (double)K * (double)Hd * (double)Wd * 3.0;
    FLAIR_CHECK(src_d < 9.0e18 && out_d < 9.0e18, "flair_face_crop_u8: a frame set of %.0f bytes or crops of %.0f bytes exceed 64-bit offsets", src_d, out_d);
    const size_t src_bytes = (size_t)Nsrc * (size_t)Hs * (size_t)Ws * 3, out_bytes = (size_t)K * (size_t)Hd * (size_t)Wd * 3;
    FLAIR_CHECK(!overlaps(out_a, out_bytes, a, src_bytes) && !(b && overlaps(out_a, out_bytes, b, src_bytes)) &&
                    !(out_b && (overlaps(out_b, out_bytes, a, src_bytes) || overlaps(out_b, out_bytes, b, src_bytes))),
                "flair_face_crop_u8: out overlaps a source (a = %p, b = %p, %zu bytes each; out_a = %p, out_b = %p, %zu bytes each)", (const void*)a,
                (const void*)b, src_bytes, (const void*)out_a, (const void*)out_b, out_bytes);
    Border bd;
    for (int c = 0; c < 3; ++c) bd.v[c] = border[c];
    hipLaunchKernelGGL(face_crop_u8_kernel, dim3((unsigned)((long)K * tilesX * tilesY)), dim3(FC_THREADS), 0, stream, a, b, Nsrc, Hs, Ws, minv,
                       src_index, Hd, Wd, tilesX, tilesY, bd, out_a, out_b);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
