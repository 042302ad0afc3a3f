// NIQE, the no-reference kernels: flair_niqe_luma, flair_niqe_moments (include/flair_noref.h, which holds the definition and
// both entries' contracts).  The AGGD fits and the distance to the pristine model are host work (flair_amd/niqe.py).
//
//   luma      one workgroup per 32 x 32 tile of the cropped luma plane: 38 x 38 haloed luma values (exact integers, reflected at
//             the crop's border) in LDS, written out as y1; the 8-tap half-scale filter along the rows into a 38 x 16 strip,
//             then along the columns, one y2 value per thread.  Integers only.
//   moments   one workgroup per (frame, block): the haloed int32 tile and the block's float64 MSCN map in LDS; per-lane sums of
//             the five maps' five moments over the thread's nine pixels tid, tid + THREADS, ..., a shuffle tree per wave, the
//             waves in order.  1024 threads at 96 and 256 at 48, because a block is one workgroup's latency; the window comes
//             through the scalar cache.
//             Built with -ffp-contract=off (Makefile): the shifted sums are the definition's, product by product.
#include "common.h"

#include "../../include/flair_noref.h"

namespace {
constexpr int NQ_THREADS = 256;                              // the luma kernel's workgroup (the moments kernel's: NiqeLds)
constexpr int NQ_WIN = 7, NQ_R = NQ_WIN / 2;                 // the MSCN window and its radius
constexpr int NQ_MOMENTS = 25;                               // five maps x (c-, c+, s-, s+, a)

// ---- luma and half scale ------------------------------------------------------------------------------------------------
constexpr int NL_TILE = 32, NL_HALF = NL_TILE / 2;           // y1 tile of a workgroup and its y2 tile
constexpr int NL_BEFORE = 3, NL_AFTER = 4;                   // output i reads inputs 2i - 3 .. 2i + 4
constexpr int NL_HALO = NL_TILE + NL_BEFORE + NL_AFTER - 1;  // 38: inputs 2 * 0 - 3 .. 2 * 15 + 4
static_assert(FLAIR_NIQE_BLOCK % NL_TILE == 0 && NL_HALF * NL_HALF == NQ_THREADS, "tiles cover the crop; one y2 value per thread");

// round_half_even((65481 R + 128553 G + 24966 B) / 255000) + 16; the numerator is at most 219000 * 255 < 2^26
__device__ __forceinline__ int niqe_luma_of(unsigned r, unsigned g, unsigned b) {
    const int num = (int)(65481u * r + 128553u * g + 24966u * b);
    const int q = num / 255000, twice = 2 * (num - q * 255000);
    return q + ((twice > 255000 || (twice == 255000 && (q & 1))) ? 1 : 0) + 16;
}

// symmetric reflection about the plane's border: -1 -> 0, -2 -> 1, n -> n - 1 (|overshoot| <= 4 < n)
__device__ __forceinline__ int niqe_reflect(int i, int n) { return i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i); }

__device__ __forceinline__ int niqe_half8(const int* p, int stride) {
    return -3 * (p[0] + p[7 * stride]) - 9 * (p[stride] + p[6 * stride]) + 29 * (p[2 * stride] + p[5 * stride]) +
           111 * (p[3 * stride] + p[4 * stride]);
}

__global__ __launch_bounds__(NQ_THREADS) void niqe_luma_kernel(const uint8_t* __restrict__ u8, int H, int W, int Hc, int Wc,
                                                                int tilesX, int tiles, int* __restrict__ y1, int* __restrict__ y2) {
    __shared__ int tile[NL_HALO][NL_HALO + 1];
    __shared__ int strip[NL_HALO][NL_HALF];
    const int tid = threadIdx.x;
    const int t = (int)(blockIdx.x % (unsigned)tiles);
    const size_t n = blockIdx.x / (unsigned)tiles;
    const int ty = t / tilesX, tx = t - ty * tilesX;
    const int gy0 = ty * NL_TILE - NL_BEFORE, gx0 = tx * NL_TILE - NL_BEFORE;
    const uint8_t* frame = u8 + n * (size_t)H * (size_t)W * 3;
    for (int e = tid; e < NL_HALO * NL_HALO; e += NQ_THREADS) {
        const int r = e / NL_HALO, c = e - r * NL_HALO;
        const int gy = niqe_reflect(gy0 + r, Hc), gx = niqe_reflect(gx0 + c, Wc);      // inside the crop, so inside the frame
        const uint8_t* px = frame + ((size_t)gy * (size_t)W + (size_t)gx) * 3;
        tile[r][c] = niqe_luma_of(px[0], px[1], px[2]);
    }
    __syncthreads();
    int* p1 = y1 + (n * (size_t)Hc + (size_t)(ty * NL_TILE)) * (size_t)Wc + (size_t)(tx * NL_TILE);
    for (int e = tid; e < NL_TILE * NL_TILE; e += NQ_THREADS) {
        const int r = e / NL_TILE, c = e % NL_TILE;
        p1[(size_t)r * (size_t)Wc + c] = tile[r + NL_BEFORE][c + NL_BEFORE];
    }
    for (int e = tid; e < NL_HALO * NL_HALF; e += NQ_THREADS) {
        const int r = e / NL_HALF, j = e % NL_HALF;
        strip[r][j] = niqe_half8(&tile[r][2 * j], 1);
    }
    __syncthreads();
    const int i = tid / NL_HALF, j = tid % NL_HALF;
    const int H2 = Hc / 2, W2 = Wc / 2;
    y2[(n * (size_t)H2 + (size_t)(ty * NL_HALF + i)) * (size_t)W2 + (size_t)(tx * NL_HALF + j)] = niqe_half8(&strip[2 * i][j], NL_HALF);
}

// ---- MSCN map and block moments -----------------------------------------------------------------------------------------
template <int B>
struct NiqeLds {                                             // a workgroup of the moments kernel: threads and dynamic LDS, doubles first
    static constexpr int THREADS = B * B / 9;                // nine pixels per thread: 1024 threads at 96, 256 at 48
    static constexpr int WAVES = THREADS / FLAIR_WAVE;
    static constexpr int T = B + 2 * NQ_R;                   // the haloed tile's side
    static constexpr int M = 0;                              // double m[B * B]
    static constexpr int RED = M + B * B;                    // double red[waves][25]
    static constexpr int TILE = RED + WAVES * NQ_MOMENTS;    // int tile[T * T], counted in doubles up to here
    static constexpr int BYTES = TILE * 8 + T * T * 4;
    static_assert(THREADS * 9 == B * B && THREADS % FLAIR_WAVE == 0 && THREADS <= 1024, "whole waves, nine pixels each");
};
static_assert(NiqeLds<FLAIR_NIQE_BLOCK>::BYTES == 118544 && NiqeLds<FLAIR_NIQE_BLOCK>::BYTES <= 160 * 1024, "the header states the size at 96");

template <int B>
__global__ __launch_bounds__(NiqeLds<B>::THREADS) void niqe_moments_kernel(const int* __restrict__ y, int Hc, int Wc, int nh, int nblocks,
                                                                            double inv_scale, const double* __restrict__ window,
                                                                            double* __restrict__ out, double* __restrict__ mscn) {
    using L = NiqeLds<B>;
    constexpr int T = L::T, THREADS = L::THREADS;
    extern __shared__ __attribute__((aligned(16))) char nq_smem[];
    double* m = reinterpret_cast<double*>(nq_smem) + L::M;
    double* red = reinterpret_cast<double*>(nq_smem) + L::RED;
    int* tile = reinterpret_cast<int*>(reinterpret_cast<double*>(nq_smem) + L::TILE);
    const int tid = threadIdx.x;
    const int blk = (int)(blockIdx.x % (unsigned)nblocks);
    const size_t n = blockIdx.x / (unsigned)nblocks;
    const int bj = blk / nh, bi = blk - bj * nh;             // block index j nh + i
    const int gy0 = bi * B - NQ_R, gx0 = bj * B - NQ_R;
    const int* plane = y + n * (size_t)Hc * (size_t)Wc;
    for (int e = tid; e < T * T; e += THREADS) {
        const int r = e / T, c = e - r * T;
        const int gy = min(max(gy0 + r, 0), Hc - 1), gx = min(max(gx0 + c, 0), Wc - 1);      // replicate border of the plane
        tile[e] = plane[(size_t)gy * (size_t)Wc + (size_t)gx];
    }
    __syncthreads();

    // M = (Y - mu) / (sigma + 1) in the shifted form: d is an exact double (an integer difference times a power of two).
    // The window's index is uniform over the wave, so its 49 doubles arrive through the scalar cache, not through LDS.
    double* pm = mscn ? mscn + (n * (size_t)Hc + (size_t)(bi * B)) * (size_t)Wc + (size_t)(bj * B) : nullptr;
    for (int p = tid; p < B * B; p += THREADS) {
        const int r = p / B, c = p - r * B;
        const int* t = tile + r * T + c;
        const int centre = t[NQ_R * T + NQ_R];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int ky = 0; ky < NQ_WIN; ++ky)
#pragma unroll
            for (int kx = 0; kx < NQ_WIN; ++kx) {
                const double d = (double)(t[ky * T + kx] - centre) * inv_scale;
                const double gd = window[NQ_WIN * NQ_WIN - 1 - (ky * NQ_WIN + kx)] * d;      // tap (dy, dx) weighs window[3 - dy][3 - dx]
                s1 += gd;
                s2 += gd * d;
            }
        const double v = -s1 / (sqrt(fabs(s2 - s1 * s1)) + 1.0);
        m[p] = v;
        if (pm) pm[(size_t)r * (size_t)Wc + c] = v;
    }
    __syncthreads();

    double acc[NQ_MOMENTS];
#pragma unroll
    for (int q = 0; q < NQ_MOMENTS; ++q) acc[q] = 0.0;
    for (int p = tid; p < B * B; p += THREADS) {
        const int r = p / B, c = p - r * B;
        const int up = (r ? r - 1 : B - 1) * B, left = c ? c - 1 : B - 1, right = c + 1 < B ? c + 1 : 0;
        const double v = m[p];
        // roll(M, s)[r][c] = M[r - s0][c - s1], wrapping inside the block: s = (0,1), (1,0), (1,1), (1,-1)
        const double x[5] = {v, v * m[r * B + left], v * m[up + c], v * m[up + left], v * m[up + right]};
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double xx = x[k] * x[k];
            const bool neg = x[k] < 0.0, pos = x[k] > 0.0;
            acc[5 * k + 0] += neg ? 1.0 : 0.0;
            acc[5 * k + 1] += pos ? 1.0 : 0.0;
            acc[5 * k + 2] += neg ? xx : 0.0;
            acc[5 * k + 3] += pos ? xx : 0.0;
            acc[5 * k + 4] += fabs(x[k]);
        }
    }
#pragma unroll
    for (int q = 0; q < NQ_MOMENTS; ++q) {
        double s = acc[q];
#pragma unroll
        for (int off = FLAIR_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, FLAIR_WAVE);
        if ((tid & (FLAIR_WAVE - 1)) == 0) red[(tid / FLAIR_WAVE) * NQ_MOMENTS + q] = s;
    }
    __syncthreads();
    if (tid < NQ_MOMENTS) {
        double s = red[tid];
#pragma unroll
        for (int w = 1; w < L::WAVES; ++w) s += red[w * NQ_MOMENTS + tid];
        out[(size_t)blockIdx.x * NQ_MOMENTS + tid] = s;
    }
}

template <int B>
int launch_moments(unsigned groups, hipStream_t stream, const int* y, int Hc, int Wc, double inv_scale, const double* window,
                   double* out, double* mscn) {
    static LdsAttrOnce attr;
    FLAIR_CHECK(flair_max_lds_once(attr, reinterpret_cast<const void*>(&niqe_moments_kernel<B>), NiqeLds<B>::BYTES) == hipSuccess,
                "flair_niqe_moments: hipFuncSetAttribute failed");
    const int nh = Hc / B, nblocks = nh * (Wc / B);
    hipLaunchKernelGGL(niqe_moments_kernel<B>, dim3(groups), dim3(NiqeLds<B>::THREADS), (size_t)NiqeLds<B>::BYTES, stream, y, Hc, Wc, nh,
                       nblocks, inv_scale, window, out, mscn);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
}  // namespace

extern "C" int flair_niqe_luma(const uint8_t* u8, int N, int H, int W, int* y1, int* y2, hipStream_t stream) {
    FLAIR_CHECK(u8 && y1 && y2, "flair_niqe_luma: null pointer (u8 = %p, y1 = %p, y2 = %p)", (const void*)u8, (const void*)y1, (const void*)y2);
    FLAIR_CHECK(N >= 1 && H >= 1 && W >= 1, "flair_niqe_luma: N = %d, H = %d, W = %d must be positive", N, H, W);
    FLAIR_CHECK(H >= FLAIR_NIQE_BLOCK && W >= FLAIR_NIQE_BLOCK, "flair_niqe_luma: frames of %dx%d hold no %dx%d block", H, W,
                FLAIR_NIQE_BLOCK, FLAIR_NIQE_BLOCK);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(y1) % 4 == 0 && reinterpret_cast<uintptr_t>(y2) % 4 == 0,
                "flair_niqe_luma: y1 = %p and y2 = %p hold int32 and must be 4-byte aligned", (const void*)y1, (const void*)y2);
    const int Hc = H / FLAIR_NIQE_BLOCK * FLAIR_NIQE_BLOCK, Wc = W / FLAIR_NIQE_BLOCK * FLAIR_NIQE_BLOCK;
    const long tilesX = Wc / NL_TILE, tiles = tilesX * (Hc / NL_TILE);
    FLAIR_CHECK(tiles <= 0x7fffffffL / N, "flair_niqe_luma: %ld tiles in each of N = %d frames of %dx%d exceed one launch", tiles, N, H, W);
    const long groups = (long)N * tiles;
    hipLaunchKernelGGL(niqe_luma_kernel, dim3((unsigned)groups), dim3(NQ_THREADS), 0, stream, u8, H, W, Hc, Wc, (int)tilesX, (int)tiles,
                       y1, y2);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_niqe_moments(const int* y, int N, int Hc, int Wc, int block, double inv_scale, const double* window,
                                  double* out, double* mscn, hipStream_t stream) {
    FLAIR_CHECK(y && window && out, "flair_niqe_moments: null pointer (y = %p, window = %p, out = %p)", (const void*)y,
                (const void*)window, (const void*)out);
    FLAIR_CHECK(N >= 1 && Hc >= 1 && Wc >= 1, "flair_niqe_moments: N = %d, Hc = %d, Wc = %d must be positive", N, Hc, Wc);
    FLAIR_CHECK(block == FLAIR_NIQE_BLOCK || block == FLAIR_NIQE_BLOCK / 2, "flair_niqe_moments: block = %d, the blocks are %d (scale 1) or %d (scale 2) pixels a side",
                block, FLAIR_NIQE_BLOCK, FLAIR_NIQE_BLOCK / 2);
    FLAIR_CHECK(Hc % block == 0 && Wc % block == 0, "flair_niqe_moments: the plane of %dx%d is not made of %dx%d blocks", Hc, Wc, block, block);
    FLAIR_CHECK(inv_scale == 1.0 || inv_scale == 1.0 / 65536.0, "flair_niqe_moments: inv_scale = %g, a plane holds the luma (1) or 65536 times the half-scale luma (2^-16)",
                inv_scale);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(y) % 4 == 0, "flair_niqe_moments: y = %p holds int32 and must be 4-byte aligned", (const void*)y);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(window) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0 && reinterpret_cast<uintptr_t>(mscn) % 8 == 0,
                "flair_niqe_moments: window = %p, out = %p and mscn = %p hold doubles and must be 8-byte aligned", (const void*)window,
                (const void*)out, (const void*)mscn);
    const long blocks = (long)(Hc / block) * (Wc / block);
    FLAIR_CHECK(blocks <= 0x7fffffffL / N, "flair_niqe_moments: %ld blocks in each of N = %d planes of %dx%d exceed one launch", blocks, N, Hc, Wc);
    const long groups = (long)N * blocks;
    return block == FLAIR_NIQE_BLOCK ? launch_moments<FLAIR_NIQE_BLOCK>((unsigned)groups, stream, y, Hc, Wc, inv_scale, window, out, mscn)
                                     : launch_moments<FLAIR_NIQE_BLOCK / 2>((unsigned)groups, stream, y, Hc, Wc, inv_scale, window, out, mscn);
}
