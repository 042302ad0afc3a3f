// Block luma sums of written frames, the input of scene-cut detection: flair_block_luma_sums (include/flair_hip.h, "scene cuts").
//
// A frame is cut into an 8 x 8 grid of blocks, block (a, b) = rows (a H) / 8 .. ((a + 1) H) / 8, columns (b W) / 8 .. ((b + 1) W) / 8.
// One workgroup of 256 threads owns up to SC_ROWS = 32 rows of ONE block of one frame, so every pixel it reads adds to one
// output entry and no pixel needs a division to find its block:
//   1. items    the bw = x1 - x0 pixels of a row of the block are 3 bw contiguous bytes at an address p of ANY alignment (rows are
//               3 W bytes, frames H W 3 bytes, the block starts 3 x0 bytes into its row).  With c = p & 3, pixel c of the segment
//               is the first whose bytes start on a dword ((p + 3 c) & 3 = 4 c & 3 = 0), and so does every fourth pixel after
//               it.  Item 0 of a row is the head, pixels 0 .. c - 1, read byte by byte; item g >= 1 is pixels c + 4 (g - 1) .. + 3,
//               three aligned dwords (consecutive lanes read consecutive 12-byte pieces), or, where fewer than four pixels
//               remain, the tail, byte by byte.  Nothing outside the segment is read and every byte of it is read once.
//   2. luma     Y = (77 R + 150 G + 29 B + 128) >> 8 per pixel, the (at most four) pixels of an item summed in 32 bits, items in 64;
//   3. reduce   64-bit shuffles inside a wave, LDS across the four waves, ONE 64-bit integer atomic add per workgroup.
// Integer arithmetic throughout: the sums are exact and do not depend on the order of the adds, so a frame's 64 values are the
// same in every run and for every N.  The entry zeroes the output on the stream before the launch.
#include "common.h"

namespace {
constexpr int SC_GRID = 8;                 // blocks per side
constexpr int SC_THREADS = 256;
constexpr int SC_ROWS = 32;                // rows of a block per workgroup

__device__ __forceinline__ unsigned luma_of(unsigned r, unsigned g, unsigned b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

__global__ __launch_bounds__(SC_THREADS) void block_luma_sums_kernel(const uint8_t* __restrict__ frames, int H, int W, int slices,
                                                                      unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[SC_THREADS / FLAIR_WAVE];
    const int tid = threadIdx.x;
    const unsigned bid = blockIdx.x;                       // = (n * 64 + 8 a + b) * slices + s
    const int s = (int)(bid % (unsigned)slices);
    const unsigned cell = bid / (unsigned)slices;          // the output entry
    const int b = (int)(cell & 7u), a = (int)((cell >> 3) & 7u);
    const size_t n = cell >> 6;
    const int ya = (int)(((long long)a * H) / SC_GRID), yb = (int)(((long long)(a + 1) * H) / SC_GRID);
    const int x0 = (int)(((long long)b * W) / SC_GRID), x1 = (int)(((long long)(b + 1) * W) / SC_GRID);
    const int y0 = ya + s * SC_ROWS;
    const int rows = min(SC_ROWS, yb - y0);
    if (rows <= 0) return;                                 // the whole workgroup: blocks of a frame differ in height by one row
    const int bw = x1 - x0;                                // >= 1 (W >= 8)
    const int gpr = 1 + (bw + 3) / 4;                      // items per row: the head and at most ceil(bw / 4) groups
    const int items = rows * gpr;
    int r = tid / gpr, g = tid - r * gpr;
    const int dr = SC_THREADS / gpr, dg = SC_THREADS - dr * gpr;

    unsigned long long acc = 0;
    for (int item = tid; item < items; item += SC_THREADS) {
        const uint8_t* p = frames + ((n * (size_t)H + (size_t)(y0 + r)) * (size_t)W + (size_t)x0) * 3u;
        const int c = (int)(reinterpret_cast<uintptr_t>(p) & 3u);
        const int first = g == 0 ? 0 : c + 4 * (g - 1);
        const int count = g == 0 ? min(c, bw) : min(4, bw - first);          // <= 0 past the end of the row
        if (g != 0 && count == 4) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p + 3 * (size_t)first);   // dword aligned (see above)
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];                  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            acc += luma_of(w0 & 0xffu, (w0 >> 8) & 0xffu, (w0 >> 16) & 0xffu) + luma_of(w0 >> 24, w1 & 0xffu, (w1 >> 8) & 0xffu) +
                   luma_of((w1 >> 16) & 0xffu, w1 >> 24, w2 & 0xffu) + luma_of((w2 >> 8) & 0xffu, (w2 >> 16) & 0xffu, w2 >> 24);
        } else {
            for (int k = 0; k < count; ++k) {
                const uint8_t* e = p + 3 * (size_t)(first + k);
                acc += luma_of(e[0], e[1], e[2]);
            }
        }
        r += dr;
        g += dg;
        if (g >= gpr) {
            g -= gpr;
            ++r;
        }
    }

    unsigned long long v = acc;
#pragma unroll
    for (int off = FLAIR_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, FLAIR_WAVE);
    if ((tid & (FLAIR_WAVE - 1)) == 0) red[tid / FLAIR_WAVE] = v;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = red[0];
#pragma unroll
        for (int w = 1; w < SC_THREADS / FLAIR_WAVE; ++w) t += red[w];
        atomicAdd(out + cell, t);
    }
}
}  // namespace

extern "C" int flair_block_luma_sums(const uint8_t* frames, int N, int H, int W, long long* out, hipStream_t stream) {
    FLAIR_CHECK(frames && out, "flair_block_luma_sums: null pointer (frames = %p, out = %p)", (const void*)frames, (const void*)out);
    FLAIR_CHECK(N >= 1, "flair_block_luma_sums: N = %d frames, need at least one", N);
    FLAIR_CHECK(H >= SC_GRID && W >= SC_GRID, "flair_block_luma_sums: frames of %dx%d are smaller than the 8x8 grid of blocks", H, W);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(out) % 8 == 0, "flair_block_luma_sums: out = %p holds 64-bit integers and must be 8-byte aligned",
                (const void*)out);
    FLAIR_CHECK(W <= (1 << 24), "flair_block_luma_sums: W = %d, rows of more than 2^24 pixels overflow the 32-bit item index", W);
    const long slices = cdiv(cdiv(H, SC_GRID), SC_ROWS);                       // the tallest block has ceil(H / 8) rows
    const long groups = (long)N * SC_GRID * SC_GRID * slices;
    FLAIR_CHECK(groups <= 0x7fffffffL, "flair_block_luma_sums: %ld workgroups (N = %d, %dx%d) exceed one launch", groups, N, H, W);
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)N * SC_GRID * SC_GRID * sizeof(long long), stream);
    if (e != hipSuccess) {
        flair_set_error("flair_block_luma_sums: hipMemsetAsync failed: %s", hipGetErrorString(e));
        return FLAIR_ERR_HIP;
    }
    hipLaunchKernelGGL(block_luma_sums_kernel, dim3((unsigned)groups), dim3(SC_THREADS), 0, stream, frames, H, W, (int)slices,
                       reinterpret_cast<unsigned long long*>(out));
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
