// Codebook search of RestoreFormer's VectorQuantizer.forward (reference guided_diffusion/restoreformer.py:43-62):
// for every token z (one NHWC pixel of D channels) the index of the nearest codebook row under the f32 squared
// distance |z|^2 + |e|^2 - 2 z.e, first index on ties (torch.min), and the gathered row.  The search is
// ~67 MFLOP per 512x512 face (256 tokens x 1024 codes x 256 channels), small next to the prior's convolutions:
// written for correctness with f32 arithmetic whatever the activation dtype, one launch per batch.
#include "common.h"

namespace {

constexpr int VQ_TOK = 8;         // tokens per workgroup (z rows staged in LDS as f32)
constexpr int VQ_MAX_D = 1024;    // 32 KiB of LDS at VQ_TOK = 8

// One workgroup = VQ_TOK tokens; thread t scans codes t, t + 256, ... (each thread reads its own codebook rows,
// 16 bytes at a time; the 1 MiB f32 codebook of the release stays L2 resident), keeps the smallest distance per token
// with the lowest index on ties, then the 256 candidates are reduced across the workgroup.
template <typename E>
__global__ __launch_bounds__(256) void vq_nearest_kernel(const E* z, int ld, long rows, int D, const float* codebook,
                                                         int N, const int* forced, int* idx, E* y, int yLd) {
    __shared__ __attribute__((aligned(16))) float zs[VQ_TOK * VQ_MAX_D];
    __shared__ float zz[VQ_TOK];
    __shared__ float red_v[4][VQ_TOK];
    __shared__ int red_i[4][VQ_TOK];
    __shared__ int best_s[VQ_TOK];
    const long row0 = (long)blockIdx.x * VQ_TOK;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (forced) {
        if (tid < VQ_TOK && row0 + tid < rows) {
            int b = forced[row0 + tid];
            best_s[tid] = b < 0 ? 0 : (b >= N ? N - 1 : b);   // an out-of-range index must not read outside the codebook
        }
    } else {
        for (int i = tid; i < VQ_TOK * D; i += 256) {
            const int t = i / D, c = i - t * D;
            zs[i] = row0 + t < rows ? ET<E>::ld(z + (row0 + t) * ld + c) : 0.f;
        }
        __syncthreads();
        // |z|^2 per token: wave w sums tokens w and w + 4
        for (int t = w; t < VQ_TOK; t += 4) {
            float s = 0.f;
            for (int c = lane; c < D; c += 64) s = fmaf(zs[t * D + c], zs[t * D + c], s);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) zz[t] = s;
        }
        __syncthreads();
        float bv[VQ_TOK];
        int bi[VQ_TOK];
#pragma unroll
        for (int t = 0; t < VQ_TOK; ++t) {
            bv[t] = INFINITY;
            bi[t] = N;
        }
        for (int n = tid; n < N; n += 256) {
            const float* e = codebook + (long)n * D;
            float dot[VQ_TOK];
#pragma unroll
            for (int t = 0; t < VQ_TOK; ++t) dot[t] = 0.f;
            float ee = 0.f;
            for (int c = 0; c < D; c += 4) {
                const float4 ev = *reinterpret_cast<const float4*>(e + c);
                ee = fmaf(ev.x, ev.x, ee);
                ee = fmaf(ev.y, ev.y, ee);
                ee = fmaf(ev.z, ev.z, ee);
                ee = fmaf(ev.w, ev.w, ee);
#pragma unroll
                for (int t = 0; t < VQ_TOK; ++t) {
                    const float4 zv = *reinterpret_cast<const float4*>(zs + t * D + c);
                    dot[t] = fmaf(zv.x, ev.x, dot[t]);
                    dot[t] = fmaf(zv.y, ev.y, dot[t]);
                    dot[t] = fmaf(zv.z, ev.z, dot[t]);
                    dot[t] = fmaf(zv.w, ev.w, dot[t]);
                }
            }
#pragma unroll
            for (int t = 0; t < VQ_TOK; ++t) {
                const float d = (zz[t] + ee) - 2.f * dot[t];
                if (d < bv[t]) {          // n increases along the scan: a later equal distance never replaces
                    bv[t] = d;
                    bi[t] = n;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < VQ_TOK; ++t) {
            float v = bv[t];
            int i = bi[t];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ov = __shfl_xor(v, off);
                const int oi = __shfl_xor(i, off);
                if (ov < v || (ov == v && oi < i)) {
                    v = ov;
                    i = oi;
                }
            }
            if (lane == 0) {
                red_v[w][t] = v;
                red_i[w][t] = i;
            }
        }
        __syncthreads();
        if (tid < VQ_TOK) {
            float v = red_v[0][tid];
            int i = red_i[0][tid];
            for (int k = 1; k < 4; ++k)
                if (red_v[k][tid] < v || (red_v[k][tid] == v && red_i[k][tid] < i)) {
                    v = red_v[k][tid];
                    i = red_i[k][tid];
                }
            best_s[tid] = i >= N ? 0 : i;     // every distance NaN: defined behaviour instead of an out-of-range read
        }
    }
    __syncthreads();
    for (int t = 0; t < VQ_TOK; ++t) {
        const long row = row0 + t;
        if (row >= rows) break;
        const int b = best_s[t];
        if (tid == 0 && idx) idx[row] = b;
        for (int c = tid; c < D; c += 256) ET<E>::st(y + row * yLd + c, codebook[(long)b * D + c]);
    }
}

}  // namespace

extern "C" int flair_vq_nearest_nhwc(const void* z, int dtype, int ld, long rows, int D, const float* codebook, int N,
                                     const int* forced_idx, int* idx, void* y, int y_ld, hipStream_t stream) {
    FLAIR_CHECK(codebook && y && (z || forced_idx), "flair_vq_nearest_nhwc: null argument");
    FLAIR_CHECK(rows > 0 && N > 0 && D > 0 && D % 4 == 0 && D <= VQ_MAX_D, "flair_vq_nearest_nhwc: D=%d unsupported", D);
    FLAIR_CHECK(ld >= D && y_ld >= D, "flair_vq_nearest_nhwc: strides");
    FLAIR_CHECK((reinterpret_cast<uintptr_t>(codebook) & 15) == 0, "flair_vq_nearest_nhwc: codebook must be 16-byte aligned");
    const dim3 grid((unsigned)((rows + VQ_TOK - 1) / VQ_TOK));
    return flair_by_dtype("flair_vq_nearest_nhwc", dtype, [&](auto e) -> int {
        using E = decltype(e);
        hipLaunchKernelGGL(vq_nearest_kernel<E>, grid, dim3(256), 0, stream, (const E*)z, ld, rows, D, codebook, N, forced_idx, idx,
                           (E*)y, y_ld);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}
