// SuperSloMo's per-timestep tail (guided_diffusion/superslomo.py:225-287) as two gather kernels on NHWC clips.
//
//  * flair_slomo_warp_pack -- stage A (:260-270): the two time-weighted flow combinations ft0 / ft1, back_warp(i0, ft0),
//                             back_warp(i1, ft1) and the 20-channel torch.cat the interpolation UNet reads.
//  * flair_slomo_blend     -- stage B (:273-287): the refined flows, the sigmoid visibility map, two more back-warps, the
//                             normalised blend and the de-normalisation, written as f32 NCHW.
//
// back_warp (:225-247) is NOT flair_flow_warp's convention: x = w + u, gx = 2 (x / W - 0.5), then F.grid_sample with its
// defaults (bilinear, zeros, align_corners=False), which maps back with ix = ((gx + 1) W - 1) / 2 = x - 0.5: the sample sits
// half a pixel up-left of w + u.  One thread per pixel; every corner is an unconditional 16-byte buffer load on a whole-clip
// descriptor (corners outside the frame get an out-of-range offset and read 0), all of them issued before the first use.
//
// The arithmetic is f32 in the reference's order of operations.  The Makefile compiles this file with -ffp-contract=off
// (under the library's -ffp-contract=fast the backend fuses whatever it can reach, pragmas or not): the flow combinations,
// the blend and the de-normalisation are sums of ROUNDED products in the reference, and `ix - floor(ix)` must see the
// rounded coordinate (warp.hip, gs_coord; bw_coord keeps that one out of reach of a fused build as well).
#include "common.h"

namespace {

template <typename E, int N>
struct Px {                                                    // the first N channels of one pixel as 16-byte pieces
    static constexpr int PIECES = (N * (int)sizeof(E) + 15) / 16;
    u32x4_t raw[PIECES];
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t r, unsigned byteOff) {
#pragma unroll
        for (int k = 0; k < PIECES; ++k)                                                  // FLAIR_OOB + 16 is out of range too
            raw[k] = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(byteOff + 16u * k), 0, 0);
    }
    __device__ __forceinline__ void get(float (&o)[PIECES * ET<E>::VEC]) const {
#pragma unroll
        for (int k = 0; k < PIECES; ++k) Vec16<E>::load(reinterpret_cast<const E*>(&raw[k]), o + k * ET<E>::VEC);
    }
};

// superslomo.py:241-242 and grid_sampler's unnormalize (align_corners=False), the round trip in the reference's order.
__device__ __forceinline__ float bw_coord(float pix, int size) {
    const float s = (float)size;
    const float g = 2.f * (pix / s - 0.5f);
    float r = ((g + 1.f) * s - 1.f) / 2.f;
    asm("" : "+v"(r));
    return r;
}

// corner (x0, y0) and grid_sampler's weights nw, ne, sw, se = (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy), (x1 - ix)(iy - y0), ...
__device__ __forceinline__ void bw_setup(float px, float py, int W, int H, int (&xy)[2], float (&wgt)[4]) {
    const float ix = bw_coord(px, W), iy = bw_coord(py, H);
    const float fx = floorf(ix), fy = floorf(iy);
    xy[0] = (int)fminf(fmaxf(fx, -2.f), (float)W);             // far outside (or NaN): any corner outside the frame
    xy[1] = (int)fminf(fmaxf(fy, -2.f), (float)H);
    const float ex = fx + 1.f, ey = fy + 1.f;
    wgt[0] = (ex - ix) * (ey - iy);
    wgt[1] = (ix - fx) * (ey - iy);
    wgt[2] = (ex - ix) * (iy - fy);
    wgt[3] = (ix - fx) * (iy - fy);
}

// byte offset of channel 0 of pixel (f, yy, xx), or out of range
template <typename E>
__device__ __forceinline__ unsigned corner_off(int f, int yy, int xx, int H, int W, int ld) {
    const bool in = (unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H;
    return in ? (unsigned)(((f * H + yy) * W + xx) * ld) * (unsigned)sizeof(E) : FLAIR_OOB;
}

// The 8 corners of the two warps: i0 (channels 0-2) at xy0, i1 (channels 3-5) at xy1.  All offsets first, then the loads
// back to back, then ONE empty asm that takes every loaded register: the only wait sits there, behind the last load.  (Left
// to itself hipcc narrowed the loads to the channels used, reshuffled each pair of results with v_mov and waited
// `vmcnt(0)` after every second load: four round trips to memory per pixel.)
template <typename E>
__device__ __forceinline__ void load_corners(__amdgpu_buffer_rsrc_t pr, int f, int H, int W, int ld, const int (&xy0)[2],
                                             const int (&xy1)[2], Px<E, 8> (&cq)[2][4]) {
    unsigned off[2][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        off[0][q] = corner_off<E>(f, xy0[1] + (q >> 1), xy0[0] + (q & 1), H, W, ld);
        off[1][q] = corner_off<E>(f, xy1[1] + (q >> 1), xy1[0] + (q & 1), H, W, ld);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        cq[0][q].load(pr, off[0][q]);
        cq[1][q].load(pr, off[1][q]);
    }
    if constexpr (Px<E, 8>::PIECES == 1)
        asm volatile("" : "+v"(cq[0][0].raw[0]), "+v"(cq[0][1].raw[0]), "+v"(cq[0][2].raw[0]), "+v"(cq[0][3].raw[0]),
                          "+v"(cq[1][0].raw[0]), "+v"(cq[1][1].raw[0]), "+v"(cq[1][2].raw[0]), "+v"(cq[1][3].raw[0]));
    else
        asm volatile("" : "+v"(cq[0][0].raw[0]), "+v"(cq[0][1].raw[0]), "+v"(cq[0][2].raw[0]), "+v"(cq[0][3].raw[0]),
                          "+v"(cq[1][0].raw[0]), "+v"(cq[1][1].raw[0]), "+v"(cq[1][2].raw[0]), "+v"(cq[1][3].raw[0]),
                          "+v"(cq[0][0].raw[1]), "+v"(cq[0][1].raw[1]), "+v"(cq[0][2].raw[1]), "+v"(cq[0][3].raw[1]),
                          "+v"(cq[1][0].raw[1]), "+v"(cq[1][1].raw[1]), "+v"(cq[1][2].raw[1]), "+v"(cq[1][3].raw[1]));
}

template <typename E>
__device__ __forceinline__ void blend_corners(const Px<E, 8> (&cq)[4], const float (&wgt)[4], int c0, float (&g)[3]) {
    float v[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) cq[q].get(v[q]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        g[c] = v[0][c0 + c] * wgt[0] + v[1][c0 + c] * wgt[1] + v[2][c0 + c] * wgt[2] + v[3][c0 + c] * wgt[3];
}

constexpr int SLOMO_IN = 20;            // i0, i1, f01, f10, ft1, ft0, warp(i1, ft1), warp(i0, ft0)
constexpr int SLOMO_IN_MAX = 32;

template <typename E>
__global__ void slomo_warp_pack_kernel(const E* pair, int pairLd, const E* flow, int flowLd, int B, int H, int W, float c0,
                                       float c1, float c2, float c3, E* out, int outLd, int outC) {
    constexpr int VEC = ET<E>::VEC;
    constexpr int FLC = VEC > 4 ? VEC : 4;                      // channels one 16-byte flow load covers
    const unsigned npix = (unsigned)B * H * W;
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(pair, (unsigned)(((size_t)(npix - 1) * pairLd + 8) * sizeof(E)));
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(flow, (unsigned)(((size_t)(npix - 1) * flowLd + FLC) * sizeof(E)));
    const int w = (int)(p % (unsigned)W), h = (int)((p / (unsigned)W) % (unsigned)H), f = (int)(p / ((unsigned)W * H));
    Px<E, 8> own;
    Px<E, 4> ownf;
    own.load(pr, p * (unsigned)pairLd * (unsigned)sizeof(E));
    ownf.load(fr, p * (unsigned)flowLd * (unsigned)sizeof(E));
    float fl[Px<E, 4>::PIECES * VEC];
    ownf.get(fl);
    const float ft0x = c0 * fl[0] + c1 * fl[2], ft0y = c0 * fl[1] + c1 * fl[3];
    const float ft1x = c2 * fl[0] + c3 * fl[2], ft1y = c2 * fl[1] + c3 * fl[3];
    int xy0[2], xy1[2];
    float wg0[4], wg1[4];
    bw_setup((float)w + ft0x, (float)h + ft0y, W, H, xy0, wg0);
    bw_setup((float)w + ft1x, (float)h + ft1y, W, H, xy1, wg1);
    Px<E, 8> cq[2][4];
    load_corners<E>(pr, f, H, W, pairLd, xy0, xy1, cq);
    float g0[3], g1[3], px[Px<E, 8>::PIECES * VEC];
    own.get(px);
    blend_corners<E>(cq[0], wg0, 0, g0);
    blend_corners<E>(cq[1], wg1, 3, g1);
    float v[SLOMO_IN_MAX];
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] = px[c];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[6 + c] = fl[c];
    v[10] = ft1x; v[11] = ft1y; v[12] = ft0x; v[13] = ft0y;
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[14 + c] = g1[c]; v[17 + c] = g0[c]; }
#pragma unroll
    for (int c = SLOMO_IN; c < SLOMO_IN_MAX; ++c) v[c] = 0.f;
    E* o = out + (size_t)p * outLd;
#pragma unroll
    for (int c = 0; c < SLOMO_IN_MAX; c += VEC)
        if (c < outC) Vec16<E>::store(o + c, v + c);
}

template <typename E>
__global__ void slomo_blend_kernel(const E* pair, int pairLd, const E* flow, int flowLd, const E* io, int ioLd, int B, int H,
                                   int W, float c0, float c1, float c2, float c3, float t0, float t1, float m0, float m1,
                                   float m2, float* out, long outBs) {
    constexpr int VEC = ET<E>::VEC;
    constexpr int FLC = VEC > 4 ? VEC : 4;
    const unsigned npix = (unsigned)B * H * W;
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(pair, (unsigned)(((size_t)(npix - 1) * pairLd + 8) * sizeof(E)));
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(flow, (unsigned)(((size_t)(npix - 1) * flowLd + FLC) * sizeof(E)));
    const __amdgpu_buffer_rsrc_t ir = make_rsrc(io, (unsigned)(((size_t)(npix - 1) * ioLd + 8) * sizeof(E)));
    const int w = (int)(p % (unsigned)W), h = (int)((p / (unsigned)W) % (unsigned)H), f = (int)(p / ((unsigned)W * H));
    Px<E, 4> ownf;
    Px<E, 8> owni;
    ownf.load(fr, p * (unsigned)flowLd * (unsigned)sizeof(E));
    owni.load(ir, p * (unsigned)ioLd * (unsigned)sizeof(E));
    float fl[Px<E, 4>::PIECES * VEC], r[Px<E, 8>::PIECES * VEC];
    ownf.get(fl);
    owni.get(r);
    const float ft0x = c0 * fl[0] + c1 * fl[2], ft0y = c0 * fl[1] + c1 * fl[3];
    const float ft1x = c2 * fl[0] + c3 * fl[2], ft1y = c2 * fl[1] + c3 * fl[3];
    int xy0[2], xy1[2];
    float wg0[4], wg1[4];
    bw_setup((float)w + (r[0] + ft0x), (float)h + (r[1] + ft0y), W, H, xy0, wg0);
    bw_setup((float)w + (r[2] + ft1x), (float)h + (r[3] + ft1y), W, H, xy1, wg1);
    Px<E, 8> cq[2][4];
    load_corners<E>(pr, f, H, W, pairLd, xy0, xy1, cq);
    const float v0 = 1.f / (1.f + expf(-r[4]));                 // exp overflows to inf for r[4] < -88.7: v0 = 0, v1 = 1
    const float v1 = 1.f - v0;
    const float a0 = t0 * v0, a1 = t1 * v1;
    const float den = a0 + a1;
    float g0[3], g1[3];
    blend_corners<E>(cq[0], wg0, 0, g0);
    blend_corners<E>(cq[1], wg1, 3, g1);
    const float mean[3] = {m0, m1, m2};
    float* o = out + (size_t)f * outBs + (size_t)h * W + w;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * H * W] = ((a0 * g0[c] + a1 * g1[c]) / den + mean[c]) * 2.f - 1.f;
}

// the size limits both entries share, for elements of esz bytes
int slomo_check(const char* fn, unsigned long long esz, int B, int H, int W, const int* lds, int n) {
    FLAIR_CHECK(B > 0 && H > 0 && W > 0, "%s: bad shape B = %d, H = %d, W = %d", fn, B, H, W);
    const unsigned long long npix = (unsigned long long)B * H * W;
    for (int i = 0; i < n; ++i)
        FLAIR_CHECK(npix < 0x80000000ull && (lds[i] <= 0 || npix * lds[i] * esz < 0x80000000ull),
                    "%s: a clip spans >= 2 GiB (32-bit gather offsets): call with fewer frames", fn);
    return FLAIR_OK;
}

}  // namespace

extern "C" int flair_slomo_warp_pack(const void* pair, int pair_ld, const void* flow, int flow_ld, int dtype, int B, int H,
                                     int W, float c0, float c1, float c2, float c3, void* out, int out_ld, int out_c,
                                     hipStream_t stream) {
    FLAIR_CHECK(pair && flow && out, "flair_slomo_warp_pack: null pointer");
    const int lds[3] = {pair_ld, flow_ld, out_ld};
    return flair_by_dtype("flair_slomo_warp_pack", dtype, [&](auto e) -> int {
        using E = decltype(e);
        constexpr int VEC = ET<E>::VEC;
        if (const int rc = slomo_check("flair_slomo_warp_pack", sizeof(E), B, H, W, lds, 3)) return rc;
        FLAIR_CHECK(out_c >= SLOMO_IN && out_c <= SLOMO_IN_MAX && out_c % VEC == 0,
                    "flair_slomo_warp_pack: out_c = %d must be %d .. %d channels and a multiple of %d", out_c, SLOMO_IN,
                    SLOMO_IN_MAX, VEC);
        FLAIR_CHECK_VIEW("flair_slomo_warp_pack", "pair", pair, pair_ld, 6, VEC);
        FLAIR_CHECK_VIEW("flair_slomo_warp_pack", "flow", flow, flow_ld, 4, VEC);
        FLAIR_CHECK_VIEW("flair_slomo_warp_pack", "out", out, out_ld, out_c, VEC);
        // one thread per pixel, no grid-stride loop: every block
        hipLaunchKernelGGL(slomo_warp_pack_kernel<E>, dim3(grid_for((long)B * H * W, 256, GRID_NO_CAP)), dim3(256), 0, stream,
                           (const E*)pair, pair_ld, (const E*)flow, flow_ld, B, H, W, c0, c1, c2, c3, (E*)out, out_ld, out_c);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}

extern "C" int flair_slomo_blend(const void* pair, int pair_ld, const void* flow, int flow_ld, const void* io, int io_ld,
                                 int dtype, int B, int H, int W, float c0, float c1, float c2, float c3, double t,
                                 const float* mean, float* out, long out_batch_stride, hipStream_t stream) {
    FLAIR_CHECK(pair && flow && io && out && mean, "flair_slomo_blend: null pointer");
    const int lds[3] = {pair_ld, flow_ld, io_ld};
    return flair_by_dtype("flair_slomo_blend", dtype, [&](auto e) -> int {
        using E = decltype(e);
        constexpr int VEC = ET<E>::VEC;
        if (const int rc = slomo_check("flair_slomo_blend", sizeof(E), B, H, W, lds, 3)) return rc;
        FLAIR_CHECK(t > 0.0 && t < 1.0, "flair_slomo_blend: t = %g is not inside (0, 1)", t);
        FLAIR_CHECK_VIEW("flair_slomo_blend", "pair", pair, pair_ld, 6, VEC);
        FLAIR_CHECK_VIEW("flair_slomo_blend", "flow", flow, flow_ld, 4, VEC);
        FLAIR_CHECK_VIEW("flair_slomo_blend", "io", io, io_ld, 5, VEC);
        // not FLAIR_CHECK_VIEW: out is planar f32, written one float at a time
        FLAIR_CHECK(out_batch_stride >= 3L * H * W && reinterpret_cast<uintptr_t>(out) % 4 == 0,
                    "flair_slomo_blend: out_batch_stride = %ld must be >= 3 H W = %ld floats, out = %p 4-byte aligned",
                    out_batch_stride, 3L * H * W, (const void*)out);
        const float t0 = (float)(1.0 - t), t1 = (float)t;            // co_eff = [1 - t, t]: Python doubles, cast by the multiply
        // one thread per pixel, no grid-stride loop: every block
        hipLaunchKernelGGL(slomo_blend_kernel<E>, dim3(grid_for((long)B * H * W, 256, GRID_NO_CAP)), dim3(256), 0, stream,
                           (const E*)pair, pair_ld, (const E*)flow, flow_ld, (const E*)io, io_ld, B, H, W, c0, c1, c2, c3, t0, t1,
                           mean[0], mean[1], mean[2], out, out_batch_stride);
        FLAIR_LAUNCH_CHECK();
        return FLAIR_OK;
    });
}
