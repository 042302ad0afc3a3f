// The pieces of AMT-G (guided_diffusion/amt.py, amt_blocks/) that the library lacked, all f32:
//
//  * flair_corr_scale         -- `corr / sqrt(dim)` of BidirCorrBlock.corr (raft.py:209), in place on the flair_matmul_f32
//                                product: a true division, as the reference does it (x * (1 / d) rounds differently).
//  * flair_corr_pool          -- one level of the correlation pyramid from the previous one, F.avg_pool2d(., 2, stride=2)
//                                over the B h w planes of a volume (raft.py:159-163); odd sizes floor.
//  * flair_corr_lookup        -- BidirCorrBlock.__call__ (raft.py:165-199) with the coordinates of AMT._corr_scale_lookup
//                                (amt.py:98-111): per query pixel and direction, levels x 49 bilinear samples of that query's
//                                planes, written straight into the NHWC input segment of convc1.
//  * flair_prelu_nhwc         -- nn.PReLU(C) on x0 (+ x1): convrelu and ResBlock's prelu(x + out) (ifrnet.py:10-14, :52).
//  * flair_axpby_nhwc         -- a x0 + b x1 on channel views: `delta + 2.0 * resize(flow, 2.0)` (ifrnet.py:109-110),
//                                `flow + scale_factor * resize(delta_flow)` (raft.py:138, amt.py:161-162), each product rounded.
//  * flair_amt_multiflow_prepare / flair_amt_multiflow_combine -- the tail: MultiFlowDecoder.forward behind its convblock
//                                (multi_flow.py:73-83) and multi_flow_combine up to comb_block (:27-54), one thread per pixel.
//  * flair_instnorm_nhwc      -- nn.InstanceNorm2d (+ ReLU) of the feature encoder (feat_enc.py:86-114), two-pass.
//  * flair_depth_to_space2_nhwc -- the second half of ConvTranspose2d(4, 2, 1) (ifrnet.py:84, :100; multi_flow.py:65) run as
//                                a 3x3 convolution with 4 Cout outputs: output parity (py, px) of pixel (2m + py, 2n + px)
//                                sits in channels [(2 py + px) C, (2 py + px + 1) C) of pixel (m, n).
//
// The lookup.  One wave per (query pixel, direction); the four waves of a workgroup take two neighbouring queries.  A
// level's 7 x 7 taps sit at centre / 2^l + (a - 3, b - 3): they share one fractional part, so their 4 x 49 bilinear corners
// are the 8 x 8 patch whose top-left is floor(centre / 2^l) - 3.  Lane p loads corner (p % 8, p / 8) of the patch (zero
// outside the plane: the `zeros` rule of grid_sample), one 4-byte load per lane and level instead of four; lane t < 49 then
// takes its four corners from the patch by ds_bpermute and blends them.  A query's plane is contiguous (h2 w2 floats), so a
// patch row is one 32-byte run; the 49 results of a level are one 196-byte run of the destination pixel.  Tap t = 7 a + b
// moves x by a - 3 and y by b - 3: the reference stacks meshgrid(dy, dx) and adds it to (x, y) (raft.py:177-184), so the
// FIRST tap axis moves x.  A level whose plane is 1 x 1 gives its one value to every tap (raft.py:186-188).
//
// Coordinates.  centre = (x, y) + flow * scale, / 2^l, + delta: each step rounded to f32 as in the reference, which is why
// the Makefile compiles this file with -ffp-contract=off (as slomo.hip).  bilinear_sampler then maps the pixel coordinate
// to [-1, 1] and grid_sample (align_corners=True) maps it back (raft.py:14-15): the identity in exact arithmetic and not
// repeated here, so an integer coordinate returns the volume entry itself, bit for bit; the reference's round trip moves a
// coordinate by a few 2^-24 of its size, which a bilinear sample with zero padding (continuous everywhere) follows by as
// little.  Weights and the four-term sum are grid_sampler's: nw = (x1 - ix)(y1 - iy), ne = (ix - x0)(y1 - iy), ...
//
// Offsets are 64-bit throughout: at 512 x 512 one direction of level 0 is 4096 planes of 4096 floats (64 MiB), and a batch
// of 32 such pairs passes 2^31 bytes.
#include "common.h"

namespace {

constexpr int CORR_TAPS = 49;           // (2 r + 1)^2 at the radius 3 AMT uses
constexpr int CORR_MAX_LEVELS = 4;

__global__ void corr_scale_kernel(float* x, long n4, long n, float d) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        float4 v = reinterpret_cast<float4*>(x)[i];
        v.x /= d; v.y /= d; v.z /= d; v.w /= d;
        reinterpret_cast<float4*>(x)[i] = v;
    } else if (i - n4 < n - 4 * n4) {
        x[4 * n4 + (i - n4)] /= d;
    }
}

__global__ void corr_pool_kernel(const float* src, long planes, int h, int w, float* dst) {
    const int ho = h >> 1, wo = w >> 1;
    const long total = planes * ho * wo;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % wo), y = (int)((i / wo) % ho);
    const long p = i / ((long)wo * ho);
    const float* s = src + (p * h + 2 * y) * (long)w + 2 * x;
    dst[i] = (((s[0] + s[1]) + s[w]) + s[w + 1]) * 0.25f;      // ATen's avg_pool2d: row-major sum, then / 4
}

struct CorrLevels {
    const float* plane[2][CORR_MAX_LEVELS];     // [direction][level]: B h w planes of lh x lw floats
    int lh[CORR_MAX_LEVELS], lw[CORR_MAX_LEVELS];
};

__global__ __launch_bounds__(256) void corr_lookup_kernel(CorrLevels L, int levels, const float* flow, int flowLd, long nq,
                                                          int h1, int w1, float scale0, float scale1, float* out, int outLd) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);        // (query, direction), wave-uniform
    if (item >= 2 * nq) return;
    const long q = item >> 1;
    const int dir = (int)(item & 1);
    const int qx = (int)(q % w1), qy = (int)((q / w1) % h1);
    // corr (direction 0) is read at coord + flow1 / t, corr_T at coord + flow0 / (1 - t)  (amt.py:108)
    const float* f = flow + q * flowLd + (dir == 0 ? 2 : 0);
    const float sc = dir == 0 ? scale0 : scale1;
    const float cx = (float)qx + f[0] * sc, cy = (float)qy + f[1] * sc;
    float* o = out + q * outLd + dir * levels * CORR_TAPS;
    const int a = lane / 7, b = lane % 7;                               // tap, lanes 0 .. 48
    const int px = lane & 7, py = lane >> 3;                            // patch corner, all 64 lanes
    float inv = 1.f;
    for (int l = 0; l < levels; ++l, inv *= 0.5f) {
        const int H = L.lh[l], W = L.lw[l];
        const float* plane = L.plane[dir][l] + q * ((long)H * W);
        float val;
        if (H == 1 && W == 1) {
            val = plane[0];
        } else {
            const float lx = cx * inv, ly = cy * inv;                   // centroid / 2^l: exact
            const float bxf = floorf(lx) - 3.f, byf = floorf(ly) - 3.f;
            // a patch further out than this has no corner inside the plane wherever it is (NaN lands at -12 as well)
            const int bx = (int)fminf(fmaxf(bxf, -12.f), (float)W + 4.f), by = (int)fminf(fmaxf(byf, -12.f), (float)H + 4.f);
            const int xx = bx + px, yy = by + py;
            float v = 0.f;
            if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H) v = plane[(long)yy * W + xx];
            const float ix = lx + (float)(a - 3), iy = ly + (float)(b - 3);
            const float x0 = floorf(ix), y0 = floorf(iy);
            // column of x0 in the patch: a, or a + 1 when the sum rounded up to the next integer (then ix - x0 = 0 and the
            // corner to its right, which may be column 8, weighs nothing: column 7 stands in for it)
            const int rx = (int)fminf(fmaxf(x0 - bxf, 0.f), 7.f), ry = (int)fminf(fmaxf(y0 - byf, 0.f), 7.f);
            const int rx1 = rx < 7 ? rx + 1 : 7, ry1 = ry < 7 ? ry + 1 : 7;
            const float nw = __shfl(v, ry * 8 + rx), ne = __shfl(v, ry * 8 + rx1);
            const float sw = __shfl(v, ry1 * 8 + rx), se = __shfl(v, ry1 * 8 + rx1);
            const float x1 = x0 + 1.f, y1 = y0 + 1.f;
            val = nw * ((x1 - ix) * (y1 - iy)) + ne * ((ix - x0) * (y1 - iy)) + sw * ((x1 - ix) * (iy - y0)) +
                  se * ((ix - x0) * (iy - y0));
        }
        if (lane < CORR_TAPS) o[l * CORR_TAPS + lane] = val;
    }
}

__global__ void prelu_kernel(const float* x0, int ld0, const float* x1, int ld1, const float* slope, int C, long P, float* y,
                             int yLd) {
    const int c4 = C >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * c4) return;
    const long p = i / c4;
    const int c = (int)(i % c4) * 4;
    float4 v = *reinterpret_cast<const float4*>(x0 + p * ld0 + c);
    if (x1) {
        const float4 u = *reinterpret_cast<const float4*>(x1 + p * ld1 + c);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    const float4 s = *reinterpret_cast<const float4*>(slope + c);
    v.x = v.x > 0.f ? v.x : s.x * v.x;
    v.y = v.y > 0.f ? v.y : s.y * v.y;
    v.z = v.z > 0.f ? v.z : s.z * v.z;
    v.w = v.w > 0.f ? v.w : s.w * v.w;
    *reinterpret_cast<float4*>(y + p * yLd + c) = v;
}

__global__ void depth_to_space2_kernel(const float* x, int xLd, long F, int H, int W, int C, float* y, int yLd) {
    const int c4 = C >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // one 16-byte piece of one OUTPUT pixel
    if (i >= F * 4 * H * W * c4) return;
    const int c = (int)(i % c4) * 4;
    const long op = i / c4;
    const int ox = (int)(op % (2 * W)), oy = (int)((op / (2 * W)) % (2 * H));
    const long f = op / ((long)4 * H * W);
    const long ip = (f * H + (oy >> 1)) * W + (ox >> 1);
    const int par = (oy & 1) * 2 + (ox & 1);
    *reinterpret_cast<float4*>(y + op * yLd + c) = *reinterpret_cast<const float4*>(x + ip * xLd + par * C + c);
}

__global__ void axpby_nhwc_kernel(const float* x0, int ld0, float a, const float* x1, int ld1, float b, int C, long P, float* y,
                                  int yLd) {
    const int c4 = C >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * c4) return;
    const long p = i / c4;
    const int c = (int)(i % c4) * 4;
    float4 v = *reinterpret_cast<const float4*>(x0 + p * ld0 + c);
    v.x *= a; v.y *= a; v.z *= a; v.w *= a;
    if (x1) {
        const float4 u = *reinterpret_cast<const float4*>(x1 + p * ld1 + c);
        v.x += b * u.x; v.y += b * u.y; v.z += b * u.z; v.w += b * u.w;
    }
    *reinterpret_cast<float4*>(y + p * yLd + c) = v;
}

constexpr int MF_N = 5;                 // num_flows of AMT-G
constexpr int MF_C = 8 * MF_N;          // delta_flow0 (2 n) | delta_flow1 (2 n) | mask (n) | img_res (3 n)

// MultiFlowDecoder.forward after its convblock (multi_flow.py:73-83): one thread per pixel.
__global__ void multiflow_prepare_kernel(const float* dec, int decLd, const float* up, int upLd, long P, float* out, int outLd) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const float* d = dec + p * decLd;
    const float4 u = *reinterpret_cast<const float4*>(up + p * upLd);      // resize(flow0 | flow1, 2.0)
    const float u2[4] = {2.f * u.x, 2.f * u.y, 2.f * u.z, 2.f * u.w};
    float v[MF_C];
#pragma unroll
    for (int c = 0; c < MF_C; c += 4) {
        const float4 t = *reinterpret_cast<const float4*>(d + c);
        v[c] = t.x; v[c + 1] = t.y; v[c + 2] = t.z; v[c + 3] = t.w;
    }
#pragma unroll
    for (int c = 0; c < 4 * MF_N; ++c) v[c] = v[c] + u2[(c & 1) + (c >= 2 * MF_N ? 2 : 0)];
#pragma unroll
    for (int c = 4 * MF_N; c < 5 * MF_N; ++c) v[c] = 1.f / (1.f + expf(-v[c]));
    float* o = out + p * outLd;
#pragma unroll
    for (int c = 0; c < MF_C; c += 4) *reinterpret_cast<float4*>(o + c) = make_float4(v[c], v[c + 1], v[c + 2], v[c + 3]);
}

// flow_utils.warp of a 3-channel image held in channels c0 .. c0 + 2 of `pair`: bilinear, border, align_corners=True
__device__ __forceinline__ void border_warp3(const float* pair, int pairLd, long frameBase, int H, int W, int c0, float px, float py,
                                             float (&g)[3]) {
    const float ix = fminf(fmaxf(px, 0.f), (float)(W - 1)), iy = fminf(fmaxf(py, 0.f), (float)(H - 1));
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;     // past the edge: weight 0
    const float ex = x0f + 1.f, ey = y0f + 1.f;
    const float wnw = (ex - ix) * (ey - iy), wne = (ix - x0f) * (ey - iy), wsw = (ex - ix) * (iy - y0f), wse = (ix - x0f) * (iy - y0f);
    const float* nw = pair + (frameBase + (long)y0 * W + x0) * pairLd + c0;
    const float* ne = pair + (frameBase + (long)y0 * W + x1) * pairLd + c0;
    const float* sw = pair + (frameBase + (long)y1 * W + x0) * pairLd + c0;
    const float* se = pair + (frameBase + (long)y1 * W + x1) * pairLd + c0;
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = nw[c] * wnw + ne[c] * wne + sw[c] * wsw + se[c] * wse;
}

// multi_flow_combine up to comb_block (multi_flow.py:27-54): the 2 n warps, the mask blend, + mean + img_res, the n
// predictions as comb_block's 3 n-channel input (zero-padded to 16) and their mean over n.
__global__ void multiflow_combine_kernel(const float* pair, int pairLd, const float* prep, int prepLd, const float* negMean,
                                         int negMeanLd, int B, int H, int W, float* x, int xLd, float* avg, int avgLd) {
    const long P = (long)B * H * W;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int w = (int)(p % W), h = (int)((p / W) % H);
    const long f = p / ((long)W * H);
    const float* r = prep + p * prepLd;
    float v[MF_C];
#pragma unroll
    for (int c = 0; c < MF_C; c += 4) {
        const float4 t = *reinterpret_cast<const float4*>(r + c);
        v[c] = t.x; v[c + 1] = t.y; v[c + 2] = t.z; v[c + 3] = t.w;
    }
    const float mean = -negMean[f * negMeanLd];
    float o[16], s[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < MF_N; ++i) {
        float g0[3], g1[3];
        border_warp3(pair, pairLd, f * H * W, H, W, 0, (float)w + v[2 * i], (float)h + v[2 * i + 1], g0);
        border_warp3(pair, pairLd, f * H * W, H, W, 3, (float)w + v[2 * MF_N + 2 * i], (float)h + v[2 * MF_N + 2 * i + 1], g1);
        const float m = v[4 * MF_N + i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = m * g0[c] + (1.f - m) * g1[c] + mean + v[5 * MF_N + 3 * i + c];
            o[3 * i + c] = t;
            s[c] = i == 0 ? t : s[c] + t;
        }
    }
    o[15] = 0.f;
    float* xo = x + p * xLd;
#pragma unroll
    for (int c = 0; c < 16; c += 4) *reinterpret_cast<float4*>(xo + c) = make_float4(o[c], o[c + 1], o[c + 2], o[c + 3]);
    *reinterpret_cast<float4*>(avg + p * avgLd) = make_float4(s[0] / (float)MF_N, s[1] / (float)MF_N, s[2] / (float)MF_N, 0.f);
}

// InstanceNorm2d (no affine) + activation, two-pass: per (frame, channel) the mean, then the variance of the CENTRED values,
// both summed in double over fixed pixel ranges in a fixed order (no atomics: the same bits in every run), then
// y = act((x - mean) * rstd).  flair_groupnorm_nhwc with one group per channel takes var = E[x^2] - mean^2, which at the 4 x 4
// and 16 x 18 maps of the feature encoder missed 4 x the f32 ATen deviation by a factor of four on planes with a mean of a
// few standard deviations; gn.hip is the benchmark's and stays as it is.
constexpr int IN_MAX_SPLIT = 64;

inline int in_split(long HW) { return (int)(HW <= 512 ? 1 : (HW / 512 > IN_MAX_SPLIT ? IN_MAX_SPLIT : HW / 512)); }

// grid (ceil(C / 64), S, F), 256 threads = 64 channels x 4 pixel phases; mean == NULL: sums of x, else of (x - mean)^2
__global__ __launch_bounds__(256) void in_partial_kernel(const float* x, int ld, int HW, int C, int S, const float* mean,
                                                         double* partial) {
    __shared__ double sh[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), pg = threadIdx.x >> 6;
    const int s = blockIdx.y;
    const long f = blockIdx.z;
    const int chunk = (HW + S - 1) / S, p0 = s * chunk, p1 = p0 + chunk < HW ? p0 + chunk : HW;
    double acc = 0.0;
    if (c < C) {
        const float m = mean ? mean[f * C + c] : 0.f;
        for (int p = p0 + pg; p < p1; p += 4) {
            const float v = x[(f * HW + p) * ld + c] - m;
            acc += mean ? (double)v * (double)v : (double)v;
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (pg == 0 && c < C)
        partial[(f * S + s) * C + c] = ((sh[threadIdx.x] + sh[threadIdx.x + 64]) + sh[threadIdx.x + 128]) + sh[threadIdx.x + 192];
}

__global__ void in_finish_kernel(const double* partial, long F, int C, int S, int HW, double eps, int second, float* stat) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * C) return;
    const long f = i / C;
    const int c = (int)(i % C);
    double t = 0.0;
    for (int s = 0; s < S; ++s) t += partial[(f * S + s) * C + c];
    t /= (double)HW;
    stat[i] = second ? (float)(1.0 / sqrt(t + eps)) : (float)t;
}

__global__ void in_apply_kernel(const float* x, int ld, long F, int HW, int C, const float* mean, const float* rstd, int relu,
                                float* y, int yLd) {
    const int c4 = C >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * HW * c4) return;
    const long p = i / c4;
    const int c = (int)(i % c4) * 4;
    const long f = p / HW;
    const float4 v = *reinterpret_cast<const float4*>(x + p * ld + c);
    const float4 m = *reinterpret_cast<const float4*>(mean + f * C + c), r = *reinterpret_cast<const float4*>(rstd + f * C + c);
    float4 o = make_float4((v.x - m.x) * r.x, (v.y - m.y) * r.y, (v.z - m.z) * r.z, (v.w - m.w) * r.w);
    if (relu) {
        o.x = o.x > 0.f ? o.x : 0.f; o.y = o.y > 0.f ? o.y : 0.f; o.z = o.z > 0.f ? o.z : 0.f; o.w = o.w > 0.f ? o.w : 0.f;
    }
    *reinterpret_cast<float4*>(y + p * yLd + c) = o;
}

}  // namespace

extern "C" int flair_corr_scale(float* x, long n, float divisor, hipStream_t stream) {
    FLAIR_CHECK(x && n > 0, "flair_corr_scale: bad argument (x = %p, n = %ld)", (const void*)x, n);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(x) % 16 == 0, "flair_corr_scale: x = %p must be 16-byte aligned", (const void*)x);
    FLAIR_CHECK(divisor > 0.f && divisor < INFINITY, "flair_corr_scale: divisor = %g must be positive and finite", divisor);
    const long n4 = n / 4, threads = n4 + (n - 4 * n4);
    FLAIR_CHECK(threads <= 0x7fffffffL * 256, "flair_corr_scale: n = %ld needs more than 2^31 workgroups", n);
    hipLaunchKernelGGL(corr_scale_kernel, dim3(grid_for(threads, 256, GRID_NO_CAP)), dim3(256), 0, stream, x, n4, n, divisor);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_corr_pool(const float* src, long planes, int h, int w, float* dst, hipStream_t stream) {
    FLAIR_CHECK(src && dst, "flair_corr_pool: null pointer");
    FLAIR_CHECK(planes > 0 && h >= 2 && w >= 2, "flair_corr_pool: planes = %ld of h = %d x w = %d: at least one 2 x 2 window each",
                planes, h, w);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0,
                "flair_corr_pool: src = %p and dst = %p must be 4-byte aligned", (const void*)src, (const void*)dst);
    const long total = planes * (h / 2) * (w / 2);
    FLAIR_CHECK(total <= 0x7fffffffL * 256, "flair_corr_pool: %ld outputs need more than 2^31 workgroups", total);
    hipLaunchKernelGGL(corr_pool_kernel, dim3(grid_for(total, 256, GRID_NO_CAP)), dim3(256), 0, stream, src, planes, h, w, dst);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_corr_lookup(const float* const* corr, const float* const* corr_t, const int* level_h, const int* level_w,
                                 int levels, const float* flow, int flow_ld, int B, int h, int w, float scale_corr,
                                 float scale_corr_t, float* out, int out_ld, hipStream_t stream) {
    FLAIR_CHECK(corr && corr_t && level_h && level_w && flow && out, "flair_corr_lookup: null pointer");
    FLAIR_CHECK(levels >= 1 && levels <= CORR_MAX_LEVELS, "flair_corr_lookup: levels = %d must be 1 .. %d", levels, CORR_MAX_LEVELS);
    FLAIR_CHECK(B > 0 && h > 0 && w > 0, "flair_corr_lookup: bad shape B = %d, h = %d, w = %d", B, h, w);
    FLAIR_CHECK(flow_ld >= 4 && flow_ld % 4 == 0 && reinterpret_cast<uintptr_t>(flow) % 16 == 0,
                "flair_corr_lookup: flow stride/alignment: flow_ld = %d must be >= 4 and a multiple of 4 floats, flow = %p "
                "16-byte aligned", flow_ld, (const void*)flow);
    FLAIR_CHECK(out_ld >= 2 * levels * CORR_TAPS && reinterpret_cast<uintptr_t>(out) % 4 == 0,
                "flair_corr_lookup: out stride/alignment: out_ld = %d must be >= 2 * levels * 49 = %d floats, out = %p 4-byte "
                "aligned", out_ld, 2 * levels * CORR_TAPS, (const void*)out);
    CorrLevels L = {};
    for (int l = 0; l < levels; ++l) {
        FLAIR_CHECK(corr[l] && corr_t[l], "flair_corr_lookup: null plane pointer at level %d", l);
        FLAIR_CHECK(reinterpret_cast<uintptr_t>(corr[l]) % 4 == 0 && reinterpret_cast<uintptr_t>(corr_t[l]) % 4 == 0,
                    "flair_corr_lookup: corr[%d] = %p and corr_t[%d] = %p must be 4-byte aligned", l, (const void*)corr[l], l,
                    (const void*)corr_t[l]);
        // raft.py:186-191: a plane is sampled when both sides are >= 2 and repeated when it is 1 x 1; the reference raises
        // on anything else
        FLAIR_CHECK((level_h[l] >= 2 && level_w[l] >= 2) || (level_h[l] == 1 && level_w[l] == 1),
                    "flair_corr_lookup: level %d planes of %d x %d: both sides >= 2, or 1 x 1", l, level_h[l], level_w[l]);
        L.plane[0][l] = corr[l];
        L.plane[1][l] = corr_t[l];
        L.lh[l] = level_h[l];
        L.lw[l] = level_w[l];
    }
    const long nq = (long)B * h * w, blocks = (2 * nq + 3) / 4;
    FLAIR_CHECK(blocks <= 0x7fffffffL, "flair_corr_lookup: %ld queries need more than 2^31 workgroups", nq);
    hipLaunchKernelGGL(corr_lookup_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, L, levels, flow, flow_ld, nq, h, w,
                       scale_corr, scale_corr_t, out, out_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_prelu_nhwc(const float* x0, int x0_ld, const float* x1, int x1_ld, const float* slope, int C, long P,
                                float* y, int y_ld, hipStream_t stream) {
    FLAIR_CHECK(x0 && slope && y && C > 0 && P > 0, "flair_prelu_nhwc: bad argument");
    FLAIR_CHECK(C % 4 == 0, "flair_prelu_nhwc: C = %d must be a multiple of 4", C);
    FLAIR_CHECK_VIEW("flair_prelu_nhwc", "x0", x0, x0_ld, C, 4);
    if (x1) FLAIR_CHECK_VIEW("flair_prelu_nhwc", "x1", x1, x1_ld, C, 4);
    FLAIR_CHECK_VIEW("flair_prelu_nhwc", "y", y, y_ld, C, 4);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(slope) % 16 == 0, "flair_prelu_nhwc: slope = %p must be 16-byte aligned",
                (const void*)slope);
    const long n = P * (C / 4);
    FLAIR_CHECK(n <= 0x7fffffffL * 256, "flair_prelu_nhwc: P = %ld pixels of %d channels need more than 2^31 workgroups", P, C);
    hipLaunchKernelGGL(prelu_kernel, dim3(grid_for(n, 256, GRID_NO_CAP)), dim3(256), 0, stream, x0, x0_ld, x1, x1_ld, slope, C, P, y, y_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_depth_to_space2_nhwc(const float* x, int x_ld, int F, int H, int W, int C, float* y, int y_ld,
                                          hipStream_t stream) {
    FLAIR_CHECK(x && y && F > 0 && H > 0 && W > 0 && C > 0, "flair_depth_to_space2_nhwc: bad argument");
    FLAIR_CHECK(C % 4 == 0, "flair_depth_to_space2_nhwc: C = %d must be a multiple of 4", C);
    FLAIR_CHECK_VIEW("flair_depth_to_space2_nhwc", "x", x, x_ld, 4 * C, 4);
    FLAIR_CHECK_VIEW("flair_depth_to_space2_nhwc", "y", y, y_ld, C, 4);
    const long n = (long)F * 4 * H * W * (C / 4);
    FLAIR_CHECK(n <= 0x7fffffffL * 256, "flair_depth_to_space2_nhwc: more than 2^31 workgroups");
    hipLaunchKernelGGL(depth_to_space2_kernel, dim3(grid_for(n, 256, GRID_NO_CAP)), dim3(256), 0, stream, x, x_ld, (long)F, H, W, C, y, y_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_axpby_nhwc(const float* x0, int x0_ld, float a, const float* x1, int x1_ld, float b, int C, long P, float* y,
                                int y_ld, hipStream_t stream) {
    FLAIR_CHECK(x0 && y && C > 0 && P > 0, "flair_axpby_nhwc: bad argument");
    FLAIR_CHECK(C % 4 == 0, "flair_axpby_nhwc: C = %d must be a multiple of 4", C);
    FLAIR_CHECK_VIEW("flair_axpby_nhwc", "x0", x0, x0_ld, C, 4);
    if (x1) FLAIR_CHECK_VIEW("flair_axpby_nhwc", "x1", x1, x1_ld, C, 4);
    FLAIR_CHECK_VIEW("flair_axpby_nhwc", "y", y, y_ld, C, 4);
    const long n = P * (C / 4);
    FLAIR_CHECK(n <= 0x7fffffffL * 256, "flair_axpby_nhwc: more than 2^31 workgroups");
    hipLaunchKernelGGL(axpby_nhwc_kernel, dim3(grid_for(n, 256, GRID_NO_CAP)), dim3(256), 0, stream, x0, x0_ld, a, x1, x1_ld, b, C, P, y, y_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_amt_multiflow_prepare(const float* dec, int dec_ld, const float* up, int up_ld, long P, float* out,
                                           int out_ld, hipStream_t stream) {
    FLAIR_CHECK(dec && up && out && P > 0, "flair_amt_multiflow_prepare: bad argument");
    FLAIR_CHECK_VIEW("flair_amt_multiflow_prepare", "dec", dec, dec_ld, MF_C, 4);
    FLAIR_CHECK_VIEW("flair_amt_multiflow_prepare", "up", up, up_ld, 4, 4);
    FLAIR_CHECK_VIEW("flair_amt_multiflow_prepare", "out", out, out_ld, MF_C, 4);
    FLAIR_CHECK(P <= 0x7fffffffL * 256, "flair_amt_multiflow_prepare: more than 2^31 workgroups");
    hipLaunchKernelGGL(multiflow_prepare_kernel, dim3(grid_for(P, 256, GRID_NO_CAP)), dim3(256), 0, stream, dec, dec_ld, up, up_ld, P, out, out_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_amt_multiflow_combine(const float* pair, int pair_ld, const float* prep, int prep_ld, const float* neg_mean,
                                           int neg_mean_ld, int B, int H, int W, float* x, int x_ld, float* avg, int avg_ld,
                                           hipStream_t stream) {
    FLAIR_CHECK(pair && prep && neg_mean && x && avg, "flair_amt_multiflow_combine: null pointer");
    FLAIR_CHECK(B > 0 && H > 0 && W > 0 && neg_mean_ld >= 1, "flair_amt_multiflow_combine: bad shape B = %d, H = %d, W = %d", B, H, W);
    FLAIR_CHECK_VIEW("flair_amt_multiflow_combine", "pair", pair, pair_ld, 6, 4);
    FLAIR_CHECK_VIEW("flair_amt_multiflow_combine", "prep", prep, prep_ld, MF_C, 4);
    FLAIR_CHECK_VIEW("flair_amt_multiflow_combine", "x", x, x_ld, 16, 4);
    FLAIR_CHECK_VIEW("flair_amt_multiflow_combine", "avg", avg, avg_ld, 4, 4);
    const long P = (long)B * H * W;
    FLAIR_CHECK(P <= 0x7fffffffL * 256, "flair_amt_multiflow_combine: more than 2^31 workgroups");
    hipLaunchKernelGGL(multiflow_combine_kernel, dim3(grid_for(P, 256, GRID_NO_CAP)), dim3(256), 0, stream, pair, pair_ld, prep, prep_ld, neg_mean,
                       neg_mean_ld, B, H, W, x, x_ld, avg, avg_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" size_t flair_instnorm_workspace_bytes(int F, int H, int W, int C) {
    if (F <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    const long HW = (long)H * W;
    return ((size_t)F * in_split(HW) * C) * sizeof(double) + (size_t)2 * F * C * sizeof(float);
}

extern "C" int flair_instnorm_nhwc(const float* x, int x_ld, int F, int H, int W, int C, double eps, int act, float* y, int y_ld,
                                   void* workspace, size_t workspace_bytes, hipStream_t stream) {
    FLAIR_CHECK(x && y && workspace, "flair_instnorm_nhwc: null pointer");
    FLAIR_CHECK(F > 0 && F <= 65535 && H > 0 && W > 0 && C > 0 && (long)H * W < 0x7fffffffL,
                "flair_instnorm_nhwc: bad shape F = %d (at most 65535), H = %d, W = %d, C = %d", F, H, W, C);
    FLAIR_CHECK(C % 4 == 0, "flair_instnorm_nhwc: C = %d must be a multiple of 4", C);
    FLAIR_CHECK(act == FLAIR_ACT_NONE || act == FLAIR_ACT_RELU, "flair_instnorm_nhwc: activation %d (none or ReLU)", act);
    FLAIR_CHECK(eps >= 0.0, "flair_instnorm_nhwc: eps = %g", eps);
    FLAIR_CHECK_VIEW("flair_instnorm_nhwc", "x", x, x_ld, C, 4);
    FLAIR_CHECK_VIEW("flair_instnorm_nhwc", "y", y, y_ld, C, 4);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(workspace) % 16 == 0 && workspace_bytes >= flair_instnorm_workspace_bytes(F, H, W, C),
                "flair_instnorm_nhwc: workspace = %p must be 16-byte aligned and hold %zu bytes (got %zu)", workspace,
                flair_instnorm_workspace_bytes(F, H, W, C), workspace_bytes);
    const int HW = H * W, S = in_split(HW);
    double* partial = static_cast<double*>(workspace);
    float* mean = reinterpret_cast<float*>(partial + (size_t)F * S * C);
    float* rstd = mean + (size_t)F * C;
    const dim3 grid((C + 63) / 64, S, F);
    const long n = (long)F * HW * (C / 4);
    FLAIR_CHECK(n <= 0x7fffffffL * 256, "flair_instnorm_nhwc: more than 2^31 workgroups");
    hipLaunchKernelGGL(in_partial_kernel, grid, dim3(256), 0, stream, x, x_ld, HW, C, S, (const float*)nullptr, partial);
    hipLaunchKernelGGL(in_finish_kernel, dim3(grid_for((long)F * C, 256, GRID_NO_CAP)), dim3(256), 0, stream, partial, (long)F, C, S, HW, eps, 0, mean);
    hipLaunchKernelGGL(in_partial_kernel, grid, dim3(256), 0, stream, x, x_ld, HW, C, S, (const float*)mean, partial);
    hipLaunchKernelGGL(in_finish_kernel, dim3(grid_for((long)F * C, 256, GRID_NO_CAP)), dim3(256), 0, stream, partial, (long)F, C, S, HW, eps, 1, rstd);
    hipLaunchKernelGGL(in_apply_kernel, dim3(grid_for(n, 256, GRID_NO_CAP)), dim3(256), 0, stream, x, x_ld, (long)F, HW, C, mean, rstd,
                       act == FLAIR_ACT_RELU ? 1 : 0, y, y_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
