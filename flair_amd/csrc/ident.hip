// ArcFace identity, the two kernels of its own: flair_ident_prepare, flair_ident_embed (include/flair_ident.h, which holds
// the definition and both entries' contracts).  The network's convolutions, PReLUs, BatchNorm and pool are entries of
// flair_hip.h; f32 in and out, float64 inside.
//
//   prepare   four lanes own one output pixel: lane 0 of them reads the four taps (12 bytes, one by one: any alignment), makes
//             the grey values and the bilinear mix in double and writes channels 0 .. 3; the other three write the zero channels.
//   embed     a workgroup owns 16 output rows, up to 16 frames and one chunk of the inputs, a quarter of it per wave; a wave
//             adds 16 x 16 x 4 products per float64 matrix instruction into four accumulator registers per lane (see below),
//             the four waves' tiles are added in wave order through 8 KiB of LDS.  One partial per (chunk, f, o); a second
//             launch adds a cell's partials in ascending order: no atomics.
#include "common.h"

#include "../../include/flair_ident.h"

namespace {
constexpr int ID_THREADS = 256;
constexpr int ID_SIDE = FLAIR_IDENT_SIDE;

// ---- prepare ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double gray_of(const uint8_t* p) {
    const double r = 2.0 * (double)p[0] / 255.0 - 1.0, g = 2.0 * (double)p[1] / 255.0 - 1.0, b = 2.0 * (double)p[2] / 255.0 - 1.0;
    return 0.2989 * r + 0.5870 * g + 0.1140 * b;
}

// source position of output index d on an axis of n pixels: i0, i1 and the weight of i1
__device__ __forceinline__ void tap_of(int d, int n, int& i0, int& i1, double& l1) {
    double src = ((double)d + 0.5) * ((double)n / (double)ID_SIDE) - 0.5;
    if (src < 0.0) src = 0.0;
    i0 = (int)src;
    if (i0 > n - 1) i0 = n - 1;
    i1 = i0 < n - 1 ? i0 + 1 : i0;
    l1 = src - (double)i0;
}

__global__ __launch_bounds__(ID_THREADS) void ident_prepare_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int N,
                                                                    int H, int W, float* __restrict__ y, int y_ld) {
    const long i = (long)blockIdx.x * ID_THREADS + threadIdx.x;         // F * 128 * 128 * 4 of them: whole workgroups
    const int q = (int)(i & 3);
    const long pix = i >> 2;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q == 0) {
        const int dx = (int)(pix % ID_SIDE), dy = (int)((pix / ID_SIDE) % ID_SIDE);
        const long f = pix / (ID_SIDE * ID_SIDE);
        const uint8_t* src = (f < N ? a : b) + (size_t)(f < N ? f : f - N) * (size_t)H * (size_t)W * 3;
        int y0, y1, x0, x1;
        double ly, lx;
        tap_of(dy, H, y0, y1, ly);
        tap_of(dx, W, x0, x1, lx);
        const double p00 = gray_of(src + ((size_t)y0 * W + x0) * 3), p01 = gray_of(src + ((size_t)y0 * W + x1) * 3);
        const double p10 = gray_of(src + ((size_t)y1 * W + x0) * 3), p11 = gray_of(src + ((size_t)y1 * W + x1) * 3);
        v.x = (float)((1.0 - ly) * ((1.0 - lx) * p00 + lx * p01) + ly * ((1.0 - lx) * p10 + lx * p11));
    }
    *reinterpret_cast<float4*>(y + (size_t)pix * (size_t)y_ld + 4 * q) = v;
}

// ---- embed --------------------------------------------------------------------------------------------------------------
// D (16 output rows x 16 frames, float64) += A (16 x 4) B (4 x 16) per v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k-group
// l >> 4] and B[k-group l >> 4][column l & 15], one double each, and D[row (l >> 4) + 4 i][column l & 15] in register i.  Which
// input a k-group stands for is free as long as A and B agree: lane (r, g) loads inputs s + 8 g .. s + 8 g + 7 of w's row r and
// of x's frame r as two float4 each (a row's four lanes read one 128-byte line), and instruction j of a step takes element j.
constexpr int EM_KCHUNK = FLAIR_IDENT_EMBED_KCHUNK;
constexpr int EM_ROWS = 16;                       // output rows of a workgroup
constexpr int EM_FRAMES = 16;                     // frames of a workgroup
constexpr int EM_WAVES = ID_THREADS / FLAIR_WAVE;
constexpr int EM_WAVE_K = EM_KCHUNK / EM_WAVES;   // consecutive inputs of one wave
constexpr int EM_STEP = 32;                       // inputs of one step of a wave: 4 k-groups x 8
static_assert(EM_WAVE_K % EM_STEP == 0 && EM_WAVES * 4 * FLAIR_WAVE == 4 * ID_THREADS, "a wave's inputs are whole steps");
typedef __attribute__((ext_vector_type(4))) double f64x4;

// four instructions: element j of both float4 is the input of k-group g in instruction j
__device__ __forceinline__ f64x4 embed_step(const float4& wv, const float4& xv, f64x4 acc) {
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)wv.x, (double)xv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)wv.y, (double)xv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)wv.z, (double)xv.z, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f64_16x16x4f64((double)wv.w, (double)xv.w, acc, 0, 0, 0);
}

__global__ __launch_bounds__(ID_THREADS) void ident_embed_kernel(const float* __restrict__ x, int x_ld, int F, int K,
                                                                  const float* __restrict__ w, int O, int chunks,
                                                                  double* __restrict__ ws) {
    __shared__ double red[EM_WAVES][4][FLAIR_WAVE];
    const int tid = threadIdx.x;
    const int lane = tid & (FLAIR_WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / FLAIR_WAVE);
    const int r = lane & 15, g = lane >> 4;
    const int chunk = (int)(blockIdx.x % (unsigned)chunks);
    const int o0 = (int)(blockIdx.x / (unsigned)chunks) * EM_ROWS;
    const int f0 = blockIdx.y * EM_FRAMES;
    const int k0 = chunk * EM_KCHUNK + wave * EM_WAVE_K;                  // this wave's inputs: none when k0 >= K
    const int k1 = k0 + EM_WAVE_K < K ? k0 + EM_WAVE_K : K;

    // a row or a frame past the end re-reads the last one and is not written
    const float* wr = w + (size_t)(o0 + r < O ? o0 + r : O - 1) * (size_t)K;
    const float* xr = x + (size_t)(f0 + r < F ? f0 + r : F - 1) * (size_t)x_ld;

    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    // whole steps without a test, the next step's loads issued before this step's arithmetic; the trip count is uniform over the wave
    int s = k0;
    if (s + EM_STEP <= k1) {
        const int off = 8 * g;
        float4 w0 = *reinterpret_cast<const float4*>(wr + s + off), w1 = *reinterpret_cast<const float4*>(wr + s + off + 4);
        float4 x0 = *reinterpret_cast<const float4*>(xr + s + off), x1 = *reinterpret_cast<const float4*>(xr + s + off + 4);
        for (s += EM_STEP; s + EM_STEP <= k1; s += EM_STEP) {
            const float4 nw0 = *reinterpret_cast<const float4*>(wr + s + off), nw1 = *reinterpret_cast<const float4*>(wr + s + off + 4);
            const float4 nx0 = *reinterpret_cast<const float4*>(xr + s + off), nx1 = *reinterpret_cast<const float4*>(xr + s + off + 4);
            acc = embed_step(w0, x0, acc);
            acc = embed_step(w1, x1, acc);
            w0 = nw0, w1 = nw1, x0 = nx0, x1 = nx1;
        }
        acc = embed_step(w0, x0, acc);
        acc = embed_step(w1, x1, acc);
    }
    // what is left of K (a multiple of 4): a float4 past the end is read at k0 instead and counts as zeros on both sides
    if (s < k1) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = s + 8 * g + 4 * h;
            const bool in = k < k1;
            float4 wv = *reinterpret_cast<const float4*>(wr + (in ? k : k0)), xv = *reinterpret_cast<const float4*>(xr + (in ? k : k0));
            if (!in) wv = xv = make_float4(0.f, 0.f, 0.f, 0.f);
            acc = embed_step(wv, xv, acc);
        }
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][i][lane] = acc[i];
    __syncthreads();
    // thread (i, l) adds the four waves' D[row (l >> 4) + 4 i][column l & 15] in wave order
    const int i = tid / FLAIR_WAVE;
    double t = red[0][i][lane];
#pragma unroll
    for (int v = 1; v < EM_WAVES; ++v) t += red[v][i][lane];
    const int o = o0 + g + 4 * i, f = f0 + r;
    if (o < O && f < F) ws[((size_t)chunk * (size_t)F + (size_t)f) * (size_t)O + (size_t)o] = t;
}

// out[f][o] = (float)(bias[o] + partial 0 + partial 1 + ...)
__global__ __launch_bounds__(ID_THREADS) void ident_embed_sum_kernel(const double* __restrict__ ws, const float* __restrict__ bias, int F,
                                                                      int O, int chunks, float* __restrict__ out, int out_ld) {
    const long i = (long)blockIdx.x * ID_THREADS + threadIdx.x;
    if (i >= (long)F * O) return;
    const int o = (int)(i % O);
    const long f = i / O;
    const double* p = ws + i;
    const size_t cell = (size_t)F * (size_t)O;
    double t = (double)bias[o];
    int c = 0;
    for (; c + 8 <= chunks; c += 8) {               // eight loads in flight, added in ascending order
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(c + j) * cell];
#pragma unroll
        for (int j = 0; j < 8; ++j) t += v[j];
    }
    for (; c < chunks; ++c) t += p[(size_t)c * cell];
    out[(size_t)f * (size_t)out_ld + o] = (float)t;
}
}  // namespace

extern "C" int flair_ident_prepare(const uint8_t* a, const uint8_t* b, int N, int H, int W, float* y, int y_ld, hipStream_t stream) {
    FLAIR_CHECK(a && y, "flair_ident_prepare: null pointer (a = %p, y = %p; b may be null)", (const void*)a, (const void*)y);
    FLAIR_CHECK(N >= 1 && H >= 1 && W >= 1, "flair_ident_prepare: N = %d, H = %d, W = %d must be positive", N, H, W);
    FLAIR_CHECK_VIEW("flair_ident_prepare", "y", y, y_ld, 16, 4);
    const long F = b ? 2L * N : (long)N;
    const long groups = F * (ID_SIDE * ID_SIDE * 4 / ID_THREADS);
    FLAIR_CHECK(groups <= 0x7fffffffL, "flair_ident_prepare: %ld frames (N = %d) exceed one launch", F, N);
    hipLaunchKernelGGL(ident_prepare_kernel, dim3((unsigned)groups), dim3(ID_THREADS), 0, stream, a, b, N, H, W, y, y_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_ident_embed(const float* x, int x_ld, int F, int K, const float* w, const float* bias, int O, float* out,
                                 int out_ld, void* ws, size_t ws_bytes, hipStream_t stream) {
    FLAIR_CHECK(x && w && bias && out && ws, "flair_ident_embed: null pointer (x = %p, w = %p, bias = %p, out = %p, ws = %p)",
                (const void*)x, (const void*)w, (const void*)bias, (const void*)out, ws);
    FLAIR_CHECK(F >= 1 && K >= 1 && O >= 1, "flair_ident_embed: F = %d, K = %d, O = %d must be positive", F, K, O);
    FLAIR_CHECK(K % 4 == 0 && K <= (1 << 30), "flair_ident_embed: K = %d is not a multiple of 4 up to 2^30 (rows of w are read in 16-byte loads)", K);
    FLAIR_CHECK_VIEW("flair_ident_embed", "x", x, x_ld, K, 4);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(w) % 16 == 0, "flair_ident_embed: w = %p must be 16-byte aligned", (const void*)w);
    FLAIR_CHECK(out_ld >= O, "flair_ident_embed: out_ld = %d must be >= O = %d", out_ld, O);
    FLAIR_CHECK(reinterpret_cast<uintptr_t>(ws) % 8 == 0, "flair_ident_embed: ws = %p holds doubles and must be 8-byte aligned", ws);
    const long chunks = cdiv(K, EM_KCHUNK);
    const size_t need = (size_t)chunks * (size_t)F * (size_t)O * sizeof(double);
    FLAIR_CHECK(ws_bytes >= need, "flair_ident_embed: ws_bytes = %zu, ceil(K / FLAIR_IDENT_EMBED_KCHUNK) * F * O * 8 = %zu", ws_bytes, need);
    const long groups = chunks * cdiv(O, EM_ROWS), tiles = cdiv(F, EM_FRAMES);
    FLAIR_CHECK(groups <= 0x7fffffffL && tiles <= 65535 && (long)F * O <= 0x7fffffffL * (long)ID_THREADS,
                "flair_ident_embed: %ld workgroups by %ld (F = %d, K = %d, O = %d) exceed one launch", groups, tiles, F, K, O);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(ident_embed_kernel, dim3((unsigned)groups, (unsigned)tiles), dim3(ID_THREADS), 0, stream, x, x_ld, F, K, w, O,
                       (int)chunks, part);
    FLAIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(ident_embed_sum_kernel, dim3((unsigned)grid_for((long)F * O, ID_THREADS, GRID_NO_CAP)), dim3(ID_THREADS), 0, stream,
                       part, bias, F, O, (int)chunks, out, out_ld);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
