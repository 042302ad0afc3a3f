// Attention kernels of the FLAIR UNet.
//
// (1) Spatial QKV attention per (frame, head) over the H*W tokens of a frame, head
//     width D in {32, 64, 128} or a multiple of 64 from 192 to 1024 (one head per layer at
//     the modules' defaults) -- replaces QKVAttentionLegacy / QKVAttention (guided_diffusion/
//     unet_new.py:540-605: einsum QK^T, f32 softmax, einsum AV), at any L.  Other widths
//     (multiples of 8) go to flair_attention_wide (prior.hip) while its LDS tile holds them
//     (d + L <= 2048).
//       * bf16: flash-style MFMA kernel.  S^T = K.Q^T is computed with keys on the
//         accumulator rows and queries on the lanes, so the softmax row statistics are
//         lane-local (+1 exchange with lane^32) and the probability tile is reused in
//         place as the B operand of O^T += V^T.P^T (cdna_hip_programming.md section 3,
//         "An accumulator tile as the next MFMA's operand").
//         From D = 192 the channels of one head are split across the waves of a workgroup,
//         which sum their partial scores through LDS (attn_mfma_bf16_wide_kernel).
//       * f32: one wavefront per query at D = 64 (one channel per lane), two queries per
//         wavefront at D = 32, two / D/64 channels per lane at D = 128 / from 192; exact f32
//         arithmetic; this is the tight-tolerance parity path, not a speed path.
// (2) Temporal window attention per pixel -- replaces TemporalAttention's
//     unfold + flash_attn_func (unet_new.py:473-515, nn.py:370-386): one query (own
//     frame) against the F-1 neighbouring frames (replicate padding at clip ends).
//     VALU / bandwidth bound: G lanes per (frame, pixel, head), 8 channels per lane; G = d/8
//     rounded up to a power of two (8 at d = 64), d any multiple of 8 in [8, 256].
#include <hip/hip_fp16.h>

#include <type_traits>

#include "common.h"

namespace {

struct AttnArgs {
    const void* qkv;  // [frames][L][ld]
    void* out;        // [frames][L][outLd], channel = head*D + d
    int ld, outLd;
    int L, heads;
    int qOff, kOff, vOff, headStride;  // channel offsets: x_off + head*headStride
    float scale;                        // applied to q.k
};

// The scaled score of the f32 paths, rounded on its own.  Written as `d *= scale`, the later `d - mn` contracts to
// fma(d, scale, -mn) (-ffp-contract=fast), which for the key that holds the running maximum (mn = round(d * scale))
// returns the product's rounding error instead of 0: its p is exp(eps) instead of 1, l and acc pick up one rounding per
// key, and a one-hot or uniform softmax no longer returns the V row / the mean of the V rows to the last bit (1 ulp and up
// to 38 ulp at L = 130 were measured wherever scale or the dot product is no power of two).  The empty asm keeps the
// product in a register of its own.
__device__ __forceinline__ float scaled_score(float d, float scale) {
    float s = d * scale;
    asm volatile("" : "+v"(s));
    return s;
}

// ------------------------------------------------------------------ f32 / generic path
template <typename E, int D>
__global__ void attn_rowwise_kernel(AttnArgs a) {
    // LPQ lanes per query (QPW queries per wavefront), CPL channels per lane: D = 32: 32 x 2 x 1, D = 64: 64 x 1 x 1,
    // D = 128: 64 x 1 x 2 (channels lane and lane + 64)
    constexpr int LPQ = D < 64 ? D : 64, QPW = 64 / LPQ, CPL = D / LPQ;
    const int lane = threadIdx.x & 63;
    const int q = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * QPW + lane / LPQ;
    const int cl = lane % LPQ;
    const int fh = blockIdx.y;
    const int f = fh / a.heads, hd = fh % a.heads;
    if (q >= a.L) return;  // D = 32: the two queries of a wavefront reduce within their own 32 lanes
    const E* base = reinterpret_cast<const E*>(a.qkv) + (long)f * a.L * a.ld + hd * a.headStride;
    float qv[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) qv[j] = ET<E>::ld(base + (long)q * a.ld + a.qOff + cl + LPQ * j);
    float m = -INFINITY, l = 0.f, acc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) acc[j] = 0.f;
    for (int s = 0; s < a.L; ++s) {
        float d = qv[0] * ET<E>::ld(base + (long)s * a.ld + a.kOff + cl);
#pragma unroll
        for (int j = 1; j < CPL; ++j) d = fmaf(qv[j], ET<E>::ld(base + (long)s * a.ld + a.kOff + cl + LPQ * j), d);
#pragma unroll
        for (int off = LPQ / 2; off > 0; off >>= 1) d += __shfl_xor(d, off);
        d = scaled_score(d, a.scale);
        const float mn = fmaxf(m, d);
        const float alpha = __expf(m - mn);
        const float p = __expf(d - mn);
        l = l * alpha + p;
#pragma unroll
        for (int j = 0; j < CPL; ++j) acc[j] = acc[j] * alpha + p * ET<E>::ld(base + (long)s * a.ld + a.vOff + cl + LPQ * j);
        m = mn;
    }
    E* o = reinterpret_cast<E*>(a.out) + ((long)f * a.L + q) * a.outLd + hd * D + cl;
#pragma unroll
    for (int j = 0; j < CPL; ++j) ET<E>::st(o + LPQ * j, acc[j] / l);
}

// -------------------------------------------------------------- bf16 MFMA, pipelined
// 32 queries per wave, the S^T and O^T products on the matrix cores, structured around the latency that the plain
// tiled kernel of round 1 exposed once per 32-token tile (load K/V -> LDS -> barrier -> compute -> barrier), for head
// widths D = 32, 64 and 128:
//   * KV tiles of KV tokens, two LDS stages, ONE barrier per tile; the next tile's K and V are requested into
//     registers before the current tile's MFMAs and written to the other stage afterwards;
//   * V stays row-major in LDS ([token][D], written with 16-byte stores) and its transposed MFMA fragments
//     come from ds_read_b64_tr_b16 (the hardware transpose read) instead of eight 2-byte scatter stores per
//     thread and tile.  Each 32-lane half of that read takes 16 dwords from each of 4 consecutive rows, so
//     the row pitch VPITCH is the smallest >= 2D bytes that is an ODD multiple of 64 B (16 banks): the four
//     rows then start 16 banks apart (mod 64) and hit four disjoint 16-bank quarters, conflict-free.
//     D = 32: 64 B (16 dwords, no padding); D = 64: 192 B (48 dwords; 128 B would put rows 0 and 2 on the
//     same banks); D = 128: 320 B (80 dwords; 256 B would put all four rows on the same banks);
//   * KV = 64 tokens at D = 32 and 64, KV = 32 at D = 128.  Two stages of 64-token K+V tiles at D = 128
//     would be 2 x 36 KB = 72 KB per workgroup: past the 64 KB of static LDS, and two workgroups per CU.
//     32-token tiles keep it at 36 KB (D = 64: 40 KB) and a tile still carries 16 MFMAs as at D = 64 (8
//     k-steps of S^T, 2 x 4 of O^T) against half the softmax work per MFMA.  D = 128 runs two workgroups
//     per CU all the same: its Q fragments (32 VGPRs) and O^T accumulators (64) do not fit the 168-register
//     budget of three (the NW = 4 build spilled 68 bytes to scratch), and 2 x 4 waves fill 256 registers;
//   * NW = 2 wavefronts (64 queries) per workgroup when 128-query workgroups would leave CUs idle (L = 256:
//     256 instead of 128 workgroups), else 4.
typedef __attribute__((ext_vector_type(4))) short s16x4_t;

// K tile of width D: rows of D/8 16-byte chunks, swizzled so that the ds_read_b128 fragment reads (row = lane&31,
// one chunk per 32-lane half) spread each 16-lane group over the 64 banks
template <int D>
__device__ __forceinline__ int k_off_d(int row, int chunk) {
    if constexpr (D == 32) return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4);
    else if constexpr (D == 64) return row * 128 + ((chunk ^ (row & 7)) << 4);
    else return row * 256 + ((chunk ^ (row & 15)) << 4);
}

// (lo, hi) -> packed bf16 pair; inline asm so that the vectoriser cannot pair the conversions by register
// neighbourhood and re-interleave afterwards (measured in the ISA: 32 cvt + 32 fix-ups instead of 16 cvt)
__device__ __forceinline__ unsigned cvt_pk_bf16_asm(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

template <int NW, int D>
__global__ __launch_bounds__(64 * NW, D == 128 ? 2 : 3) void attn_mfma_bf16_v2_kernel(AttnArgs a) {
    static_assert(D == 32 || D == 64 || D == 128, "head width");
    constexpr int NT = 64 * NW, KV = D == 128 ? 32 : 64, H2 = KV / 32;
    constexpr int CH = D / 8, LOG2CH = D == 32 ? 2 : D == 64 ? 3 : 4;  // 16-byte chunks per row
    constexpr int KPITCH = 2 * D, VPITCH = D == 32 ? 64 : D == 64 ? 192 : 320;
    constexpr int STAGE = KV * KPITCH + KV * VPITCH;                 // 8 / 20 / 18 KB per stage
    constexpr int PIECES = KV * CH;                                  // 16-byte pieces of one K (or V) tile
    constexpr int LI = (PIECES + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int fh = blockIdx.y;
    const int f = fh / a.heads, hd = fh % a.heads;
    const bf16_t* base = reinterpret_cast<const bf16_t*>(a.qkv) + (long)f * a.L * a.ld + hd * a.headStride;
    const int q = blockIdx.x * (32 * NW) + wave * 32 + lr;
    const bool qok = q < a.L;

    uint4 qf[D / 16];
#pragma unroll
    for (int s = 0; s < D / 16; ++s)
        qf[s] = qok ? *reinterpret_cast<const uint4*>(base + (long)q * a.ld + a.qOff + 16 * s + 8 * lh)
                    : make_uint4(0, 0, 0, 0);

    f32x16 o[D / 32];
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m = -1e30f, l = 0.f;
    const float sc = a.scale * 1.4426950408889634f;                  // scores in log2 units: exp2 instead of exp

    uint4 kreg[LI], vreg[LI];
    auto issue = [&](int t) {
#pragma unroll
        for (int i = 0; i < LI; ++i) {
            const int id = i * NT + tid;
            const int kv = id >> LOG2CH, ch = id & (CH - 1);
            const int tok = t * KV + kv;
            const bool ok = id < PIECES && tok < a.L;
            kreg[i] = ok ? *reinterpret_cast<const uint4*>(base + (long)tok * a.ld + a.kOff + ch * 8) : make_uint4(0, 0, 0, 0);
            vreg[i] = ok ? *reinterpret_cast<const uint4*>(base + (long)tok * a.ld + a.vOff + ch * 8) : make_uint4(0, 0, 0, 0);
        }
    };
    auto stage = [&](int buf) {
        char* sk = smem + buf * STAGE;
        char* sv = sk + KV * KPITCH;
#pragma unroll
        for (int i = 0; i < LI; ++i) {
            const int id = i * NT + tid;
            if (id < PIECES) {
                const int kv = id >> LOG2CH, ch = id & (CH - 1);
                *reinterpret_cast<uint4*>(sk + k_off_d<D>(kv, ch)) = kreg[i];
                *reinterpret_cast<uint4*>(sv + kv * VPITCH + ch * 16) = vreg[i];
            }
        }
    };

    const int ntile = (a.L + KV - 1) / KV;
    issue(0);
    stage(0);
    __syncthreads();
    // this lane's address inside a transposed 4-row x 16-column block of V (lane 4q+p of a 16-lane group supplies
    // row q, columns 4p..4p+3); group g = lane>>4: columns 16*(g&1).., k-half g>>1 (= lh)
    const int gl = lane & 15;
    const int trOff = ((gl >> 2) + 4 * lh) * VPITCH + (16 * ((lane >> 4) & 1) + 4 * (gl & 3)) * 2;
    // one KV tile out of LDS stage BUF (a compile-time constant: the two stages are two unrolled copies of the body,
    // so every fragment address is loop-invariant instead of 30 address adds per tile)
    auto tile = [&](int t, auto bufc) {
        constexpr int BUF = decltype(bufc)::value;
        const char* sk = smem + BUF * STAGE;
        const char* sv = sk + KV * KPITCH;
        if (t + 1 < ntile) issue(t + 1);

        // ---- S^T[kv][q] = K . Q^T for the 32-token parts of the tile
        f32x16 s[H2];
#pragma unroll
        for (int h2 = 0; h2 < H2; ++h2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[h2][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < D / 16; ++ks) {
                const uint4 kf = *reinterpret_cast<const uint4*>(sk + k_off_d<D>(32 * h2 + lr, 2 * ks + lh));
                s[h2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf),
                                                            __builtin_bit_cast(bf16x8, qf[ks]), s[h2], 0, 0, 0);
            }
        }
        // rows of this lane: kv = 32*h2 + (r&3) + 8*(r>>2) + 4*lh.  The softmax is the VALU bottleneck of this
        // kernel (32 scores per lane and tile against 16 MFMAs at D = 64), so: tokens beyond L are masked only in the
        // last tile (wave-uniform branch), the scale rides in the exponent's FMA (p = 2^(s*sc - m), the running
        // maximum is kept in scaled units), v_exp_f32 directly, and the accumulators are rescaled only when some
        // row's maximum grew
        if ((t + 1) * KV > a.L) {
            asm volatile("; partly masked last tile" ::: "memory");   // keeps this a branch (if-converted it is 64 VALU per tile)
#pragma unroll
            for (int h2 = 0; h2 < H2; ++h2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = t * KV + 32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (kv >= a.L) s[h2][r] = -1e30f;
                }
        }
        float tmax = -1e30f;
#pragma unroll
        for (int h2 = 0; h2 < H2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[h2][r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32)) * sc;
        const float mn = fmaxf(m, tmax);
        float ps[4] = {0.f, 0.f, 0.f, 0.f};                     // four short add chains instead of one of 32
#pragma unroll
        for (int h2 = 0; h2 < H2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[h2][r] = __builtin_amdgcn_exp2f(fmaf(s[h2][r], sc, -mn));
                ps[r & 3] += s[h2][r];
            }
        float psum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
        psum += __shfl_xor(psum, 32);
        if (__builtin_amdgcn_ballot_w64(mn > m) != 0) {          // some query's running maximum moved: rescale
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            l *= alpha;
#pragma unroll
            for (int i = 0; i < D / 32; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
            m = mn;
        }
        l += psum;

        // ---- O^T[d][q] += V^T[d][kv] . P^T[kv][q]: k-step (h2, ks2) covers tokens 32*h2 + 16*ks2 .. +15 in the
        // order (r&3) + 8*(r>>2) + 4*lh of the accumulator registers 8*ks2 .. 8*ks2+7 (any order, used on both sides)
#pragma unroll
        for (int h2 = 0; h2 < H2; ++h2)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                uint4 pf;
                pf.x = cvt_pk_bf16_asm(s[h2][8 * ks + 0], s[h2][8 * ks + 1]);
                pf.y = cvt_pk_bf16_asm(s[h2][8 * ks + 2], s[h2][8 * ks + 3]);
                pf.z = cvt_pk_bf16_asm(s[h2][8 * ks + 4], s[h2][8 * ks + 5]);
                pf.w = cvt_pk_bf16_asm(s[h2][8 * ks + 6], s[h2][8 * ks + 7]);
#pragma unroll
                for (int i = 0; i < D / 32; ++i) {
                    // elements 0..3: tokens row0 + 4*lh + {0..3}; elements 4..7: the same rows + 8
                    const char* vb = sv + (32 * h2 + 16 * ks) * VPITCH + 64 * i + trOff;
                    const s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4_t*)(vb));
                    const s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4_t*)(vb + 8 * VPITCH));
                    uint4 vf;
                    vf.x = ((const unsigned*)&v0)[0]; vf.y = ((const unsigned*)&v0)[1];
                    vf.z = ((const unsigned*)&v1)[0]; vf.w = ((const unsigned*)&v1)[1];
                    o[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf),
                                                                   __builtin_bit_cast(bf16x8, pf), o[i], 0, 0, 0);
                }
            }
        if (t + 1 < ntile) stage(BUF ^ 1);
        __syncthreads();
    };
    for (int t = 0; t < ntile; t += 2) {
        tile(t, std::integral_constant<int, 0>{});
        if (t + 1 < ntile) tile(t + 1, std::integral_constant<int, 1>{});
    }
    if (!qok) return;
    const float inv = 1.f / l;
    bf16_t* op = reinterpret_cast<bf16_t*>(a.out) + ((long)f * a.L + q) * a.outLd + hd * D;
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint2 pk;
            pk.x = pack2bf(o[i][4 * g + 0] * inv, o[i][4 * g + 1] * inv);
            pk.y = pack2bf(o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv);
            *reinterpret_cast<uint2*>(op + 32 * i + 8 * g + 4 * lh) = pk;
        }
}

// -------------------------------------------------------- bf16 MFMA, wide heads (d = 192 ... 1024)
// One head of d = 64 * nc channels (nc = 3 ... 16) for 32 queries per workgroup of NW waves, KV tiles of 32 tokens.
// A 32 x d f32 O^T tile is 4 KiB per 32 channels, too much for one wave, so the CHANNELS are split across the waves:
// 64-channel chunk c belongs to wave c % NW, which owns up to CPW chunks (template parameters; the run-time nc masks
// the last one): NW = 4, CPW = 1 up to d = 256, NW = 4, CPW = 2 up to 512, NW = 8, CPW = 2 beyond (4 waves with 3 or 4
// chunks each need 416 / > 512 registers: the 4-chunk build spilled).  Per tile, every wave
//   * computes its partial S^T = K_c . Q_c^T over its own chunks (the K fragments come straight from global memory:
//     no other wave reads them, and the 16-byte loads of one chunk consume whole 128-byte lines);
//   * writes the partial (16 floats per lane) to LDS; ONE workgroup barrier; reads the NW partials and adds them in
//     wave order, so all waves hold the same S^T bit for bit;
//   * runs the online softmax of v2 on it (redundantly in each wave: the same cost per wave as one wave doing it,
//     and no second barrier to hand P around) and keeps P^T in registers as the B operand;
//   * does O^T_c += V_c^T . P^T for its own chunks, V_c read transposed (ds_read_b64_tr_b16) from a tile that only
//     this wave writes: [32 tokens][64 * CPW] bf16 rows at pitch 64 * (2 * CPW + 1) bytes, an odd multiple of 64 B
//     (conflict-free transposed reads, see v2).  The wave writes V(t) there after its S MFMAs and reads it after the
//     barrier; LDS operations of one wave are executed in order, so no barrier guards this tile.
// K(t+1) is requested into registers right after tile t's S MFMAs, V(t+1) right after tile t's softmax (so it is not
// live across the exchange, where the NW partials are); both land during the remaining work of tile t.  The
// partials are double-buffered by tile parity, so the one barrier per tile also orders tile t+2's writes after tile
// t's reads.  LDS: 2 x NW x 4 KiB of partials + NW x 32 x pitch = 56 / 72 / 144 KiB (two / two / one per CU).
template <int NW, int CPW>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void attn_mfma_bf16_wide_kernel(AttnArgs a, int nc) {
    constexpr int VP = 64 * (2 * CPW + 1);
    extern __shared__ __attribute__((aligned(16))) char wsmem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int fh = blockIdx.y;
    const int f = fh / a.heads, hd = fh % a.heads;
    const bf16_t* base = reinterpret_cast<const bf16_t*>(a.qkv) + (long)f * a.L * a.ld + hd * a.headStride;
    const int q = blockIdx.x * 32 + lr;
    const bool qok = q < a.L;
    float4* sS = reinterpret_cast<float4*>(wsmem);                    // [parity][wave][4][64 lanes] float4
    char* sv = wsmem + 2 * NW * 4 * 64 * 16 + wave * 32 * VP;         // this wave's V tile
    // chunk j of this wave: channels 64 * (wave + NW*j) ..; only the last j can be beyond nc (wave-uniform)
    auto own = [&](int j) { return wave + NW * j < nc; };
    auto chan = [&](int j) { return own(j) ? 64 * (wave + NW * j) : 0; };

    // rows beyond L (queries of the last block, tokens of the last tile) are read from row L-1 instead of masked
    // loads: those queries are not stored, those tokens' scores are set to -1e30 after the exchange (P = 0 against
    // finite V); a chunk the wave does not own reads chunk 0 (in bounds) and is skipped by wave-uniform branches
    const int qc = qok ? q : a.L - 1;
    uint4 qf[CPW][4];
#pragma unroll
    for (int j = 0; j < CPW; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s)
            qf[j][s] = *reinterpret_cast<const uint4*>(base + (long)qc * a.ld + a.qOff + chan(j) + 16 * s + 8 * lh);
    f32x16 o[CPW][2];
#pragma unroll
    for (int j = 0; j < CPW; ++j)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[j][b][r] = 0.f;
    float m = -1e30f, l = 0.f;
    const float sc = a.scale * 1.4426950408889634f;

    // K fragments (A operand of S^T: row kv = lane&31, channels 16s + 8*lh ..) and V (token lane>>1, channels
    // 32*(lane&1) + 8i .. of the chunk: one address per lane and chunk) of tile t
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;   // a register value: uint4 copies into LDS went
    uint4 kf[CPW][4];                                                // through a scratch temporary (memcpy)
    u32x4 vr[CPW][4];
    auto issueK = [&](int t) {
        const int tk = min(t * 32 + lr, a.L - 1);
#pragma unroll
        for (int j = 0; j < CPW; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                kf[j][s] = *reinterpret_cast<const uint4*>(base + (long)tk * a.ld + a.kOff + chan(j) + 16 * s + 8 * lh);
    };
    auto issueV = [&](int t) {
        const int tv = min(t * 32 + (lane >> 1), a.L - 1);
#pragma unroll
        for (int j = 0; j < CPW; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                vr[j][i] = *reinterpret_cast<const u32x4*>(base + (long)tv * a.ld + a.vOff + chan(j) + 32 * (lane & 1) + 8 * i);
    };
    const int gl = lane & 15;
    const int trOff = ((gl >> 2) + 4 * lh) * VP + (16 * ((lane >> 4) & 1) + 4 * (gl & 3)) * 2;

    const int ntile = (a.L + 31) / 32;
    issueK(0);
    issueV(0);
    for (int t = 0; t < ntile; ++t) {
        // ---- partial S^T[kv][q] over this wave's chunks
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int j = 0; j < CPW; ++j)
            if (own(j))
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf[j][ks]),
                                                                __builtin_bit_cast(bf16x8, qf[j][ks]), s, 0, 0, 0);
        if (t + 1 < ntile) issueK(t + 1);
        // ---- V(t) into this wave's tile (after tile t-1's transposed reads: same wave, in order)
#pragma unroll
        for (int j = 0; j < CPW; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *reinterpret_cast<u32x4*>(sv + (lane >> 1) * VP + 128 * j + 64 * (lane & 1) + 16 * i) = vr[j][i];
        asm volatile("" ::: "memory");   // and this tile's transposed reads behind these stores
        // ---- sum the NW partials through LDS (same order in every wave)
        float4* slot = sS + (t & 1) * NW * 256;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            slot[wave * 256 + g * 64 + lane] = make_float4(s[4 * g], s[4 * g + 1], s[4 * g + 2], s[4 * g + 3]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 v = slot[w * 256 + g * 64 + lane];
                s[4 * g] += v.x; s[4 * g + 1] += v.y; s[4 * g + 2] += v.z; s[4 * g + 3] += v.w;
            }
        // ---- online softmax (as v2): rows of this lane are kv = (r&3) + 8*(r>>2) + 4*lh
        if ((t + 1) * 32 > a.L) {
            asm volatile("; partly masked last tile" ::: "memory");
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh >= a.L) s[r] = -1e30f;
        }
        float tmax = -1e30f;
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32)) * sc;
        const float mn = fmaxf(m, tmax);
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], sc, -mn));
            ps[r & 3] += s[r];
        }
        float psum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
        psum += __shfl_xor(psum, 32);
        if (__builtin_amdgcn_ballot_w64(mn > m) != 0) {
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            l *= alpha;
#pragma unroll
            for (int j = 0; j < CPW; ++j)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[j][b][r] *= alpha;
            m = mn;
        }
        l += psum;
        if (t + 1 < ntile) issueV(t + 1);   // lands during this P.V and the next S (not live across the exchange)
        // ---- O^T[d][q] += V^T[d][kv] . P^T[kv][q] for this wave's chunks
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 pf;
            pf.x = cvt_pk_bf16_asm(s[8 * ks + 0], s[8 * ks + 1]);
            pf.y = cvt_pk_bf16_asm(s[8 * ks + 2], s[8 * ks + 3]);
            pf.z = cvt_pk_bf16_asm(s[8 * ks + 4], s[8 * ks + 5]);
            pf.w = cvt_pk_bf16_asm(s[8 * ks + 6], s[8 * ks + 7]);
#pragma unroll
            for (int j = 0; j < CPW; ++j)
                if (own(j))
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const char* vb = sv + 16 * ks * VP + 128 * j + 64 * b + trOff;
                        const s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) s16x4_t*)(vb));
                        const s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) s16x4_t*)(vb + 8 * VP));
                        uint4 vf;
                        vf.x = ((const unsigned*)&v0)[0]; vf.y = ((const unsigned*)&v0)[1];
                        vf.z = ((const unsigned*)&v1)[0]; vf.w = ((const unsigned*)&v1)[1];
                        o[j][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf),
                                                                          __builtin_bit_cast(bf16x8, pf), o[j][b], 0, 0, 0);
                    }
        }
        asm volatile("" ::: "memory");   // the next tile's V stores stay behind these reads
    }
    if (!qok) return;
    const float inv = 1.f / l;
    bf16_t* op = reinterpret_cast<bf16_t*>(a.out) + ((long)f * a.L + q) * a.outLd + hd * 64 * nc;
#pragma unroll
    for (int j = 0; j < CPW; ++j)
        if (own(j))
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint2 pk;
                    pk.x = pack2bf(o[j][b][4 * g + 0] * inv, o[j][b][4 * g + 1] * inv);
                    pk.y = pack2bf(o[j][b][4 * g + 2] * inv, o[j][b][4 * g + 3] * inv);
                    *reinterpret_cast<uint2*>(op + 64 * (wave + NW * j) + 32 * b + 8 * g + 4 * lh) = pk;
                }
}

// f32 at the wide widths: attn_rowwise_kernel's one wavefront per query with nc = d / 64 channels per lane (lane + 64j)
__global__ void attn_rowwise_wide_kernel(AttnArgs a, int nc) {
    constexpr int MAXC = 16;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int fh = blockIdx.y;
    const int f = fh / a.heads, hd = fh % a.heads;
    if (q >= a.L) return;
    const float* base = reinterpret_cast<const float*>(a.qkv) + (long)f * a.L * a.ld + hd * a.headStride + lane;
    float qv[MAXC], acc[MAXC];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        qv[j] = j < nc ? base[(long)q * a.ld + a.qOff + 64 * j] : 0.f;
        acc[j] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int s = 0; s < a.L; ++s) {
        const float* kr = base + (long)s * a.ld + a.kOff;
        float d = qv[0] * kr[0];
#pragma unroll
        for (int j = 1; j < MAXC; ++j)
            if (j < nc) d = fmaf(qv[j], kr[64 * j], d);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
        d = scaled_score(d, a.scale);
        const float mn = fmaxf(m, d);
        const float alpha = __expf(m - mn);
        const float p = __expf(d - mn);
        l = l * alpha + p;
        const float* vr = base + (long)s * a.ld + a.vOff;
#pragma unroll
        for (int j = 0; j < MAXC; ++j)
            if (j < nc) acc[j] = acc[j] * alpha + p * vr[64 * j];
        m = mn;
    }
    float* o = reinterpret_cast<float*>(a.out) + ((long)f * a.L + q) * a.outLd + hd * 64 * nc + lane;
#pragma unroll
    for (int j = 0; j < MAXC; ++j)
        if (j < nc) o[64 * j] = acc[j] / l;
}

// ---------------------------------------------------------------- temporal window
template <typename E> __device__ __forceinline__ void load8(const E* p, float* v);
template <> __device__ __forceinline__ void load8<float>(const float* p, float* v) {
    Vec16<float>::load(p, v);
    Vec16<float>::load(p + 4, v + 4);
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float* v) { Vec16<bf16_t>::load(p, v); }
template <typename E> __device__ __forceinline__ void store8(E* p, const float* v);
template <> __device__ __forceinline__ void store8<float>(float* p, const float* v) {
    Vec16<float>::store(p, v);
    Vec16<float>::store(p + 4, v + 4);
}
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float* v) { Vec16<bf16_t>::store(p, v); }

__device__ __forceinline__ float rh(float v) { return __half2float(__float2half(v)); }

struct TAttnArgs {
    const void* qkv;  // [T][HW][ld]: q | k | v, each C wide, channel = head*d + c
    const float* kpos;  // [window-1][C]: W_k . pe_j, added to k of window slot j
    void* out;          // [T][HW][outLd]
    int ld, outLd, T, C, window;
    long HW;
    int roundFp16;
    float scale;
    int headDim;        // d, a multiple of 8 in [8, 256]
};

// G lanes per item, 8 channels each.  MASKED = false: d = 8*G (a compile-time width); MASKED = true: d/8 < G, the
// lanes sub >= d/8 read the head's first 8 channels (in bounds), add 0 to the dot product and store nothing.
template <typename E, int G, bool MASKED>
__global__ void temporal_attn_kernel(TAttnArgs a) {
    constexpr int LOG2G = G == 1 ? 0 : G == 2 ? 1 : G == 4 ? 2 : G == 8 ? 3 : G == 16 ? 4 : 5;
    static_assert((1 << LOG2G) == G && G <= 32, "lane group");
    const int D = MASKED ? a.headDim : 8 * G;
    const int heads = a.C / D;
    const long items = (long)a.T * a.HW * heads;  // one item = (t, pixel, head), G lanes each
    const long gid = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long item = gid >> LOG2G;
    const int sub = (int)(gid & (G - 1));
    if (item >= items) return;  // whole G-lane groups leave together
    const bool on = !MASKED || sub * 8 < D;
    const int hd = (int)(item % heads);
    const long tp = item / heads;
    const long pix = tp % a.HW;
    const int t = (int)(tp / a.HW);
    const int c = hd * D + (on ? sub * 8 : 0);
    const E* base = reinterpret_cast<const E*>(a.qkv);
    float q[8];
    load8<E>(base + ((long)t * a.HW + pix) * a.ld + c, q);
    if (a.roundFp16)
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = rh(q[i]);
    const int half = a.window / 2;
    float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    int slot = 0;
    for (int j = -half; j <= half; ++j) {
        if (j == 0) continue;
        int tt = t + j;
        tt = tt < 0 ? 0 : (tt >= a.T ? a.T - 1 : tt);
        const E* row = base + ((long)tt * a.HW + pix) * a.ld;
        float k[8], v[8];
        load8<E>(row + a.C + c, k);
        load8<E>(row + 2 * a.C + c, v);
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float kk = k[i] + a.kpos[slot * a.C + c + i];
            if (a.roundFp16) {
                kk = rh(kk);
                v[i] = rh(v[i]);
            }
            d = fmaf(q[i], kk, d);
        }
        if (!on) d = 0.f;
#pragma unroll
        for (int off = 1; off < G; off <<= 1) d += __shfl_xor(d, off);
        d = scaled_score(d, a.scale);
        const float mn = fmaxf(m, d);
        const float alpha = __expf(m - mn), p = __expf(d - mn);
        l = l * alpha + p;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = acc[i] * alpha + p * v[i];
        m = mn;
        ++slot;
    }
    const float inv = 1.f / l;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        acc[i] *= inv;
        if (a.roundFp16) acc[i] = rh(acc[i]);
    }
    if (on) store8<E>(reinterpret_cast<E*>(a.out) + ((long)t * a.HW + pix) * a.outLd + c, acc);
}

template <typename E, int G>
void launch_temporal(const TAttnArgs& a, hipStream_t stream) {
    const long threads = (long)a.T * a.HW * (a.C / a.headDim) * G;
    const int grid = (int)((threads + 255) / 256);
    if (a.headDim == 8 * G)
        hipLaunchKernelGGL((temporal_attn_kernel<E, G, false>), dim3(grid), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((temporal_attn_kernel<E, G, true>), dim3(grid), dim3(256), 0, stream, a);
}

template <typename E>
void launch_temporal(const TAttnArgs& a, hipStream_t stream) {
    const int n = a.headDim / 8;   // lanes that carry channels; the group is n rounded up to a power of two
    if (n <= 1) launch_temporal<E, 1>(a, stream);
    else if (n <= 2) launch_temporal<E, 2>(a, stream);
    else if (n <= 4) launch_temporal<E, 4>(a, stream);
    else if (n <= 8) launch_temporal<E, 8>(a, stream);
    else if (n <= 16) launch_temporal<E, 16>(a, stream);
    else launch_temporal<E, 32>(a, stream);
}

template <int D>
void launch_qkv_bf16(const flair_attn_params* p, const AttnArgs& a, hipStream_t stream) {
    const long wg128 = (long)((p->L + 127) / 128) * p->frames * p->heads;
    if (wg128 >= 256)
        hipLaunchKernelGGL((attn_mfma_bf16_v2_kernel<4, D>), dim3((p->L + 127) / 128, p->frames * p->heads), dim3(256),
                           0, stream, a);
    else
        hipLaunchKernelGGL((attn_mfma_bf16_v2_kernel<2, D>), dim3((p->L + 63) / 64, p->frames * p->heads), dim3(128), 0,
                           stream, a);
}

template <int D>
void launch_qkv_f32(const flair_attn_params* p, const AttnArgs& a, hipStream_t stream) {
    constexpr int QPB = 4 * (D < 64 ? 64 / D : 1);   // queries per 256-thread workgroup
    hipLaunchKernelGGL((attn_rowwise_kernel<float, D>), dim3((p->L + QPB - 1) / QPB, p->frames * p->heads), dim3(256), 0,
                       stream, a);
}

// d = 64 * nc, nc = 3 ... 16: 4 waves with 1 or 2 chunks each up to nc = 8, else 8 waves with up to 2 chunks
template <int NW, int CPW>
int launch_qkv_bf16_wide_cfg(const flair_attn_params* p, const AttnArgs& a, int nc, hipStream_t stream) {
    constexpr int lds = 2 * NW * 4 * 64 * 16 + NW * 32 * 64 * (2 * CPW + 1);
    static LdsAttrOnce attr;
    FLAIR_CHECK(flair_max_lds_once(attr, reinterpret_cast<const void*>(&attn_mfma_bf16_wide_kernel<NW, CPW>), lds) ==
                    hipSuccess,
                "flair_qkv_attention: hipFuncSetAttribute failed");
    hipLaunchKernelGGL((attn_mfma_bf16_wide_kernel<NW, CPW>), dim3((p->L + 31) / 32, p->frames * p->heads), dim3(64 * NW),
                       lds, stream, a, nc);
    return FLAIR_OK;
}

int launch_qkv_bf16_wide(const flair_attn_params* p, const AttnArgs& a, hipStream_t stream) {
    const int nc = p->head_dim / 64;
    if (nc <= 4) return launch_qkv_bf16_wide_cfg<4, 1>(p, a, nc, stream);
    if (nc <= 8) return launch_qkv_bf16_wide_cfg<4, 2>(p, a, nc, stream);
    return launch_qkv_bf16_wide_cfg<8, 2>(p, a, nc, stream);
}

}  // namespace

// flair_attention_wide (prior.hip) holds 16 rows of d + L floats in 128 KiB of LDS
constexpr int kWideAttnMaxDL = 2048;
// flair_qkv_attention's wide-head kernels: multiples of 64 in [192, 1024] at any L
constexpr int kWideHeadMin = 192, kWideHeadMax = 1024;

extern "C" int flair_qkv_attention(const flair_attn_params* p, const void* qkv, void* out, hipStream_t stream) {
    FLAIR_CHECK(p && qkv && out, "flair_qkv_attention: null argument");
    FLAIR_CHECK_DTYPE("flair_qkv_attention", p->dtype);
    FLAIR_CHECK(p->frames > 0 && p->L > 0 && p->heads > 0, "flair_qkv_attention: empty shape");
    const int d = p->head_dim;
    const bool native = d == 32 || d == 64 || d == 128;
    const bool wide = d % 64 == 0 && d >= kWideHeadMin && d <= kWideHeadMax;
    FLAIR_CHECK(native || wide || (d > 0 && d % 8 == 0 && d + p->L <= kWideAttnMaxDL),
                "flair_qkv_attention: head width %d unsupported at L = %d (32, 64 and 128 and multiples of 64 from %d to "
                "%d at any L; other multiples of 8 while head width + L <= %d)", d, p->L, kWideHeadMin, kWideHeadMax,
                kWideAttnMaxDL);
    FLAIR_CHECK(p->ld % 8 == 0 && p->out_ld % 8 == 0 && p->q_off % 8 == 0 && p->k_off % 8 == 0 &&
                    p->v_off % 8 == 0 && p->head_stride % 8 == 0,
                "flair_qkv_attention: offsets/strides must be multiples of 8 elements");
    const int hi_off = p->q_off > p->k_off ? (p->q_off > p->v_off ? p->q_off : p->v_off)
                                           : (p->k_off > p->v_off ? p->k_off : p->v_off);
    FLAIR_CHECK(hi_off + (long)(p->heads - 1) * p->head_stride + d <= p->ld && (long)p->heads * d <= p->out_ld,
                "flair_qkv_attention: %d heads of width %d exceed ld %d / out_ld %d", p->heads, d, p->ld, p->out_ld);
    if (!native && !wide) return flair_attention_wide(p, qkv, out, stream);
    AttnArgs a;
    a.qkv = qkv; a.out = out; a.ld = p->ld; a.outLd = p->out_ld; a.L = p->L; a.heads = p->heads;
    a.qOff = p->q_off; a.kOff = p->k_off; a.vOff = p->v_off; a.headStride = p->head_stride;
    a.scale = p->scale;
    if (p->dtype == FLAIR_BF16) {
        if (wide) {
            const int rc = launch_qkv_bf16_wide(p, a, stream);
            if (rc != FLAIR_OK) return rc;
        } else if (d == 32)
            launch_qkv_bf16<32>(p, a, stream);
        else if (d == 128)
            launch_qkv_bf16<128>(p, a, stream);
        else
            launch_qkv_bf16<64>(p, a, stream);
    } else {
        if (wide)
            hipLaunchKernelGGL(attn_rowwise_wide_kernel, dim3((p->L + 3) / 4, p->frames * p->heads), dim3(256), 0, stream,
                               a, d / 64);
        else if (d == 32)
            launch_qkv_f32<32>(p, a, stream);
        else if (d == 128)
            launch_qkv_f32<128>(p, a, stream);
        else
            launch_qkv_f32<64>(p, a, stream);
    }
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}

extern "C" int flair_temporal_attention(const flair_tattn_params* p, const void* qkv, const float* kpos, void* out,
                                        hipStream_t stream) {
    FLAIR_CHECK(p && qkv && kpos && out, "flair_temporal_attention: null argument");
    FLAIR_CHECK_DTYPE("flair_temporal_attention", p->dtype);
    const int d = p->head_dim ? p->head_dim : 64;   // 0: the width-64 default of ABI version <= 6
    FLAIR_CHECK(d % 8 == 0 && d >= 8 && d <= 256,
                "flair_temporal_attention: head width %d unsupported (multiples of 8 from 8 to 256)", d);
    FLAIR_CHECK(p->C > 0 && p->C % d == 0 && p->window % 2 == 1 && p->window >= 3,
                "flair_temporal_attention: C=%d head width=%d window=%d", p->C, d, p->window);
    FLAIR_CHECK(p->ld >= 3 * p->C && p->ld % 8 == 0 && p->out_ld % 8 == 0, "flair_temporal_attention: strides");
    TAttnArgs a;
    a.qkv = qkv; a.kpos = kpos; a.out = out; a.ld = p->ld; a.outLd = p->out_ld; a.T = p->T; a.C = p->C;
    a.window = p->window; a.HW = (long)p->H * p->W; a.roundFp16 = p->round_fp16; a.scale = p->scale;
    a.headDim = d;
    if (p->dtype == FLAIR_BF16)
        launch_temporal<bf16_t>(a, stream);
    else
        launch_temporal<float>(a, stream);
    FLAIR_LAUNCH_CHECK();
    return FLAIR_OK;
}
