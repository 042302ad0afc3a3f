// Building blocks shared by the MFMA convolution kernels (conv.hip, chain.hip, dcn.hip).  gfx950 only, like common.h;
// everything here is __device__ __forceinline__ and restates what the kernels did inline: no helper may change the
// instructions a kernel issues or their order (the kernels' counted `s_waitcnt vmcnt(n)` depend on both).
//
// THE RULE these helpers were introduced under (profiles/mfma_tile_isa_diff.txt): a kernel uses a helper only where hipcc
// still emits the same instructions for it, or the same up to register names and the order of independent address
// arithmetic with unchanged registers, scratch, LDS, MFMA / LDS-DMA / s_barrier / s_waitcnt counts.  hipcc's schedule
// follows the source order closely, and in the hand-interleaved kernels (conv3x3_dma_kernel's epilogues,
// conv_resident_kernel's epilogue pieces, conv3x3_halo_kernel, act_vec and the slopes in chain.hip) a helper moved it; those
// keep their own copy of an idiom, with a comment that names this rule.  Before replacing such a copy, compare the assembly again.
//
// ---- the 32x32 accumulator and its octets ------------------------------------------------------------------------
// The kernels compute D^T (couts x pixels): weights are the MFMA A operand, pixels the B operand.  In the f32x16 result
// of a 32x32 MFMA, lane l holds pixel l & 31; with lh = l >> 5, register r holds cout 8 (r / 4) + 4 lh + r % 4 of the
// fragment: four register QUADS of 4 consecutive couts, quads 2 jj and 2 jj + 1 being couts 16 jj + 4 lh .. + 3 and
// 16 jj + 8 + 4 lh .. + 3.  A v_permlane32_swap of register 8 jj + e with register 8 jj + 4 + e exchanges the upper
// half-wave's first operand with the lower half-wave's second, after which lane l holds the OCTET of couts
// 16 jj + 8 lh .. + 7 of its pixel: one 16-byte bf16 piece (two f32 pieces) for stores, bias and residual loads.
//
// ---- LDS images ---------------------------------------------------------------------------------------------------
// Register-staged kernels (halo, K-split halo, chain) keep 64-byte rows (one pixel or one (cout, tap) of a K chunk) at
// an 80-byte PITCH: an odd multiple of 16 bytes, so the 32 rows of a ds_read_b128 fragment read are conflict-free;
// staged_row() (conv.hip) orders the ds_write_b128 pieces to match.  LDS-DMA kernels cannot pad (the DMA writes 64 lanes
// x 16 bytes linearly), so their rows are 64 bytes and the 16-byte piece is XOR-swizzled instead -- on the SOURCE
// address when staging, on the LDS address when reading: piece ^ ((column >> 2) & 3) for pixel rows,
// piece ^ ((cout >> 2) & 3) for weight rows (dma_frag_offsets, dma_halo_coords below).
#pragma once
#include "common.h"

// ---- the MFMA wrapper: one K step = 64 bytes of channels per row ---------------------------------------------------
template <typename E> struct Mma;

// bf16: one K step = 32 channels = two 32x32x16 MFMAs per (cout fragment, pixel fragment) pair.
template <> struct Mma<bf16_t> {
    static constexpr int BKE = 32;
    // fr[0], fr[1]: the two 16-byte chunks this lane needs from its 64-byte row.
    static __device__ __forceinline__ int chunk(int i, int half) { return 2 * i + half; }
    static __device__ __forceinline__ void run(const uint4 (&a)[2], const uint4 (&b)[2], f32x16& acc) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[0]),
                                                      __builtin_bit_cast(bf16x8, b[0]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[1]),
                                                      __builtin_bit_cast(bf16x8, b[1]), acc, 0, 0, 0);
    }
    // one half of the K step (16 channels)
    static __device__ __forceinline__ void run1(const uint4& a, const uint4& b, f32x16& acc) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                      acc, 0, 0, 0);
    }
    static constexpr int MFMA_PER_HALF = 1, MFMA_PER_STEP = 2;     // what run1 / run issue (sched_group_barrier counts)
};

// f32: one K step = 16 channels = eight 32x32x2 MFMAs.  Lane half h consumes channels
// 8h..8h+7 of the step (the same permutation on both operands, so the sum is complete).
template <> struct Mma<float> {
    static constexpr int BKE = 16;
    static __device__ __forceinline__ int chunk(int i, int half) { return 2 * half + i; }
    static __device__ __forceinline__ void run(const uint4 (&a)[2], const uint4 (&b)[2], f32x16& acc) {
        const float* af = reinterpret_cast<const float*>(a);
        const float* bf = reinterpret_cast<const float*>(b);
#pragma unroll
        for (int s = 0; s < 8; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[s], acc, 0, 0, 0);
    }
    static __device__ __forceinline__ void run1(const uint4& a, const uint4& b, f32x16& acc) {
        const float* af = reinterpret_cast<const float*>(&a);
        const float* bf = reinterpret_cast<const float*>(&b);
#pragma unroll
        for (int s = 0; s < 4; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[s], acc, 0, 0, 0);
    }
    static constexpr int MFMA_PER_HALF = 4, MFMA_PER_STEP = 8;
};

// ---- octet primitives ----------------------------------------------------------------------------------------------
// v = couts 16 jj + 8 lh .. + 7 of this lane's pixel (see the head of the file).  EVERY lane of the wave must call this:
// the swaps cross the half-waves, and under a divergent branch the active half is handed garbage.  Lanes whose couts or
// pixel are padding take part and drop their loads / stores instead.  (c by value: through a reference hipcc reads the
// whole accumulator ahead of the picks and schedules the surrounding code differently.)
__device__ __forceinline__ void acc_octet(const f32x16 c, int jj, float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const auto sw2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(c[8 * jj + e]), __float_as_uint(c[8 * jj + 4 + e]), false, false);
        v[e] = __uint_as_float(sw2[0]);
        v[4 + e] = __uint_as_float(sw2[1]);
    }
}

// Activation class 0: none / ReLU / LeakyReLU(0.1 | 0.2) as max(v, slope v), slope in [0, 1].
__device__ __forceinline__ float leaky_slope(int act) {
    return act == FLAIR_ACT_NONE ? 1.f : act == FLAIR_ACT_RELU ? 0.f : act == FLAIR_ACT_LRELU01 ? 0.1f : 0.2f;
}
template <int N>
__device__ __forceinline__ void leaky_act(float (&v)[N], float slope) {
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = fmaxf(v[e], v[e] * slope);
}
// The other classes (1 DCN offsets / masks, 2 SiLU, 3 exact GELU or "nothing") stay with their kernels: each copy's
// arithmetic differs on purpose (IEEE silu_f | v_rcp | exp2 with the scale folded in; dcn_offset_act | _fast) and the
// comment at each copy gives the measurement behind it.

// v[OFF .. OFF + VEC) += the 16-byte piece of residual elements at p (global memory), or a piece loaded earlier and
// kept in registers.  v: the VEC values of one piece, or an octet of which an f32 piece is one half (OFF = 0 | VEC).
template <typename E, int OFF = 0, int N>
__device__ __forceinline__ void add_piece(float (&v)[N], const E* p) {
    static_assert(OFF >= 0 && OFF + ET<E>::VEC <= N, "the piece lies inside v");
    float r[ET<E>::VEC];
    Vec16<E>::load(p, r);
#pragma unroll
    for (int e = 0; e < ET<E>::VEC; ++e) v[OFF + e] += r[e];
}
template <typename E, int OFF = 0, int N>
__device__ __forceinline__ void add_piece(float (&v)[N], const uint4& regs) { add_piece<E, OFF>(v, reinterpret_cast<const E*>(&regs)); }

// The buffer-descriptor form of the epilogue's end: store_piece(rsrc, pack_piece<E>(v), byteOff).  pack_piece: the
// 16-byte piece v[0 .. VEC) (bf16: an octet) in the element type; store_piece: one buffer store (FLAIR_OOB: dropped).
// Two calls, in this argument order, so that the pack stands ahead of the offset arithmetic as it did when every
// epilogue spelled this out (hipcc's schedule follows the source order).
template <typename E>
__device__ __forceinline__ u32x4_t pack_piece(const float* v) {
    alignas(16) E out[ET<E>::VEC];
    Vec16<E>::store(out, v);
    const uint4 ov = *reinterpret_cast<const uint4*>(out);
    return u32x4_t{ov.x, ov.y, ov.z, ov.w};
}
__device__ __forceinline__ void store_piece(__amdgpu_buffer_rsrc_t rsrc, u32x4_t piece, unsigned byteOff) {
    __builtin_amdgcn_raw_buffer_store_b128(piece, rsrc, (int)byteOff, 0, 0);
}

// ---- LDS-DMA images: 64-byte rows, 8 wavefronts, one image row of 32 pixels per fragment ----------------------------
// Fragment read offsets of lane (lr, lh) for the two 16-channel k-steps ks of a chunk.  A: weight row lr of a
// (tap, 32-cout fragment) block, piece 2 ks + lh; B: pixel row0 + kw + lr of the halo image, row0 = the first pixel of
// the wave's image row (a multiple of the 34-pixel pitch, so kw + lr is the column: the swizzle key), same piece.
__device__ __forceinline__ void dma_frag_offsets(int lr, int lh, int row0, unsigned (&aoff)[2], unsigned (&boff)[3][2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        aoff[ks] = (unsigned)(lr * 64 + (((2 * ks + lh) ^ ((lr >> 2) & 3)) << 4));
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
            boff[kw][ks] = (unsigned)((row0 + kw + lr) * 64 + (((2 * ks + lh) ^ (((kw + lr) >> 2) & 3)) << 4));
    }
}

// Halo DMA instruction k of a (rows x 34)-pixel image whose pixel (0, 0) is image pixel (h0 - 1, w0 - 1): lane (lrow =
// lane >> 2, lchunk = lane & 3) fills LDS row 16 k + lrow.  hpix: that pixel's index inside the H x W frame, 0xffffffff
// outside the image or past the last staged row (the DMA then writes zeros: zero padding); hpiece: byte offset of the
// swizzled 16-byte piece inside the pixel's 64-byte chunk.
__device__ __forceinline__ void dma_halo_coords(int k, int lrow, int lchunk, int rows, int h0, int w0, int H, int W, unsigned& hpix, unsigned& hpiece) {
    constexpr int HWP = 34;
    const int R = k * 16 + lrow;
    const int hr = R / HWP, c = R - hr * HWP;
    const int hh = h0 - 1 + hr, ww = w0 - 1 + c;
    const bool ok = R < rows * HWP && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W;
    hpix = ok ? (unsigned)(hh * W + ww) : 0xffffffffu;
    hpiece = (unsigned)((lchunk ^ ((c >> 2) & 3)) << 4);
}

// One chunk out of an LDS-DMA image pair for a wave that owns one image row: 3 column taps x 3 row taps x (2 cout
// fragments x 2 k-steps) MFMAs.  wb: the weight stage ([tap = 3 kh + kw][64 couts] rows), xb: the halo image (34-pixel
// rows).  Steps run column-major (kw = step / 3, kh = step % 3); the fragments of step n + 1 (A: 4 reads; B: 6 more when
// the column tap changes) are requested before the MFMAs of step n, in two alternating sets.  `hook(step)` runs after the MFMAs of a
// step have been issued (conv_resident_kernel: epilogue pieces, DMA instructions of a later stage); dma_no_hook where a
// kernel has none.
struct dma_no_hook {
    __device__ __forceinline__ void operator()(int) const {}
};
template <typename Hook>
__device__ __forceinline__ void dma_tap_loop(const char* wb, const char* xb, const unsigned (&aoff)[2], const unsigned (&boff)[3][2], f32x16 (&acc)[2], Hook&& hook) {
    constexpr int HWP = 34;
    uint4 fb[2][3][2];   // [set][halo row wave + h][k-step]
    uint4 fa[2][2][2];   // [set][cout fragment][k-step]
    auto load_b = [&](int set, int kw) {
#pragma unroll
        for (int h = 0; h < 3; ++h)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) fb[set][h][ks] = *reinterpret_cast<const uint4*>(xb + h * (HWP * 64) + boff[kw][ks]);
    };
    auto load_a = [&](int set, int kh, int kw) {
#pragma unroll
        for (int cf = 0; cf < 2; ++cf)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) fa[set][cf][ks] = *reinterpret_cast<const uint4*>(wb + (kh * 3 + kw) * 4096 + cf * 2048 + aoff[ks]);
    };
    load_b(0, 0);
    load_a(0, 0, 0);
#pragma unroll
    for (int step = 0; step < 9; ++step) {
        const int kq = step / 3, kh = step % 3;
        const int nkq = (step + 1) / 3, nkh = (step + 1) % 3;
        if (step < 8) {
            if (nkh == 0) load_b(nkq & 1, nkq);
            load_a((step + 1) & 1, nkh, nkq);
        }
#pragma unroll
        for (int cf = 0; cf < 2; ++cf) Mma<bf16_t>::run(fa[step & 1][cf], fb[kq & 1][kh], acc[cf]);
        hook(step);
    }
}
