// mcq_bf16_kernels.h -- gfx950 kernels of the Lloyd step over a bf16 raw store (include/mcq_bf16.h, rules 56-59): the nearest
// centroid of every bf16 vector on the bf16 matrix cores.  The order (pair_less), the meeting of the parts (k_kmeans_finish)
// and the whole update (k_kmeans_scan, k_kmeans_sums<kRowBf16, VEC>, k_kmeans_mean) are those of mcq_kmeans_kernels.h; the
// branch-free row loads (half_load, half_keep), the chunk of 32 elements and the pitch of 80 bytes are those of
// mcq_half_kernels.h, which move 16-bit elements without looking into them.
//
// k_bf16_split: fp32 centroids -> three bf16 planes [hi: L rows][mid: L rows][lo: L rows] of Dp = 32 ceil(D / 32) elements
// each, once per call: hi = bf16(c), mid = bf16(c - f32(hi)), lo = bf16((c - f32(hi)) - f32(mid)), every conversion to nearest
// even, an element past D +0.0 in all three.  bf16 has fp32's exponent, so nothing is scaled (the fp16 lo plane is, by 2^11)
// and the three pieces of an element can share one accumulator.  One thread per group of 8 elements (one 16-byte store per
// plane), a grid-stride loop.
//
// k_kmeans_assign_bf16: one workgroup of 8 waves per (tile of 256 vectors, part of the centroid tiles of 128).  The fp16
// kernel's plan does not carry over: 128 vector rows and 3 x 128 plane rows at 80 bytes, double-buffered, are 81,920 B + 1,024 B
// of terms, two of which pass the 160 KiB of a compute unit by 2 KB, and one workgroup of 4 waves leaves a wave alone on its
// SIMD with nothing to cover its barriers.  So the tile is twice as tall and the workgroup twice as large: wave w owns the
// 64 x 64 block of vectors 64 (w % 4) and centroids 64 (w / 4) as 2 x 2 blocks of 32 x 32 and runs v_mfma_f32_32x32x16_bf16 with
// the CENTROIDS as the A operand: lane l supplies 8 consecutive elements of row l % 32 at k = 8 (l / 32) of a step of 16 and
// receives, in register r of block (vi, ci), the dot of vector 32 vi + l % 32 with centroid 32 ci + 8 (r / 4) + 4 (l / 32) + r % 4.
// Every block has ONE accumulator: four accumulators of 16 registers, 64 a lane (the fp16 kernel: 128).  A fragment is one
// 16-byte LDS read; a step reads eight (2 vector, 2 lo, 2 mid, 2 hi) and issues twelve MFMAs, the lo, then the mid, then the hi
// product of each block, so the small pieces are in the accumulator before the large one arrives; the four blocks alternate, so
// no MFMA waits for the one before it.  After a tile score = fl(h[l] - A), and the running best of a lane's two vectors is a
// register pair each, compared under pair_less with no step across lanes.
// D goes through LDS in chunks of 32 elements (two steps), double-buffered, one barrier a chunk.  A buffer is 640 rows (256
// vector, 128 hi, 128 mid, 128 lo) of 80 bytes = 20 banks: the 16 lanes whose 16-byte reads are served together read rows
// 20 i mod 64 = 4 (5 i mod 16) banks apart and cover the 64 banks once.  Thread t stages elements [8 (t % 4), 8 (t % 4) + 8) of
// vector rows t / 4 and t / 4 + 128 and of row t / 4 of each plane: five 16-byte registers.  A plane row is always one 16-byte
// load; a vector row is one where D % 8 == 0 and the base is 16-byte aligned (VEC, the host decides) and eight 2-byte loads
// otherwise -- the same bits to the same places.  No load stands under a branch (half_load): an absent row or element reads one
// that is there, and the zero goes in at the LDS store, behind the chunk's products.  Each plane row is staged once per 256
// vectors, where the fp16 kernel stages its rows once per 128.
// The terms of a tile's 128 centroids sit in LDS too (two tiles of 512 B, by tile parity).
// LDS 2 x 640 x 80 + 1,024 = 103,424 B: ONE workgroup per compute unit, 8 waves, two per SIMD, so at most 256 registers a lane
// (__launch_bounds__(512, 2)); profiles/kmeans_bf16_isa.txt has the compiler's report for both forms: no scratch.  The parts
// that fill the chip are therefore counted in tiles of 256 vectors against 256 workgroups (kBfFullBlocks), not rule 44's 512.
// At the end of the part the halves of a wave meet through one shuffle and the two waves of a vector (w and w + 4) through LDS.
//
// The update's sums over bf16 rows are the kRowBf16 form of k_kmeans_sums (mcq_kmeans_kernels.h), not a kernel of this file.
#pragma once
#include "mcq_half_kernels.h"

namespace mcq {

// ---- launch arithmetic (mcq_kmeans_bf16_parts and mcq_kmeans_bf16_planes of mcq_api.hip are the plan)
constexpr int kBfWaves = 8;                // waves per workgroup of k_kmeans_assign_bf16
constexpr int kBfVT = 256;                 // vectors of a tile
constexpr int kBfFullBlocks = 256;         // vector tiles that fill the chip alone: one workgroup per CU
constexpr int kBfStageRows = kBfVT + 3 * kKmCT;          // one buffer: the vector rows, the hi, the mid and the lo rows
constexpr int kBfStageHalves = kBfStageRows * kHalfPitch;
constexpr int kBfLds = 2 * kBfStageHalves * 2;           // the staging; behind it the terms of two centroid tiles
constexpr int kBfLdsAll = kBfLds + 2 * kKmCT * 4;
static_assert(kBfStageRows * (kHalfDC / 8) == 5 * 64 * kBfWaves, "a thread stages two vector rows and one row of each plane");
static_assert(kBfVT == 4 * 64 && kKmCT == 2 * 64 && kBfWaves == 4 * 2, "a wave owns 64 vectors x 64 centroids of the tile");
static_assert(kBfStageHalves * 2 >= kBfVT * 8, "the last reduction borrows the first staging buffer");
static_assert(kBfLdsAll <= 160 * 1024 && kBfLds % 16 == 0, "one workgroup per compute unit");

typedef __bf16 bf16_v8 __attribute__((ext_vector_type(8)));

// bf16(x), round to nearest even, as bits; a NaN stays a NaN, a finite x past the bf16 range becomes an infinity
__device__ __forceinline__ unsigned bf16_bits(float x) {
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ float bf16_widen(unsigned bits) { return __uint_as_float(bits << 16); }

__global__ void __launch_bounds__(64 * kKmWaves)
k_bf16_split(const float *__restrict__ centroids, int L, int D, unsigned short *__restrict__ planes) {
    const int Dp = half_padded_dim(D), groups = Dp / 8;
    const long total = (long)L * groups;
    for (long g = (long)blockIdx.x * (64 * kKmWaves) + threadIdx.x; g < total; g += (long)gridDim.x * (64 * kKmWaves)) {
        const long row = g / groups;
        const int e = (int)(g % groups) * 8;
        unsigned hi[8], mid[8], lo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float c = e + j < D ? centroids[row * D + e + j] : 0.f;
            hi[j] = bf16_bits(c);
            const float rest = c - bf16_widen(hi[j]);        // (exact in fp32, and so is the next)
            mid[j] = bf16_bits(rest);
            lo[j] = bf16_bits(rest - bf16_widen(mid[j]));
        }
        unsigned short *at = planes + row * Dp + e;
        *reinterpret_cast<uint4 *>(at) = make_uint4(hi[0] | hi[1] << 16, hi[2] | hi[3] << 16, hi[4] | hi[5] << 16, hi[6] | hi[7] << 16);
        *reinterpret_cast<uint4 *>(at + (long)L * Dp) =
            make_uint4(mid[0] | mid[1] << 16, mid[2] | mid[3] << 16, mid[4] | mid[5] << 16, mid[6] | mid[7] << 16);
        *reinterpret_cast<uint4 *>(at + 2 * (long)L * Dp) =
            make_uint4(lo[0] | lo[1] << 16, lo[2] | lo[3] << 16, lo[4] | lo[5] << 16, lo[6] | lo[7] << 16);
    }
}

// planes: what k_bf16_split wrote for these centroids.  Part s of vector v leaves as one pair at [v * parts + s]
template <bool VEC>
__global__ void __launch_bounds__(64 * kBfWaves, 2)
k_kmeans_assign_bf16(const unsigned short *__restrict__ vectors, int B, const unsigned short *__restrict__ planes, int L, int D,
                     const float *__restrict__ terms, int parts, float *__restrict__ part_score, int *__restrict__ part_list,
                     int *__restrict__ changed) {
    extern __shared__ __attribute__((aligned(16))) char bf16_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int vt = blockIdx.x / parts, part = blockIdx.x % parts;
    if (changed && blockIdx.x == 0 && tid == 0) *changed = 0;      // (k_kmeans_finish counts behind this kernel)
    const long v0 = (long)vt * kBfVT;
    const long T = ((long)L + kKmCT - 1) / kKmCT;
    const long lo = T * part / parts, hi = T * (part + 1) / parts;
    const int Dp = half_padded_dim(D), chunks = Dp / kHalfDC;
    const long plane = (long)L * Dp;

    unsigned short *stage = reinterpret_cast<unsigned short *>(bf16_smem);
    const int srow = tid >> 2, scol = (tid & 3) * 8;         // staging: this thread's first row and first element of a chunk
    const int frow = lane & 31, half = lane >> 5;            // fragments: this lane's row and k group of a step
    const int wv = (wave & 3) * 64, wc = (wave >> 2) * 64;   // this wave's block of the tile
    float *tt = reinterpret_cast<float *>(bf16_smem + kBfLds);      // the terms of a tile's centroids, two tiles
    const unsigned short *vtile = vectors + v0 * D;
    const int vleft = (int)(B - v0);
    uint4 rv[2], rp[3];
    bool okv[2], okc;
    auto load = [&](long tile, int c) {
        const int e = c * kHalfDC + scol;
        const unsigned short *ctile = planes + tile * kKmCT * Dp;
        const int cleft = (int)(L - tile * kKmCT);
#pragma unroll
        for (int j = 0; j < 2; ++j) rv[j] = half_load<VEC>(vtile, srow + 128 * j, vleft, D, e, okv[j]);
#pragma unroll
        for (int p = 0; p < 3; ++p) rp[p] = half_load<true>(ctile + p * plane, srow, cleft, Dp, e, okc);   // (e < Dp: a padded row is wholly there)
    };
    auto store = [&](int buf) {
        unsigned short *b = stage + buf * kBfStageHalves + srow * kHalfPitch + scol;
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<uint4 *>(b + 128 * j * kHalfPitch) = half_keep(okv[j], rv[j]);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4 *>(b + (kBfVT + kKmCT * p) * kHalfPitch) = half_keep(okc, rp[p]);
    };

    float bs[2] = {__builtin_inff(), __builtin_inff()};      // the running best of vectors wv + frow and wv + 32 + frow
    int bi[2] = {kNoIndex, kNoIndex};
    for (long tile = lo; tile < hi; ++tile) {
        // the tile's terms, NaN for a centroid past L (its scores are NaN and pass nothing).  Buffer tile % 2: a wave that is
        // still in the epilogue of the tile before reads the other one, and the readers of this one passed a barrier since
        float *tw = tt + (tile & 1) * kKmCT;
        if (tid < kKmCT) {
            const long cl = tile * kKmCT + tid;
            const float t = terms[cl < L ? cl : L - 1];
            tw[tid] = cl < L ? t : __builtin_nanf("");
        }
        load(tile, 0);
        store(0);
        __syncthreads();
        coarse_f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a >> 1][a & 1][r] = 0.f;
        for (int c = 0; c < chunks; ++c) {
            if (c + 1 < chunks) load(tile, c + 1);
            const unsigned short *b = stage + (c & 1) * kBfStageHalves + 8 * half;
            const unsigned short *va = b + (wv + frow) * kHalfPitch;
            const unsigned short *pa = b + (kBfVT + wc + frow) * kHalfPitch;
#pragma unroll
            for (int s = 0; s < kHalfDC / 16; ++s) {
                bf16_v8 x[2], y[3][2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    x[i] = *reinterpret_cast<const bf16_v8 *>(va + 32 * i * kHalfPitch + 16 * s);
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        y[p][i] = *reinterpret_cast<const bf16_v8 *>(pa + (kKmCT * p + 32 * i) * kHalfPitch + 16 * s);
                }
#pragma unroll
                for (int p = 2; p >= 0; --p)                 // step 2 c + s of the four blocks: lo, then mid, then hi
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        acc[a >> 1][a & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(y[p][a & 1], x[a >> 1], acc[a >> 1][a & 1], 0, 0, 0);
            }
            if (c + 1 < chunks) store((c + 1) & 1);
            __syncthreads();
        }
        // this lane's two vectors against its 32 centroids of the tile
        const int first = (int)(tile * kKmCT), left = L - first;
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c0 = wc + 32 * ci + 8 * (r / 4) + 4 * half + (r % 4);
                if (c0 < left) {
                    const int c = first + c0;
                    const float term = tw[c0];
#pragma unroll
                    for (int vi = 0; vi < 2; ++vi) {
                        const float sc = term - acc[vi][ci][r];
                        if (pair_less(sc, c, bs[vi], bi[vi])) {
                            bs[vi] = sc;
                            bi[vi] = c;
                        }
                    }
                }
            }
    }
    // the four holders of a vector: the halves of a wave, then waves w and w + 4 (the staging is free behind the last barrier)
    float *ms = reinterpret_cast<float *>(bf16_smem);
    int *mi = reinterpret_cast<int *>(ms + kBfVT);
#pragma unroll
    for (int vi = 0; vi < 2; ++vi) {
        const float os = __shfl_xor(bs[vi], 32, 64);
        const int oi = __shfl_xor(bi[vi], 32, 64);
        if (pair_less(os, oi, bs[vi], bi[vi])) {
            bs[vi] = os;
            bi[vi] = oi;
        }
        if (wave >= 4 && half == 0) {
            ms[wv + 32 * vi + frow] = bs[vi];
            mi[wv + 32 * vi + frow] = bi[vi];
        }
    }
    __syncthreads();
    if (wave < 4 && half == 0) {
#pragma unroll
        for (int vi = 0; vi < 2; ++vi) {
            const int at = wv + 32 * vi + frow;
            const float os = ms[at];
            const int oi = mi[at];
            if (pair_less(os, oi, bs[vi], bi[vi])) {
                bs[vi] = os;
                bi[vi] = oi;
            }
            if (v0 + at < B) {
                part_score[(v0 + at) * parts + part] = bs[vi];
                part_list[(v0 + at) * parts + part] = bi[vi];
            }
        }
    }
}

}  // namespace mcq
