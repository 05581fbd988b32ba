// mcq_split_kernels.h -- gfx950 kernel of the Lloyd step for fp32 rows on the bf16 matrix cores (include/mcq_split.h, rules
// 60-63): the nearest centroid of every fp32 vector from six products of bf16 planes.  The order (pair_less), the meeting of
// the parts (k_kmeans_finish) and the whole update are those of mcq_kmeans_kernels.h; the split of the centroids (k_bf16_split,
// bf16_widen) is that of mcq_bf16_kernels.h, unchanged; the plane row loads (half_load<true>, half_keep), the chunk of 32
// elements and the pitch of 80 bytes are those of mcq_half_kernels.h.
//
// k_kmeans_assign_split: one workgroup of 4 waves per (tile of 128 vectors, part of the centroid tiles of 128), one workgroup
// per compute unit.  BOTH operands are three bf16 planes: hi = bf16(v), mid = bf16(v - hi), lo = bf16((v - hi) - mid), every
// conversion to nearest even.  The centroids' planes come from k_bf16_split, once per call; a vector is split HERE, while its
// chunk goes from registers to LDS, so no plane copy of the store exists.  Wave w owns the 64 x 64 block of vectors 64 (w % 2)
// and centroids 64 (w / 2) as 2 x 2 blocks of 32 x 32 and runs v_mfma_f32_32x32x16_bf16 with the CENTROIDS as the A operand, the
// lane and register layout of k_kmeans_assign_bf16.  Every block has ONE accumulator (64 registers a lane).  A fragment is one
// 16-byte LDS read; a step reads twelve (2 row blocks x 3 planes, each side) and issues 24 MFMAs, two per fragment: per block, in
// rule 61's order (vector plane . centroid plane) lo.hi, mid.mid, hi.lo, mid.hi, hi.mid, hi.hi, so the small pieces are in the
// accumulator before the large one arrives, and on rows of bf16 numbers (mid = lo = +0.0) what is left is rule 57's lo, mid,
// hi.  The four blocks alternate inside each product, so no MFMA waits for the one before it.
// D goes through LDS in chunks of 32 elements (two steps), double-buffered, one barrier a chunk.  A buffer is 768 rows (128
// each of the vectors' hi, mid, lo and of the centroids' hi, mid, lo) of 80 bytes = 20 banks, conflict-free as in the 16-bit
// kernels.  Thread t stages elements [8 (t % 4), 8 (t % 4) + 8) of rows t / 4 and t / 4 + 64 of each side: for a vector row two
// 16-byte fp32 loads where D % 4 == 0 and the base is 16-byte aligned (VEC, the host decides) and eight 4-byte loads otherwise,
// the same bits to the same places; for each plane row one 16-byte load.  No load stands under a branch: an absent row or
// element reads one that is there, and the zero goes in at the LDS store, behind the chunk's products, where the split runs
// too: per pair of elements v_cvt_pk_bf16_f32, a shift and a mask (the widening), v_pk_add_f32, twice, and a third
// v_cvt_pk_bf16_f32: nine VALU instructions a pair, 72 a staged row group, then three 16-byte LDS stores.
// The terms of a tile's 128 centroids sit in LDS too (two tiles of 512 B, by tile parity).
// LDS 2 x 768 x 80 + 1,024 = 123,904 B: ONE workgroup per compute unit, one wave per SIMD, 512 registers a lane
// (__launch_bounds__(256, 1)); profiles/kmeans_split_isa.txt has the compiler's report for both forms: no scratch.  The parts
// that fill the chip are counted in tiles of 128 vectors against 256 workgroups (kSpFullBlocks).
// At the end of the part the halves of a wave meet through one shuffle and the two waves of a vector through LDS, as in
// k_kmeans_assign_half.
#pragma once
#include "mcq_bf16_kernels.h"

namespace mcq {

// ---- launch arithmetic (mcq_kmeans_split_parts and mcq_kmeans_split_planes of mcq_api.hip are the plan)
constexpr int kRowSplit = 3;               // beside kRowF32, kRowF16 and kRowBf16: fp32 rows that meet the centroids as planes
constexpr int kSpVT = 128;                 // vectors of a tile
constexpr int kSpFullBlocks = 256;         // vector tiles that fill the chip alone: one workgroup per CU
constexpr int kSpStageRows = 3 * kSpVT + 3 * kKmCT;      // one buffer: the vectors' hi, mid, lo rows, then the centroids'
constexpr int kSpStageHalves = kSpStageRows * kHalfPitch;
constexpr int kSpLds = 2 * kSpStageHalves * 2;           // the staging; behind it the terms of two centroid tiles
constexpr int kSpLdsAll = kSpLds + 2 * kKmCT * 4;
static_assert((kSpVT + 3 * kKmCT) * (kHalfDC / 8) == 8 * 64 * kKmWaves, "a thread stages two vector rows and two rows of each plane");
static_assert(kSpVT == 2 * 64 && kKmCT == 2 * 64 && kKmWaves == 2 * 2, "a wave owns 64 vectors x 64 centroids of the tile");
static_assert(kSpStageHalves * 2 >= kSpVT * 8, "the last reduction borrows the first staging buffer");
static_assert(kSpLdsAll <= 160 * 1024 && kSpLds % 16 == 0, "one workgroup per compute unit");

typedef __bf16 split_bf16x2 __attribute__((ext_vector_type(2)));
typedef float split_f32x2 __attribute__((ext_vector_type(2)));

// elements [e, e + 8) of fp32 row `row` of a tile whose first row `base` points at (wave-uniform) and from which on the array
// has `rows` >= 1 rows, as two groups of four.  The address is the uniform base and a 32-bit offset (a tile is at most 128 rows
// of 16,384 floats).  No load stands under a branch: an absent row or element reads row `rows - 1` or element 0 instead.  VEC
// (D % 4 == 0: a group of four lies wholly inside the row or wholly outside): the 16 bytes come back as loaded and ok[q] says
// whether group q counts; the zero goes in at the LDS store (split_store).  Element by element: masked here, ok is true
template <bool VEC>
__device__ __forceinline__ void split_load(const float *__restrict__ base, int row, int rows, int D, int e, float4 (&v)[2], bool (&ok)[2]) {
    const bool there = row < rows;
    const unsigned at = (unsigned)(there ? row : rows - 1) * (unsigned)D;
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            ok[q] = there && e + 4 * q < D;
            v[q] = *reinterpret_cast<const float4 *>(base + (at + (unsigned)(e + 4 * q < D ? e + 4 * q : 0)));
        }
    } else {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = base[at + (unsigned)(e + j < D ? e + j : 0)];
            f[j] = there && e + j < D ? x : 0.f;
        }
        ok[0] = ok[1] = true;
        v[0] = make_float4(f[0], f[1], f[2], f[3]);
        v[1] = make_float4(f[4], f[5], f[6], f[7]);
    }
}

// rule 60 for two elements: the pair's hi, mid and lo as packed bf16 (element 0 in the low half).  Both subtractions are
// exact in fp32; a bf16 widens as its bits shifted left by 16
__device__ __forceinline__ void split_pair(float a, float b, unsigned &hi, unsigned &mid, unsigned &lo) {
    split_f32x2 x = {a, b};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(x, split_bf16x2));
    x = split_f32x2{x.x - __uint_as_float(hi << 16), x.y - __uint_as_float(hi & 0xffff0000u)};
    mid = __builtin_bit_cast(unsigned, __builtin_convertvector(x, split_bf16x2));
    x = split_f32x2{x.x - __uint_as_float(mid << 16), x.y - __uint_as_float(mid & 0xffff0000u)};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(x, split_bf16x2));
}

// eight staged elements, +0.0 where they do not count, as their three planes to rows `at`, `at` + kSpVT and `at` + 2 kSpVT
__device__ __forceinline__ void split_store(unsigned short *at, const float4 (&v)[2], const bool (&ok)[2]) {
    unsigned hi[4], mid[4], lo[4];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        split_pair(ok[q] ? v[q].x : 0.f, ok[q] ? v[q].y : 0.f, hi[2 * q], mid[2 * q], lo[2 * q]);
        split_pair(ok[q] ? v[q].z : 0.f, ok[q] ? v[q].w : 0.f, hi[2 * q + 1], mid[2 * q + 1], lo[2 * q + 1]);
    }
    *reinterpret_cast<uint4 *>(at) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4 *>(at + kSpVT * kHalfPitch) = make_uint4(mid[0], mid[1], mid[2], mid[3]);
    *reinterpret_cast<uint4 *>(at + 2 * kSpVT * kHalfPitch) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// planes: what k_bf16_split wrote for these centroids.  Part s of vector v leaves as one pair at [v * parts + s]
template <bool VEC>
__global__ void __launch_bounds__(64 * kKmWaves, 1)
k_kmeans_assign_split(const float *__restrict__ vectors, int B, const unsigned short *__restrict__ planes, int L, int D,
                      const float *__restrict__ terms, int parts, float *__restrict__ part_score, int *__restrict__ part_list,
                      int *__restrict__ changed) {
    extern __shared__ __attribute__((aligned(16))) char split_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int vt = blockIdx.x / parts, part = blockIdx.x % parts;
    if (changed && blockIdx.x == 0 && tid == 0) *changed = 0;      // (k_kmeans_finish counts behind this kernel)
    const long v0 = (long)vt * kSpVT;
    const long T = ((long)L + kKmCT - 1) / kKmCT;
    const long lo = T * part / parts, hi = T * (part + 1) / parts;
    const int Dp = half_padded_dim(D), chunks = Dp / kHalfDC;
    const long plane = (long)L * Dp;

    unsigned short *stage = reinterpret_cast<unsigned short *>(split_smem);
    const int srow = tid >> 2, scol = (tid & 3) * 8;         // staging: this thread's first row and first element of a chunk
    const int frow = lane & 31, half = lane >> 5;            // fragments: this lane's row and k group of a step
    const int wv = (wave & 1) * 64, wc = (wave >> 1) * 64;   // this wave's block of the tile
    float *tt = reinterpret_cast<float *>(split_smem + kSpLds);     // the terms of a tile's centroids, two tiles
    const float *vtile = vectors + v0 * D;
    const int vleft = (int)(B - v0);
    float4 rv[2][2];
    uint4 rp[3][2];
    bool okv[2][2], okc[2];
    auto load = [&](long tile, int c) {
        const int e = c * kHalfDC + scol;
        const unsigned short *ctile = planes + tile * kKmCT * Dp;
        const int cleft = (int)(L - tile * kKmCT);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            split_load<VEC>(vtile, srow + 64 * j, vleft, D, e, rv[j], okv[j]);
#pragma unroll
            for (int p = 0; p < 3; ++p) rp[p][j] = half_load<true>(ctile + p * plane, srow + 64 * j, cleft, Dp, e, okc[j]);   // (e < Dp: a padded row is wholly there)
        }
    };
    auto store = [&](int buf) {
        unsigned short *b = stage + buf * kSpStageHalves + srow * kHalfPitch + scol;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            split_store(b + 64 * j * kHalfPitch, rv[j], okv[j]);
#pragma unroll
            for (int p = 0; p < 3; ++p)
                *reinterpret_cast<uint4 *>(b + (3 * kSpVT + kKmCT * p + 64 * j) * kHalfPitch) = half_keep(okc[j], rp[p][j]);
        }
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
            const unsigned short *b = stage + (c & 1) * kSpStageHalves + 8 * half;
            const unsigned short *va = b + (wv + frow) * kHalfPitch;
            const unsigned short *pa = b + (3 * kSpVT + wc + frow) * kHalfPitch;
#pragma unroll
            for (int s = 0; s < kHalfDC / 16; ++s) {
                bf16_v8 x[3][2], y[3][2];                    // [plane: hi, mid, lo][row block]
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        x[p][i] = *reinterpret_cast<const bf16_v8 *>(va + (kSpVT * p + 32 * i) * kHalfPitch + 16 * s);
                        y[p][i] = *reinterpret_cast<const bf16_v8 *>(pa + (kKmCT * p + 32 * i) * kHalfPitch + 16 * s);
                    }
                // step 2 c + s of the four blocks, rule 61's order: lo.hi, mid.mid, hi.lo, mid.hi, hi.mid, hi.hi
                constexpr int vp[6] = {2, 1, 0, 1, 0, 0}, cp[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
                for (int k = 0; k < 6; ++k)
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        acc[a >> 1][a & 1] =
                            __builtin_amdgcn_mfma_f32_32x32x16_bf16(y[cp[k]][a & 1], x[vp[k]][a >> 1], acc[a >> 1][a & 1], 0, 0, 0);
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
    // the four holders of a vector: the halves of a wave, then the two waves (the staging is free behind the last barrier)
    float *ms = reinterpret_cast<float *>(split_smem);
    int *mi = reinterpret_cast<int *>(ms + kSpVT);
#pragma unroll
    for (int vi = 0; vi < 2; ++vi) {
        const float os = __shfl_xor(bs[vi], 32, 64);
        const int oi = __shfl_xor(bi[vi], 32, 64);
        if (pair_less(os, oi, bs[vi], bi[vi])) {
            bs[vi] = os;
            bi[vi] = oi;
        }
        if (wave >= 2 && half == 0) {
            ms[wv + 32 * vi + frow] = bs[vi];
            mi[wv + 32 * vi + frow] = bi[vi];
        }
    }
    __syncthreads();
    if (wave < 2 && half == 0) {
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
