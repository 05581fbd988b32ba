// mcq_half_kernels.h -- gfx950 kernels of the Lloyd step over an fp16 raw store (include/mcq_half.h, rules 48-51): the nearest
// centroid of every fp16 vector on the f16 matrix cores.  The order (pair_less), the tile plan and its recommended parts
// (kKmFullBlocks), the meeting of the parts (k_kmeans_finish) and the whole update (k_kmeans_scan, k_kmeans_sums<kRowF16, VEC>,
// k_kmeans_mean) are those of mcq_kmeans_kernels.h.
//
// k_half_split: fp32 centroids -> two fp16 planes [hi: L rows][lo: L rows] of Dp = 32 ceil(D / 32) halves each, once per call:
// hi = f16(c), lo = f16((c - f32(hi)) * 2^11), an element past D is +0.0 in both.  One thread per group of 8 elements (one
// 16-byte store per plane), a grid-stride loop.  The conversions stay out of the product loop, where every vector tile would
// repeat them on every centroid tile.
//
// k_kmeans_assign_half: one workgroup of 4 waves per (tile of 128 vectors, part of the centroid tiles of 128), as
// k_kmeans_assign.  A wave owns a 64 x 64 block as 2 x 2 blocks of 32 x 32 and runs v_mfma_f32_32x32x16_f16 with the CENTROIDS
// as the A operand: lane l supplies 8 consecutive halves of row l % 32 at k = 8 (l / 32) of a step of 16 elements and receives,
// in register r of block (vi, ci), the dot of vector 32 vi + l % 32 with centroid 32 ci + 8 (r / 4) + 4 (l / 32) + r % 4.  Every
// block has TWO accumulators, A_hi (vector x hi plane) and A_lo (vector x lo plane): eight accumulators of 16 registers, 128 a
// lane.  A fragment is one 16-byte LDS read; a step reads six (2 vector, 2 hi, 2 lo) and issues eight MFMAs, every vector
// fragment feeding four.  After a tile dot = fl(A_hi + fl(A_lo * 2^-11)), score = fl(h[l] - dot), and the running best of a lane's
// two vectors is a register pair each, compared under pair_less with no step across lanes.
// D goes through LDS in chunks of 32 halves (two steps), double-buffered, one barrier a chunk.  A buffer is 384 rows (128
// vector, 128 hi, 128 lo) with a pitch of 40 halves = 80 bytes = 20 banks: the 16 lanes whose 16-byte reads are served together
// read rows 20 i mod 64 = 4 (5 i mod 16) banks apart, a permutation of the sixteen 4-bank groups, so they cover the 64 banks
// once.  Thread t stages halves [8 (t % 4), 8 (t % 4) + 8) of rows t / 4 + 64 j, j < 2, of each of the three: six 16-byte
// registers.  A plane row is always one 16-byte load (the planes are 16-byte aligned and padded); a vector row is one 16-byte
// load where D % 8 == 0 and the base is 16-byte aligned (VEC, the host decides) and eight 2-byte loads otherwise -- the same
// bits to the same places.  A row past B or L and an element past D is +0.0: no load stands under a branch, it reads a row or
// an element that is there instead and the zero is put in when the registers go to LDS, behind the chunk's products, so the
// next chunk's loads are in flight meanwhile (half_load).
// The terms of a tile's 128 centroids sit in LDS too (two tiles of 512 B, by tile parity), so no global load stands between
// the products of two tiles.
// LDS 2 x 384 x 80 + 1,024 = 62,464 B: two workgroups per compute unit (160 KiB), two waves per SIMD, so at most 256 registers a
// lane: VEC takes 247 VGPRs, no AGPRs, no scratch (__launch_bounds__(256, 2)).  The element-wise form would spill 20 bytes a
// lane under that cap, so it is built for one wave per SIMD (215 VGPRs + 128 AGPRs, no scratch): one workgroup per compute unit
// for a store that is not 16-byte aligned or has D % 8 != 0.  profiles/kmeans_half_isa.txt has the compiler's report.  A chunk
// of 64 halves at a pitch of 72 would take 110,592 B and leave every store one workgroup per compute unit with nothing to cover
// its barriers.
// At the end of the part the halves of a wave meet through one shuffle and the two waves of a vector through LDS: the last 33
// lines of k_kmeans_assign, kept as a copy here because one shared function gave k_kmeans_assign two scalar registers fewer
// and every assign kernel another instruction text behind its loops (profiles/lloyd_fold_isa.txt).
//
// The update's sums over fp16 rows are the kRowF16 form of k_kmeans_sums (mcq_kmeans_kernels.h), not a kernel of this file.
#pragma once
#include "mcq_kmeans_kernels.h"

namespace mcq {

// ---- launch arithmetic (mcq_kmeans_half_planes of mcq_api.hip is the plan; the parts are rule 44's, kKmFullBlocks: this
// kernel too runs two workgroups per compute unit)
constexpr int kHalfDC = 32;                // halves of a D chunk: two steps of 16
constexpr int kHalfPitch = kHalfDC + 8;    // halves of a staged row
constexpr int kHalfStageHalves = (kKmVT + 2 * kKmCT) * kHalfPitch;   // one buffer: the vector rows, the hi rows, the lo rows
constexpr int kHalfLds = 2 * kHalfStageHalves * 2;      // the staging; behind it the terms of two centroid tiles
constexpr int kHalfLdsAll = kHalfLds + 2 * kKmCT * 4;
constexpr int kHalfSplitBlocks = 1 << 16;  // the most workgroups of k_half_split
constexpr float kHalfLoScale = 2048.f;     // 2^11
static_assert(kHalfPitch * 2 % 16 == 0 && kHalfDC % 16 == 0, "a fragment is one aligned 16-byte read; a chunk is whole steps");
static_assert((kKmVT + 2 * kKmCT) * (kHalfDC / 8) == 6 * 64 * kKmWaves, "a thread stages two rows of each of the three operands");
static_assert(kHalfStageHalves * 2 >= kKmVT * 8, "the last reduction borrows the first staging buffer");
static_assert(kHalfLdsAll * 2 <= 160 * 1024 && kHalfLds % 16 == 0, "two workgroups per compute unit");

typedef _Float16 half_f16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ constexpr int half_padded_dim(int D) { return (D + kHalfDC - 1) / kHalfDC * kHalfDC; }

__device__ __forceinline__ unsigned half_bits(float x) { return (unsigned)__half_as_ushort(__float2half_rn(x)); }

__global__ void __launch_bounds__(64 * kKmWaves)
k_half_split(const float *__restrict__ centroids, int L, int D, unsigned short *__restrict__ planes) {
    const int Dp = half_padded_dim(D), groups = Dp / 8;
    const long total = (long)L * groups;
    for (long g = (long)blockIdx.x * (64 * kKmWaves) + threadIdx.x; g < total; g += (long)gridDim.x * (64 * kKmWaves)) {
        const long row = g / groups;
        const int e = (int)(g % groups) * 8;
        unsigned hi[8], lo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float c = e + j < D ? centroids[row * D + e + j] : 0.f;
            const __half h = __float2half_rn(c);
            hi[j] = (unsigned)__half_as_ushort(h);
            lo[j] = half_bits((c - __half2float(h)) * kHalfLoScale);
        }
        unsigned short *at = planes + row * Dp + e;
        *reinterpret_cast<uint4 *>(at) = make_uint4(hi[0] | hi[1] << 16, hi[2] | hi[3] << 16, hi[4] | hi[5] << 16, hi[6] | hi[7] << 16);
        *reinterpret_cast<uint4 *>(at + (long)L * Dp) =
            make_uint4(lo[0] | lo[1] << 16, lo[2] | lo[3] << 16, lo[4] | lo[5] << 16, lo[6] | lo[7] << 16);
    }
}

// the eight halves [e, e + 8) of row `row` of a tile whose first row `base` points at (wave-uniform) and from which on the
// array has `rows` >= 1 rows; +0.0 past D and past the last row.  The address is the uniform base and a 32-bit offset (a tile
// is at most 128 rows of 16,384 halves).  No load stands under a branch: an absent row or element reads row `rows - 1` or
// element 0 instead.  VEC: the 16 bytes come back as loaded and `ok` says whether they count; the caller puts the zero in when
// it stores them to LDS, behind the products of the chunk before, so the loads of the next chunk stay in flight meanwhile (a
// select at the load, like a load under a per-lane branch, is waited for at once).  Element by element: masked here, `ok` is true
template <bool VEC>
__device__ __forceinline__ uint4 half_load(const unsigned short *__restrict__ base, int row, int rows, int D, int e, bool &ok) {
    const bool there = row < rows;
    const unsigned at = (unsigned)(there ? row : rows - 1) * (unsigned)D;
    if constexpr (VEC) {                                     // (D % 8 == 0: a group lies wholly inside the row or wholly outside)
        ok = there && e < D;
        return *reinterpret_cast<const uint4 *>(base + (at + (unsigned)(e < D ? e : 0)));
    } else {
        ok = true;
        unsigned h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned v = base[at + (unsigned)(e + j < D ? e + j : 0)];
            h[j] = there && e + j < D ? v : 0u;
        }
        return make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
    }
}

// v where it counts, else +0.0 (component by component: a select between two objects would go through memory)
__device__ __forceinline__ uint4 half_keep(bool ok, uint4 v) { return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u); }

// planes: what k_half_split wrote for these centroids.  Part s of vector v leaves as one pair at [v * parts + s]
template <bool VEC>
__global__ void __launch_bounds__(64 * kKmWaves, VEC ? 2 : 1)
k_kmeans_assign_half(const unsigned short *__restrict__ vectors, int B, const unsigned short *__restrict__ planes, int L, int D,
                     const float *__restrict__ terms, int parts, float *__restrict__ part_score, int *__restrict__ part_list,
                     int *__restrict__ changed) {
    extern __shared__ __attribute__((aligned(16))) char half_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int vt = blockIdx.x / parts, part = blockIdx.x % parts;
    if (changed && blockIdx.x == 0 && tid == 0) *changed = 0;      // (k_kmeans_finish counts behind this kernel)
    const long v0 = (long)vt * kKmVT;
    const long T = ((long)L + kKmCT - 1) / kKmCT;
    const long lo = T * part / parts, hi = T * (part + 1) / parts;
    const int Dp = half_padded_dim(D), chunks = Dp / kHalfDC;
    const unsigned short *lo_plane = planes + (long)L * Dp;

    unsigned short *stage = reinterpret_cast<unsigned short *>(half_smem);
    const int srow = tid >> 2, scol = (tid & 3) * 8;         // staging: this thread's first row and first half of a chunk
    const int frow = lane & 31, half = lane >> 5;            // fragments: this lane's row and k group of a step
    const int wv = (wave & 1) * 64, wc = (wave >> 1) * 64;   // this wave's block of the tile
    float *tt = reinterpret_cast<float *>(half_smem + kHalfLds);    // the terms of a tile's centroids, two tiles
    const unsigned short *vtile = vectors + v0 * D;
    const int vleft = (int)(B - v0);
    uint4 rv[2], rh[2], rl[2];
    bool okv[2], okc[2];
    auto load = [&](long tile, int c) {
        const int e = c * kHalfDC + scol;
        const long coff = tile * kKmCT * Dp;
        const int cleft = (int)(L - tile * kKmCT);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            rv[j] = half_load<VEC>(vtile, srow + 64 * j, vleft, D, e, okv[j]);
            rh[j] = half_load<true>(planes + coff, srow + 64 * j, cleft, Dp, e, okc[j]);     // (e < Dp: a padded row is wholly there)
            rl[j] = half_load<true>(lo_plane + coff, srow + 64 * j, cleft, Dp, e, okc[j]);
        }
    };
    auto store = [&](int buf) {
        unsigned short *b = stage + buf * kHalfStageHalves + srow * kHalfPitch + scol;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            *reinterpret_cast<uint4 *>(b + 64 * j * kHalfPitch) = half_keep(okv[j], rv[j]);
            *reinterpret_cast<uint4 *>(b + (kKmVT + 64 * j) * kHalfPitch) = half_keep(okc[j], rh[j]);
            *reinterpret_cast<uint4 *>(b + (kKmVT + kKmCT + 64 * j) * kHalfPitch) = half_keep(okc[j], rl[j]);
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
        coarse_f32x16 ah[2][2], al[2][2];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) ah[a >> 1][a & 1][r] = al[a >> 1][a & 1][r] = 0.f;
        for (int c = 0; c < chunks; ++c) {
            if (c + 1 < chunks) load(tile, c + 1);
            const unsigned short *b = stage + (c & 1) * kHalfStageHalves + 8 * half;
            const unsigned short *va = b + (wv + frow) * kHalfPitch;
            const unsigned short *ha = b + (kKmVT + wc + frow) * kHalfPitch;
            const unsigned short *la = ha + kKmCT * kHalfPitch;
#pragma unroll
            for (int s = 0; s < kHalfDC / 16; ++s) {
                half_f16x8 x[2], yh[2], yl[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    x[i] = *reinterpret_cast<const half_f16x8 *>(va + 32 * i * kHalfPitch + 16 * s);
                    yh[i] = *reinterpret_cast<const half_f16x8 *>(ha + 32 * i * kHalfPitch + 16 * s);
                    yl[i] = *reinterpret_cast<const half_f16x8 *>(la + 32 * i * kHalfPitch + 16 * s);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)                  // step 2 c + s of the four blocks: into A_hi, then into A_lo
                    ah[a >> 1][a & 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(yh[a & 1], x[a >> 1], ah[a >> 1][a & 1], 0, 0, 0);
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    al[a >> 1][a & 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(yl[a & 1], x[a >> 1], al[a >> 1][a & 1], 0, 0, 0);
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
                        const float low = al[vi][ci][r] * (1.f / kHalfLoScale);
                        const float dot = ah[vi][ci][r] + low;
                        const float sc = term - dot;
                        if (pair_less(sc, c, bs[vi], bi[vi])) {
                            bs[vi] = sc;
                            bi[vi] = c;
                        }
                    }
                }
            }
    }
    // the four holders of a vector: the halves of a wave, then the two waves (the staging is free behind the last barrier)
    float *ms = reinterpret_cast<float *>(half_smem);
    int *mi = reinterpret_cast<int *>(ms + kKmVT);
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
