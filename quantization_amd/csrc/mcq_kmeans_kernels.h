// mcq_kmeans_kernels.h -- gfx950 kernels of one Lloyd step over the coarse centroids (include/mcq_kmeans.h, rules 44-47): the
// nearest centroid of every training vector, and the members' mean per list.  The score and the order are those of the coarse
// probes (rule 41, pair_less), the staging (coarse_load, coarse_store, the pitch of 34) is that of mcq_coarse_kernels.h and the
// row-bounded gather (rerank_row, rerank_load) that of mcq_rerank_kernels.h; nothing of those files is changed.  The fp16 form of
// the step (mcq_half_kernels.h, rules 48-51) and the bf16 form (mcq_bf16_kernels.h, rules 56-59) have an assign kernel of their own
// each and share the rest: k_kmeans_finish, k_kmeans_scan, k_kmeans_sums (its ROW tag) and k_kmeans_mean.
//
// k_kmeans_assign: one workgroup of 4 waves per (tile of 128 vectors, part of the centroid tiles of 128).  A wave owns a 64 x 64
// block as 2 x 2 accumulators of 32 x 32 and runs v_mfma_f32_32x32x2_f32 with the CENTROIDS as the A operand: lane l supplies
// centroid rows l % 32 (+ 32) and vector rows l % 32 (+ 32) of its block at k = l / 32 and receives, in register r of
// accumulator (vi, ci), the dot of vector 32 vi + l % 32 with centroid 32 ci + 8 (r / 4) + 4 (l / 32) + r % 4.  So a lane holds
// TWO vectors and 32 centroids of each, the four 8-byte LDS words it reads per two k steps feed eight MFMAs (k_coarse_scores:
// two words, two MFMAs), and the running best (score, list) of a vector is one register pair per lane that is compared under
// pair_less after every tile with no step across lanes.  A product does not depend on which operand carries which factor, and
// every accumulator sees the steps of rule 41 in its order, so the scores keep rule 41's bits (tests/test_gpu_kmeans.py holds
// them to mcq_coarse_probe's).  D goes in chunks of 32 elements through LDS, double-buffered, one barrier a chunk: thread t
// stages elements [4 (t % 8), 4 (t % 8) + 4) of vector rows and centroid rows t / 8 + 32 j, j < 4.  At the end of the part the
// two halves of a wave meet through one shuffle and the two waves that share a vector through LDS; part s of vector v leaves as
// one pair at [v * parts + s].  LDS 69,632 B (2 buffers of 256 rows x 34 floats): two workgroups per compute unit.
//
// k_kmeans_finish: one thread per vector takes the least pair of its parts, writes assign and score and, with prev_assign,
// counts the changes: one integer atomic per wave on `changed`, which block 0 of k_kmeans_assign zeroed.
//
// k_kmeans_scan: one workgroup: block_first[l] = the number of blocks of 4,096 members in the lists before l.
// k_kmeans_sums: one workgroup per (block, slab of 1,024 elements); it finds its (list, block) by binary search in block_first, a
// surplus workgroup exits.  A wave owns a quarter of 1,024 members and a lane 16 float64 accumulators, elements 256 t + 4 lane
// + j of the slab; the rows of four members are loaded (16 loads a lane) before the first add and added in member order.  A
// row is read through a descriptor that covers that row alone; a member that names no row, and an element past D, reads +0.0
// without a memory access, and an accumulator that starts at +0.0 is never -0.0, so adding it changes no bit.  The quarter sums
// meet in LDS (32 KiB) as ((q0 + q1) + q2) + q3.  ROW = kRowF16: the rows are fp16 (rerank_row<true>, rerank_load<true, VEC>, one
// 8-byte load per group of four under VEC), each element widened exactly (fp16 -> fp32 -> float64) into the same tree.  ROW =
// kRowBf16: the rows are bf16, read through the same 2-byte descriptor, each element widened exactly as its bits shifted left by
// 16 (kmeans_row_load).
// k_kmeans_mean: one workgroup per (list, slab) counts the list's members that name a row, adds its block sums in ascending
// order, divides in float64 and rounds once; an empty list copies centroids_in.
#pragma once
#include "mcq_coarse_kernels.h"

namespace mcq {

// ---- launch arithmetic (mcq_kmeans_parts and mcq_kmeans_blocks of mcq_api.hip are the plan)
constexpr int kKmWaves = 4;                // waves per workgroup, every kernel of this file
constexpr int kKmVT = 128;                 // vectors of a tile
constexpr int kKmCT = 128;                 // centroid rows of a tile
constexpr int kKmFullBlocks = 512;         // vector tiles that fill the chip alone: two workgroups per CU
constexpr int kKmStageFloats = (kKmVT + kKmCT) * kCoarsePitch;   // one buffer: the vector rows, then the centroid rows
constexpr int kKmLds = 2 * kKmStageFloats * 4;
constexpr int kKmBlock = 4096;             // members of a block of the update's tree
constexpr int kKmQuarter = kKmBlock / kKmWaves;   // members a wave sums sequentially
constexpr int kKmSlab = 1024;              // elements of a row one workgroup sums: 16 per lane
constexpr int kKmRows = 4;                 // members whose loads are issued before the first add
static_assert(kKmVT == 32 * 64 * kKmWaves / 64 && kKmVT * 8 == 4 * 64 * kKmWaves, "a thread stages one group of four rows of each operand");
static_assert(kKmStageFloats * 4 >= kKmVT * 8, "the last reduction borrows the first staging buffer");
static_assert(kKmSlab == 16 * 64 && 64 % kKmRows == 0, "16 accumulators a lane; a batch of rows never straddles 64 members");

__global__ void __launch_bounds__(64 * kKmWaves)
k_kmeans_assign(const float *__restrict__ vectors, int B, const float *__restrict__ centroids, int L, int D,
                const float *__restrict__ terms, int parts, int vec, float *__restrict__ part_score, int *__restrict__ part_list,
                int *__restrict__ changed) {
    extern __shared__ __attribute__((aligned(16))) char kmeans_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int vt = blockIdx.x / parts, part = blockIdx.x % parts;
    if (changed && blockIdx.x == 0 && tid == 0) *changed = 0;      // (k_kmeans_finish counts behind this kernel)
    const long v0 = (long)vt * kKmVT;
    const long T = ((long)L + kKmCT - 1) / kKmCT;
    const long lo = T * part / parts, hi = T * (part + 1) / parts;

    float *stage = reinterpret_cast<float *>(kmeans_smem);
    const int srow = tid >> 3, scol = (tid & 7) * 4;         // staging: this thread's first row and first element of a chunk
    const int frow = lane & 31, half = lane >> 5;            // fragments: this lane's row and k of a step
    const int wv = (wave & 1) * 64, wc = (wave >> 1) * 64;   // this wave's block of the tile
    const int chunks = (D + kCoarseDC - 1) / kCoarseDC;
    float4 rv[4], rc[4];
    auto load = [&](long tile, int c) {
        const int e = c * kCoarseDC + scol;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rv[j] = coarse_load(vectors, v0 + srow + 32 * j, B, D, e, vec);
            rc[j] = coarse_load(centroids, tile * kKmCT + srow + 32 * j, L, D, e, vec);
        }
    };
    auto store = [&](int buf) {
        float *b = stage + buf * kKmStageFloats;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            coarse_store(b + (srow + 32 * j) * kCoarsePitch + scol, rv[j]);
            coarse_store(b + (kKmVT + srow + 32 * j) * kCoarsePitch + scol, rc[j]);
        }
    };

    float bs[2] = {__builtin_inff(), __builtin_inff()};      // the running best of vectors wv + frow and wv + 32 + frow
    int bi[2] = {kNoIndex, kNoIndex};
    for (long tile = lo; tile < hi; ++tile) {
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
            const float *b = stage + (c & 1) * kKmStageFloats;
            const float *va = b + (wv + frow) * kCoarsePitch + 2 * half;
            const float *ca = b + (kKmVT + wc + frow) * kCoarsePitch + 2 * half;
#pragma unroll
            for (int m = 0; m < kCoarseDC / 4; ++m) {
                float2 x[2], y[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    x[i] = *reinterpret_cast<const float2 *>(va + 32 * i * kCoarsePitch + 4 * m);
                    y[i] = *reinterpret_cast<const float2 *>(ca + 32 * i * kCoarsePitch + 4 * m);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)                  // step 2 m of the four accumulators, then step 2 m + 1
                    acc[a >> 1][a & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(y[a & 1].x, x[a >> 1].x, acc[a >> 1][a & 1], 0, 0, 0);
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    acc[a >> 1][a & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(y[a & 1].y, x[a >> 1].y, acc[a >> 1][a & 1], 0, 0, 0);
            }
            if (c + 1 < chunks) store((c + 1) & 1);
            __syncthreads();
        }
        // this lane's two vectors against its 32 centroids of the tile
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long cl = tile * kKmCT + wc + 32 * ci + 8 * (r / 4) + 4 * half + (r % 4);
                if (cl < L) {
                    const int c = (int)cl;
                    const float term = terms[c];
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
    float *ms = stage;
    int *mi = reinterpret_cast<int *>(stage + kKmVT);
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

// B == 0: nothing but the zero of `changed`
__global__ void __launch_bounds__(64 * kKmWaves)
k_kmeans_finish(const float *__restrict__ part_score, const int *__restrict__ part_list, int B, int parts,
                const int *__restrict__ prev, int *__restrict__ assign, float *__restrict__ score, int *__restrict__ changed) {
    if (B == 0) {
        if (changed && threadIdx.x == 0) *changed = 0;
        return;
    }
    const long v = (long)blockIdx.x * (64 * kKmWaves) + threadIdx.x;
    bool differs = false;
    if (v < B) {
        float bs = __builtin_inff();
        int bi = kNoIndex;
        for (int s = 0; s < parts; ++s) {
            const float os = part_score[v * parts + s];
            const int oi = part_list[v * parts + s];
            if (pair_less(os, oi, bs, bi)) {
                bs = os;
                bi = oi;
            }
        }
        const int a = bi == kNoIndex ? -1 : bi;
        assign[v] = a;
        score[v] = bs;
        differs = prev && prev[v] != a;
    }
    if (prev) {
        const int n = __builtin_popcountll(__ballot(differs));
        if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(changed, n);
    }
}

// the positions [lo, hi) of list l in `order`, cut to [0, B): offsets that build_lists did not make reach no other memory
__device__ __forceinline__ void kmeans_list(const int64_t *__restrict__ off, long l, long B, long &lo, long &hi) {
    const long a = off[l], z = off[l + 1];
    lo = a < 0 ? 0 : (a > B ? B : a);
    hi = z < lo ? lo : (z > B ? B : z);
}

__global__ void __launch_bounds__(64 * kKmWaves)
k_kmeans_scan(const int64_t *__restrict__ off, int L, long B, int64_t *__restrict__ first) {
    constexpr int THREADS = 64 * kKmWaves;
    __shared__ long s[THREADS];
    const int tid = threadIdx.x;
    long carry = 0;
    for (long base = 0; base < L; base += THREADS) {
        const long l = base + tid;
        long nb = 0;
        if (l < L) {
            long lo, hi;
            kmeans_list(off, l, B, lo, hi);
            nb = (hi - lo + kKmBlock - 1) / kKmBlock;
        }
        s[tid] = nb;
        __syncthreads();
        for (int d = 1; d < THREADS; d <<= 1) {
            const long t = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        if (l < L) first[l] = carry + s[tid] - nb;
        carry += s[THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) first[L] = carry;
}

// the type of a vector row: what the host paths and k_kmeans_sums are instantiated by (two of them are two bytes wide)
constexpr int kRowF32 = 0, kRowF16 = 1, kRowBf16 = 2;

// rerank_load for a row of type ROW: the four elements of one lane and trip as fp32, from element e of the row on
template <int ROW, bool VEC>
__device__ __forceinline__ void kmeans_row_load(float (&x)[4], __amdgpu_buffer_rsrc_t rs, int e) {
    if constexpr (ROW != kRowBf16) {
        rerank_load<ROW == kRowF16, VEC>(x, rs, e);
    } else if constexpr (VEC) {
        const rerank_v2i raw = __builtin_amdgcn_raw_buffer_load_b64(rs, e * 2, 0, 0);
        const unsigned lo = (unsigned)raw[0], hi = (unsigned)raw[1];             // elements e, e + 1 | e + 2, e + 3
        x[0] = __uint_as_float(lo << 16);
        x[1] = __uint_as_float(lo & 0xffff0000u);
        x[2] = __uint_as_float(hi << 16);
        x[3] = __uint_as_float(hi & 0xffff0000u);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            x[j] = __uint_as_float((unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rs, (e + j) * 2, 0, 0) << 16);
    }
}

// cap: the blocks block_sums holds (the grid's x); sums is [cap][D]
template <int ROW, bool VEC>
__global__ void __launch_bounds__(64 * kKmWaves)
k_kmeans_sums(const void *__restrict__ vectors, long B, int D, const int64_t *__restrict__ order,
              const int64_t *__restrict__ off, int L, const int64_t *__restrict__ first, long cap, double *__restrict__ sums) {
    __shared__ double quarter[kKmWaves * kKmSlab];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = blockIdx.x;
    const int slab = blockIdx.y;
    if (g >= first[L] || g >= cap) return;                   // (uniform) a surplus workgroup
    long a = 0, z = L;                                       // first[a] <= g < first[z]: the last such a is the block's list
    while (z - a > 1) {
        const long mid = a + (z - a) / 2;
        if (first[mid] <= g) a = mid;
        else z = mid;
    }
    long lo, hi;
    kmeans_list(off, a, B, lo, hi);
    const long p0 = lo + (g - first[a]) * kKmBlock + (long)wave * kKmQuarter;
    const long p1 = p0 + kKmQuarter < hi ? p0 + kKmQuarter : hi;
    double acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = 0.0;
    const int e0 = slab * kKmSlab + lane * 4;
#pragma unroll 1
    for (long p = p0; p < p1; p += 64) {
        int row = -1;                                        // lane j: the row of member p + j, -1 where it names none
        if (p + lane < p1) {
            const int64_t r = order[p + lane];
            if (r >= 0 && r < B) row = (int)r;
        }
        const int n = p1 - p < 64 ? (int)(p1 - p) : 64;
#pragma unroll 1
        for (int j0 = 0; j0 < n; j0 += kKmRows) {
            float x[kKmRows][4][4];
#pragma unroll
            for (int r = 0; r < kKmRows; ++r) {
                const __amdgpu_buffer_rsrc_t rs = rerank_row<ROW != kRowF32>(vectors, __builtin_amdgcn_readlane(row, j0 + r), D);
#pragma unroll
                for (int t = 0; t < 4; ++t) kmeans_row_load<ROW, VEC>(x[r][t], rs, e0 + 256 * t);
            }
#pragma unroll
            for (int r = 0; r < kKmRows; ++r)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[t][j] = acc[t][j] + (double)x[r][t][j];
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) quarter[wave * kKmSlab + 256 * t + lane * 4 + j] = acc[t][j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kKmSlab / (64 * kKmWaves); ++i) {
        const int e = tid + 64 * kKmWaves * i;
        const double sum = ((quarter[e] + quarter[kKmSlab + e]) + quarter[2 * kKmSlab + e]) + quarter[3 * kKmSlab + e];
        if (slab * kKmSlab + e < D) sums[g * D + slab * kKmSlab + e] = sum;
    }
}

__global__ void __launch_bounds__(64 * kKmWaves)
k_kmeans_mean(const int64_t *__restrict__ order, long B, const int64_t *__restrict__ off, const int64_t *__restrict__ first,
              long cap, const double *__restrict__ sums, int D, const float *__restrict__ centroids_in,
              float *__restrict__ centroids_out, int *__restrict__ counts) {
    constexpr int THREADS = 64 * kKmWaves;
    __shared__ int wave_n[kKmWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long l = blockIdx.x;
    const int slab = blockIdx.y;
    long lo, hi;
    kmeans_list(off, l, B, lo, hi);
    int n = 0;
    for (long p = lo + tid; p < hi; p += THREADS) {
        const int64_t r = order[p];
        n += r >= 0 && r < B;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m, 64);
    if (lane == 0) wave_n[wave] = n;
    __syncthreads();
    n = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    const long nb = (hi - lo + kKmBlock - 1) / kKmBlock, f = first[l];
    for (int i = 0; i < kKmSlab / THREADS; ++i) {
        const int e = slab * kKmSlab + tid + THREADS * i;
        if (e >= D) continue;
        float out = centroids_in[l * D + e];
        if (n > 0) {
            double sum = 0.0;
            for (long b = 0; b < nb && f + b < cap; ++b) sum = sum + sums[(f + b) * D + e];
            out = (float)(sum / (double)n);
        }
        centroids_out[l * D + e] = out;
    }
    if (slab == 0 && tid == 0) counts[l] = n;
}

}  // namespace mcq
