// mcq_coarse_kernels.h -- gfx950 kernels of the coarse probes (include/mcq_coarse.h, rules 40-43): score every query against
// every coarse centroid on the fp32 matrix cores and keep the P best per query, exactly.  The order (pair_less), the merge list
// (WideList) and the row-bounded gather of the biases (rerank_row, rerank_group) are those of mcq_search_kernels.h,
// mcq_wide_kernels.h and mcq_rerank_kernels.h; nothing of those files is changed.
//
// k_coarse_scores: one workgroup of 4 waves per (tile of 32 queries, part of the centroid tiles).  A centroid tile is 128 rows,
// 32 per wave; a wave holds one 32 x 32 accumulator (16 registers) and runs v_mfma_f32_32x32x2_f32 with the QUERIES as the A
// operand: lane l supplies query row l % 32 and centroid row l % 32 of its wave at k = l / 32, and receives, in register r, the
// dot of query 8 (r / 4) + 4 (l / 32) + r % 4 with centroid l % 32.  So a lane holds ONE centroid and 16 queries, and the
// centroid's term is one load per lane and tile.
// D goes in chunks of 32 elements through LDS, double-buffered, one barrier a chunk.  Thread t stages elements [4 (t % 8),
// 4 (t % 8) + 4) of query row t / 8 and of centroid rows t / 8 + 32 j, j < 4: one 16-byte load each where D % 4 == 0 and the
// base pointers are 16-byte aligned (`vec`, the host decides), element by element otherwise -- the same values to the same
// places.  An element past D and a row past Q or L is +0.0 and is not loaded.  A staged row has a pitch of 34 floats and its
// groups of four are stored as (e0, e2 | e1, e3): the lane of half h = l / 32 then reads ONE 8-byte word at 4 m + 2 h per two
// k steps, (e_h, e_{2 + h}), which are its operands of steps 2 m (elements 4 m, 4 m + 1) and 2 m + 1 (4 m + 2, 4 m + 3): rule
// 41's "k ascends two elements a step".  With the pitch of 34 the 32 rows a half-wave reads start 2 banks apart (34 i mod 64 =
// 2 (17 i mod 32), a permutation of the even banks), so its 32 eight-byte reads cover the 64 banks once.
//
// Selection: a list per query of the tile in LDS, kCoarseM = 256 entries: [0, P) the P best so far, ascending under pair_less,
// behind them the pending entries.  After a tile's D loop a lane offers its 16 scores: one below that query's bound is appended
// behind an LDS integer counter per query (the only atomics).  A tile appends at most 128 entries to a list, so the wave that
// owns a query (8 queries per wave) sorts its list when fewer than 128 free entries are left, and at the end of the part: a
// bitonic network under pair_less over the smallest power of two that holds the P + pending entries (the rest of the list is
// (+inf, kNoIndex), behind every candidate), one wave, no workgroup barrier.  The bound is then the entry of rank P - 1.
// pair_less is a strict total order over what a list holds (a NaN never passes a bound; a centroid is offered once), so the
// result does not depend on the order of arrival, on the tile or part a centroid falls into, or on `parts`.
//
// k_coarse_finish: one workgroup per query merges the parts' lists through a WideList, writes the probes and their scores,
// and, with BIAS, recomputes <q, c> for the P winners alone as rule 29's plain fp32 dot (rerank_group under the inner product,
// 16 winners a wave and round): each row through a descriptor that covers that row alone, a tail entry makes no access.
#pragma once
#include "mcq_rerank_kernels.h"

namespace mcq {

// ---- launch arithmetic (mirrored by nothing: mcq_coarse_parts is the plan, and the caller may choose another)
constexpr int kCoarseMaxP = 128;           // the largest nprobe
constexpr int kCoarseMaxD = kRerankMaxD;   // the longest row (the finishing kernel stages the query as k_rerank does)
constexpr int kCoarseWaves = 4;            // waves per workgroup
constexpr int kCoarseQT = 32;              // queries of a tile
constexpr int kCoarseCT = 32 * kCoarseWaves;   // centroid rows of a tile
constexpr int kCoarseDC = 32;              // elements of a D chunk
constexpr int kCoarsePitch = kCoarseDC + 2;    // floats of a staged row
constexpr int kCoarseM = 256;              // entries of a query's list: P <= 128 sorted and room for a tile's 128
constexpr int kCoarseFullBlocks = 256;     // query tiles that fill the chip alone: one per CU
constexpr int kCoarseTargetBlocks = 512;   // workgroups mcq_coarse_parts aims at otherwise: two per CU
static_assert(kCoarseM >= kCoarseMaxP + kCoarseCT && (kCoarseM & (kCoarseM - 1)) == 0, "a list takes a whole tile behind P entries");
static_assert(kCoarseQT == 8 * kCoarseWaves && kCoarseQT * 8 == 64 * kCoarseWaves, "8 queries a wave; a thread stages one group of a query row");

constexpr int kCoarseStageFloats = (kCoarseQT + kCoarseCT) * kCoarsePitch;       // one buffer: the query rows, then the centroid rows
// LDS of k_coarse_scores: [2 staging buffers][scores 32 x 256][indexes 32 x 256][32 counters][32 bound scores][32 bound indexes]
constexpr int kCoarseLds = 2 * kCoarseStageFloats * 4 + kCoarseQT * kCoarseM * 8 + 3 * kCoarseQT * 4;
// LDS of k_coarse_finish: [the query, as k_rerank stages it (BIAS and parts > 0 only)][the wide list]
__host__ __device__ constexpr int coarse_finish_lds(bool bias, int D, int P) {
    return (bias ? rerank_query_floats(D) * 4 : 0) + wide_list_bytes(P);
}

typedef float coarse_f32x16 __attribute__((ext_vector_type(16)));

// the four elements [e, e + 4) of row `row` (of `rows`) of x; +0.0 past D and past the last row
__device__ __forceinline__ float4 coarse_load(const float *__restrict__ x, long row, long rows, int D, int e, int vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows) {
        const float *p = x + row * D + e;
        if (vec) {
            if (e < D) v = *reinterpret_cast<const float4 *>(p);                  // (D % 4 == 0: wholly inside the row)
        } else {
            if (e + 0 < D) v.x = p[0];
            if (e + 1 < D) v.y = p[1];
            if (e + 2 < D) v.z = p[2];
            if (e + 3 < D) v.w = p[3];
        }
    }
    return v;
}

// (e0, e2 | e1, e3): see the header comment
__device__ __forceinline__ void coarse_store(float *at, float4 v) {
    *reinterpret_cast<float2 *>(at) = make_float2(v.x, v.z);
    *reinterpret_cast<float2 *>(at + 2) = make_float2(v.y, v.w);
}

// what orders the LDS accesses of ONE wave against each other (its lanes exchange entries through LDS between two stages of
// the sort): LDS instructions of a wave complete in order, this keeps the compiler from moving them
__device__ __forceinline__ void coarse_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (one wave)  the list (s, i) of a query with n pending entries behind its P sorted ones: sorted, the pending part emptied,
// the bound refreshed
__device__ __forceinline__ void coarse_sort(float *s, int *i, int P, int n, int *cnt, float *bound_s, int *bound_i, int lane) {
    int m = 2;
    while (m < P + n) m <<= 1;                               // (P + n <= kCoarseM)
    coarse_wave_sync();
    for (int size = 2; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < m / 2; t += 64) {
                const int a = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), z = a | stride;
                const bool up = (a & size) == 0;
                const float sa = s[a], sz = s[z];
                const int ia = i[a], iz = i[z];
                if (pair_less(sz, iz, sa, ia) == up) {
                    s[a] = sz;
                    i[a] = iz;
                    s[z] = sa;
                    i[z] = ia;
                }
            }
            coarse_wave_sync();
        }
    }
    const float ts = s[P - 1];
    const int tb = i[P - 1];
    coarse_wave_sync();
    for (int e = P + lane; e < m; e += 64) {
        s[e] = __builtin_inff();
        i[e] = kNoIndex;
    }
    if (lane == 0) {
        *cnt = 0;
        *bound_s = ts;
        *bound_i = tb;
    }
    coarse_wave_sync();
}

// terms: L2 h[l] = 0.5 |c_l|^2, cosine r[l] = rnorm_of(|c_l|^2) (the caller passes NULL under the inner product: not read).
// part s of query q leaves as P entries, ascending, at part_score / part_list [(q * parts + s) * P]; the tail is (+inf, -1)
template <int METRIC>
__global__ void __launch_bounds__(64 * kCoarseWaves)
k_coarse_scores(const float *__restrict__ queries, int Q, const float *__restrict__ centroids, int L, int D,
                const float *__restrict__ terms, int P, int parts, int vec, float *__restrict__ part_score,
                int *__restrict__ part_list) {
    extern __shared__ __attribute__((aligned(16))) char coarse_smem[];
    constexpr int THREADS = 64 * kCoarseWaves;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x / parts, part = blockIdx.x % parts;
    const long q0 = (long)qt * kCoarseQT;
    const long T = ((long)L + kCoarseCT - 1) / kCoarseCT;
    const long lo = T * part / parts, hi = T * (part + 1) / parts;

    float *stage = reinterpret_cast<float *>(coarse_smem);
    float *ls = stage + 2 * kCoarseStageFloats;
    int *li = reinterpret_cast<int *>(ls + kCoarseQT * kCoarseM);
    int *cnt = li + kCoarseQT * kCoarseM;
    float *bound_s = reinterpret_cast<float *>(cnt + kCoarseQT);
    int *bound_i = reinterpret_cast<int *>(bound_s + kCoarseQT);
    for (int e = tid; e < kCoarseQT * kCoarseM; e += THREADS) {
        ls[e] = __builtin_inff();
        li[e] = kNoIndex;
    }
    if (tid < kCoarseQT) {
        cnt[tid] = 0;
        bound_s[tid] = __builtin_inff();
        bound_i[tid] = kNoIndex;
    }

    const int srow = tid >> 3, scol = (tid & 7) * 4;         // staging: this thread's row and first element of a chunk
    const int frow = lane & 31, half = lane >> 5;            // fragments: this lane's row and k of a step
    const int chunks = (D + kCoarseDC - 1) / kCoarseDC;
    float4 rq, rc[4];
    auto load = [&](long tile, int c) {
        const int e = c * kCoarseDC + scol;
        rq = coarse_load(queries, q0 + srow, Q, D, e, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) rc[j] = coarse_load(centroids, tile * kCoarseCT + srow + 32 * j, L, D, e, vec);
    };
    auto store = [&](int buf) {
        float *b = stage + buf * kCoarseStageFloats;
        coarse_store(b + srow * kCoarsePitch + scol, rq);
#pragma unroll
        for (int j = 0; j < 4; ++j) coarse_store(b + (kCoarseQT + srow + 32 * j) * kCoarsePitch + scol, rc[j]);
    };

    for (long tile = lo; tile < hi; ++tile) {
        load(tile, 0);
        store(0);
        __syncthreads();                                     // (and: the lists and bounds are as the tile before left them)
        coarse_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int c = 0; c < chunks; ++c) {
            if (c + 1 < chunks) load(tile, c + 1);
            const float *b = stage + (c & 1) * kCoarseStageFloats;
            const float *qa = b + frow * kCoarsePitch + 2 * half;
            const float *cb = b + (kCoarseQT + 32 * wave + frow) * kCoarsePitch + 2 * half;
#pragma unroll
            for (int m = 0; m < kCoarseDC / 4; ++m) {
                const float2 a = *reinterpret_cast<const float2 *>(qa + 4 * m);
                const float2 x = *reinterpret_cast<const float2 *>(cb + 4 * m);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, x.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, x.y, acc, 0, 0, 0);
            }
            if (c + 1 < chunks) store((c + 1) & 1);
            __syncthreads();
        }
        // the offers: this lane's centroid against its 16 queries
        const long cl = tile * kCoarseCT + 32 * wave + frow;
        if (cl < L) {
            const int c = (int)cl;
            float term = 0.f;
            if constexpr (METRIC != kMetricIP) term = terms[c];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = 8 * (r / 4) + 4 * half + (r % 4);
                float sc;
                if constexpr (METRIC == kMetricL2) sc = term - acc[r];
                else if constexpr (METRIC == kMetricIP) sc = -acc[r];
                else sc = -(acc[r] * term);
                if (q0 + qi < Q && pair_less(sc, c, bound_s[qi], bound_i[qi])) {
                    const int slot = P + atomicAdd(&cnt[qi], 1);
                    if (slot < kCoarseM) {                   // (a tile appends at most 128: defence alone)
                        ls[qi * kCoarseM + slot] = sc;
                        li[qi * kCoarseM + slot] = c;
                    }
                }
            }
        }
        __syncthreads();
        const bool last = tile + 1 == hi;
        for (int j = 0; j < 8; ++j) {
            const int qi = 8 * wave + j;
            int n = __builtin_amdgcn_readfirstlane(cnt[qi]);
            n = n > kCoarseM - P ? kCoarseM - P : n;
            if (n > 0 && (last || n + kCoarseCT > kCoarseM - P))
                coarse_sort(ls + qi * kCoarseM, li + qi * kCoarseM, P, n, cnt + qi, bound_s + qi, bound_i + qi, lane);
        }
    }
    __syncthreads();
    for (int e = tid; e < kCoarseQT * P; e += THREADS) {
        const int qi = e / P, p = e % P;
        if (q0 + qi < Q) {
            const long out = ((q0 + qi) * parts + part) * P + p;
            const int at = li[qi * kCoarseM + p];
            part_score[out] = ls[qi * kCoarseM + p];
            part_list[out] = at == kNoIndex ? -1 : at;
        }
    }
}

// parts == 0: no centroid at all (L == 0): the tail alone, and no input is read
template <bool BIAS>
__global__ void __launch_bounds__(64 * kWideWaves)
k_coarse_finish(const float *__restrict__ part_score, const int *__restrict__ part_list, int parts, int P,
                const float *__restrict__ queries, const float *__restrict__ centroids, int L, int D, int vec,
                int *__restrict__ out_list, float *__restrict__ out_score, float *__restrict__ out_bias) {
    extern __shared__ __attribute__((aligned(16))) char coarse_fin_smem[];
    constexpr int THREADS = 64 * kWideWaves;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool dots = BIAS && parts > 0;
    const int Dq = dots ? rerank_query_floats(D) : 0;
    float *qs = reinterpret_cast<float *>(coarse_fin_smem);
    for (int e = tid; e < Dq; e += THREADS) qs[e] = e < D ? queries[(long)q * D + e] : 0.f;
    WideList<THREADS> list;
    list.init(coarse_fin_smem + Dq * 4, P, tid);             // (ends on a barrier: the query is staged)
    const long total = (long)parts * P, base = (long)q * total;
    float sc = 0.f;
    int b = -1;
    if (tid < total) {
        sc = part_score[base + tid];
        b = part_list[base + tid];
    }
    int parity = 0;
    for (long e0 = 0; e0 < total; e0 += THREADS) {
        if (e0 > 0) list.begin_round(parity ^ 1, tid);
        float sn = 0.f;
        int bn = -1;
        if (e0 + THREADS + tid < total) {
            sn = part_score[base + e0 + THREADS + tid];
            bn = part_list[base + e0 + THREADS + tid];
        }
        list.offer(sc, b, b >= 0 && b < L, lane);
        list.end_round(parity, wave, lane);
        sc = sn;
        b = bn;
        parity ^= 1;
    }
    __syncthreads();
    list.flush(tid);
    for (int e = tid; e < P; e += THREADS) {
        const int at = list.i[e];
        out_score[(long)q * P + e] = list.s[e];
        out_list[(long)q * P + e] = at == kNoIndex ? -1 : at;
    }
    if constexpr (BIAS) {
        const int chunks = Dq / (256 * kRerankTrips);
        for (int g = wave; g * kRerankGroup < P; g += kWideWaves) {
            const int p = g * kRerankGroup + lane;
            int row = -1;
            if (lane < kRerankGroup && p < P && list.i[p] != kNoIndex) row = list.i[p];
            float ip = 0.f;                                  // -<q, c>: the inner-product score of rule 29
            if (dots) ip = vec ? rerank_group<false, kMetricIP, true>(qs, centroids, D, chunks, row, lane)
                               : rerank_group<false, kMetricIP, false>(qs, centroids, D, chunks, row, lane);
            if (lane < kRerankGroup && p < P) out_bias[(long)q * P + p] = row >= 0 ? 2.f * ip : 0.f;
        }
    }
}

// one wave per centroid: the sum of squares in rule 29's order
template <int METRIC>
__global__ void __launch_bounds__(64 * kCoarseWaves)
k_coarse_terms(const float *__restrict__ centroids, int L, int D, float *__restrict__ terms) {
    const int lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * kCoarseWaves + (threadIdx.x >> 6);
    if (c >= L) return;
    const float *row = centroids + c * D;
    float acc = 0.f;
    for (int e = lane * 4; e < D; e += 256)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < D) {
                const float x = row[e + j];
                acc = acc + x * x;
            }
    acc = rerank_butterfly(acc);
    if (lane == 0) terms[c] = METRIC == kMetricL2 ? 0.5f * acc : rnorm_of(acc);
}

}  // namespace mcq
