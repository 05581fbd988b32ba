// mcq_coarse_half_kernels.h -- gfx950 kernels of the coarse probes for fp16 queries (include/mcq_coarse_half.h, rules 52-55):
// score every fp16 query against every coarse centroid on the f16 matrix cores and keep the P best per query, exactly.  The
// product is rule 49's (the two fp16 planes of k_half_split, v_mfma_f32_32x32x16_f16, two fp32 accumulators a pair) and its
// staging is that of k_kmeans_assign_half (half_load, half_keep, the pitch of 40 halves, chunks of 32 halves double-buffered);
// the order (pair_less), the sort's network (coarse_sort's, here over several lists at once), the merge of the parts (WideList)
// and the winners' bias (rerank_group) are those of mcq_coarse_kernels.h.  Nothing of those files is changed.
//
// k_coarse_probe_half<METRIC, VEC, M>: one workgroup of 2 waves per (tile of 64 queries, part of the centroid tiles of 64).  A
// query is owned by ONE wave: wave w holds queries 32 w .. 32 w + 31 of the tile against all 64 centroids, as 2 blocks of 32 x
// 32 with two accumulators each (A_hi, A_lo): 64 registers.  The CENTROIDS are the A operand, as in k_kmeans_assign_half: lane l
// supplies 8 halves of row l % 32 at k = 8 (l / 32) and receives, in register r of block ci, the dot of query l % 32 with
// centroid 32 ci + 8 (r / 4) + 4 (l / 32) + r % 4.  So a lane holds ONE query and 16 centroids of each block, the two lanes of a
// query sit in the same wave, and the query's bound is a register pair that every score meets before anything touches LDS.  A
// step reads five 16-byte fragments (1 query, 2 hi, 2 lo) and issues four MFMAs.
// Thread t stages halves [8 (t % 4), 8 (t % 4) + 8) of rows t / 4 + 32 j, j < 2, of the queries, the hi rows and the lo rows:
// six 16-byte registers.  The tile's terms sit in LDS by tile parity, as in k_kmeans_assign_half.
//
// Selection: a list per query in LDS, M entries: [0, P) the P best so far, ascending under pair_less, behind them the pending
// entries.  The list is wave-private, so its counter is an LDS integer that only the two lanes of the query add to (the only
// atomics), and no workgroup barrier stands in the epilogue.  The offers go block by block: before a block of 32 centroids the
// wave sorts (coarse_half_sort, one wave, coarse_wave_sync alone) every list of its queries that has fewer than 32 free entries
// left, all of them together, then every lane reloads its bound; a block appends at most 32 entries to a list, so a slot is
// always there, in ANY order of the scores -- also when every centroid beats the bound.  A list therefore needs P + 32 entries
// rounded up to the sort's power of two, and M is a class of P the host picks:
//     P <= 16: M = 64     lists 32 KiB, all 64,768 B: two workgroups per compute unit
//     P <= 64: M = 128    lists 64 KiB, all 97,536 B: one workgroup per compute unit
//     P <= 128: M = 256   lists 128 KiB, all 163,072 B: one workgroup per compute unit (160 KiB is 163,840)
// The classes end well short of M - 32: a list that is nearly all P has no room for pending entries and sorts at every block
// that brings one (measured with classes that ended at 32 and 96: 1,024 x 65,536 took 3.2 ms at P = 32 and 1.8 ms at P = 33,
// 15.4 ms at P = 96 and 4.1 ms at P = 97).
// With 2 KiB a query in the last class 64 queries are what a compute unit holds, and with that the tile is 64 queries in every
// class; the first class then runs two of them side by side.  pair_less is a strict total order over what a list holds (a NaN
// never passes a bound; a centroid is offered once), so the result does not depend on the order of arrival, on `parts`, or on
// where a sort falls.
//
// k_coarse_finish_half: k_coarse_finish for an fp16 query: one workgroup per query merges the parts through a WideList, writes
// the probes and scores and, with BIAS, recomputes <q, c> for the winners as rule 29's plain fp32 dot, the query widened exactly
// when it is staged.  A copy of that kernel with one line changed, because a flag on k_coarse_finish would rename its
// instantiations and a shared body would give them another instruction text.
#pragma once
#include "mcq_half_kernels.h"

namespace mcq {

// ---- launch arithmetic (mcq_coarse_half_parts of mcq_api.hip is the plan, and the caller may choose another)
constexpr int kChWaves = 2;                // waves per workgroup
constexpr int kChQT = 32 * kChWaves;       // queries of a tile: 32 per wave
constexpr int kChBlocks = 2;               // blocks of 32 centroids a wave holds
constexpr int kChCT = 32 * kChBlocks;      // centroid rows of a tile
constexpr int kChStageHalves = (kChQT + 2 * kChCT) * kHalfPitch;   // one buffer: the query rows, the hi rows, the lo rows
constexpr int kChTermsAt = 2 * kChStageHalves * 2;                 // behind the staging: the terms of two centroid tiles
constexpr int kChListsAt = kChTermsAt + 2 * kChCT * 4;             // behind them: the lists
// LDS: [2 staging buffers][terms 2 x 64][entries 64 x M of (score, list)][64 counters][64 bound scores][64 bound indexes]
__host__ __device__ constexpr int coarse_half_lds(int M) { return kChListsAt + kChQT * M * 8 + 3 * kChQT * 4; }
__host__ __device__ constexpr int coarse_half_list(int P) { return P <= 16 ? 64 : (P <= 64 ? 128 : 256); }
constexpr int kChTargetBlocks = 512;       // workgroups mcq_coarse_half_parts aims at where two fit a compute unit, half otherwise
static_assert((kChQT + 2 * kChCT) * (kHalfDC / 8) == 6 * 64 * kChWaves, "a thread stages two rows of each of the three operands");
static_assert(kChCT <= 64 * kChWaves, "a thread stages at most one term of a tile");
static_assert(coarse_half_list(16) >= 16 + 32 && coarse_half_list(64) >= 64 + 32 && coarse_half_list(kCoarseMaxP) >= kCoarseMaxP + 32,
              "a list takes a block of 32 behind its P entries");
static_assert(coarse_half_lds(64) * 2 <= 160 * 1024 && coarse_half_lds(256) <= 160 * 1024 && kChListsAt % 16 == 0, "the LDS budget");

// (one wave)  the lists of the wave's 32 queries, M entries (score, list) each, the P best in front and pending entries behind
// them: those whose bit is set in `need` are sorted TOGETHER, coarse_sort's bitonic network under pair_less over all M entries
// (what lies behind the pending entries is (+inf, kNoIndex), behind every candidate), then their pending parts are emptied and
// their bounds refreshed.  One list has M / 2 exchanges a stage, less than a wave where M = 64 and a latency-bound trickle at
// any M; K lists have K M / 2, and a stage costs one coarse_wave_sync however many lists it serves.  Where M = 256 a lane takes
// U = 4 exchanges at a time, the eight 8-byte reads issued before the first write (the pairs of a stage are disjoint); at the
// shorter lists that form measured slower than one at a time (1,024 x 65,536 x 512, P = 8: 1.05 against 0.81 ms; P = 64: 3.06
// against 2.75; P = 128: 3.81 against 4.08), so U is a function of M.  Lane k finds the k-th set bit of `need` once, and a work
// item fetches its list's through one shuffle that every lane executes.
template <int M>
__device__ __forceinline__ void coarse_half_sort(float2 *le, int *cnt, float *bound_s, int *bound_i, int P, unsigned need, int lane) {
    constexpr int PAIRS = M / 2, U = M >= 256 ? 4 : 1;
    const int K = __builtin_popcount(need);
    unsigned rest = need;
    for (int k = 0; k < (lane & 31); ++k) rest &= rest - 1;
    const int sel = rest != 0 ? __builtin_ctz(rest) : 0;     // lane k < K: the k-th list to sort
    const int total = K * PAIRS;
    coarse_wave_sync();
    for (int size = 2; size <= M; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t0 = 0; t0 < total; t0 += 64 * U) {
                float2 *pa[U], *pz[U], ea[U], ez[U];
                bool on[U], up[U];
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const int t = t0 + 64 * j + lane;
                    on[j] = t < total;
                    const int q = __shfl(sel, on[j] ? t / PAIRS : 0, 64), u = t % PAIRS;
                    const int a = ((u & ~(stride - 1)) << 1) | (u & (stride - 1));
                    up[j] = (a & size) == 0;
                    pa[j] = le + q * M + a;
                    pz[j] = pa[j] + stride;
                    ea[j] = ez[j] = make_float2(0.f, 0.f);
                    if (on[j]) {
                        ea[j] = *pa[j];
                        ez[j] = *pz[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < U; ++j)
                    if (on[j] && pair_less(ez[j].x, __float_as_int(ez[j].y), ea[j].x, __float_as_int(ea[j].y)) == up[j]) {
                        *pa[j] = ez[j];
                        *pz[j] = ea[j];
                    }
            }
            coarse_wave_sync();
        }
    }
    if (lane < K) {
        const float2 last = le[sel * M + P - 1];
        cnt[sel] = 0;
        bound_s[sel] = last.x;
        bound_i[sel] = __float_as_int(last.y);
    }
    for (int t0 = 0; t0 < K * M; t0 += 64) {
        const int t = t0 + lane;                             // (K M is a multiple of 64: every lane has an entry)
        const int q = __shfl(sel, t / M, 64), e = t % M;
        if (e >= P) le[q * M + e] = make_float2(__builtin_inff(), __int_as_float(kNoIndex));
    }
    coarse_wave_sync();
}

// planes: what k_half_split wrote for the centroids.  terms: as k_coarse_scores takes them (NULL under the inner product).
// part s of query q leaves as P entries, ascending, at part_score / part_list [(q * parts + s) * P]; the tail is (+inf, -1)
template <int METRIC, bool VEC, int M>
__global__ void __launch_bounds__(64 * kChWaves)
k_coarse_probe_half(const unsigned short *__restrict__ queries, int Q, const unsigned short *__restrict__ planes, int L, int D,
                    const float *__restrict__ terms, int P, int parts, float *__restrict__ part_score,
                    int *__restrict__ part_list) {
    extern __shared__ __attribute__((aligned(16))) char coarse_half_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x / parts, part = blockIdx.x % parts;
    const long q0 = (long)qt * kChQT;
    const long T = ((long)L + kChCT - 1) / kChCT;
    const long lo = T * part / parts, hi = T * (part + 1) / parts;
    const int Dp = half_padded_dim(D), chunks = Dp / kHalfDC;
    const unsigned short *lo_plane = planes + (long)L * Dp;

    unsigned short *stage = reinterpret_cast<unsigned short *>(coarse_half_smem);
    float *tt = reinterpret_cast<float *>(coarse_half_smem + kChTermsAt);
    float2 *le = reinterpret_cast<float2 *>(coarse_half_smem + kChListsAt);      // an entry: (score, the list's bits)
    int *cnt = reinterpret_cast<int *>(le + kChQT * M);
    float *bound_s = reinterpret_cast<float *>(cnt + kChQT);
    int *bound_i = reinterpret_cast<int *>(bound_s + kChQT);
    const int srow = tid >> 2, scol = (tid & 3) * 8;         // staging: this thread's first row and first half of a chunk
    const int frow = lane & 31, half = lane >> 5;            // fragments: this lane's row and k group of a step
    const int qi = 32 * wave + frow;                         // this lane's query of the tile: its wave owns it
    const bool qthere = q0 + qi < Q;
    // the lists of this wave's queries: wave-private from here on, so no barrier stands between this and their first use
    for (int e = lane; e < 32 * M; e += 64) le[32 * wave * M + e] = make_float2(__builtin_inff(), __int_as_float(kNoIndex));
    if (lane < 32) {
        cnt[qi] = 0;
        bound_s[qi] = __builtin_inff();
        bound_i[qi] = kNoIndex;
    }
    float bs = __builtin_inff();                             // the bound of query qi: what LDS held after the last sort
    int bi = kNoIndex;

    const unsigned short *qtile = queries + q0 * D;
    const int qleft = (int)(Q - q0);
    uint4 rq[2], rh[2], rl[2];
    bool okq[2], okc[2];
    auto load = [&](long tile, int c) {
        const int e = c * kHalfDC + scol;
        const long coff = tile * kChCT * Dp;
        const int cleft = (int)(L - tile * kChCT);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            rq[j] = half_load<VEC>(qtile, srow + 32 * j, qleft, D, e, okq[j]);
            rh[j] = half_load<true>(planes + coff, srow + 32 * j, cleft, Dp, e, okc[j]);     // (e < Dp: a padded row is wholly there)
            rl[j] = half_load<true>(lo_plane + coff, srow + 32 * j, cleft, Dp, e, okc[j]);
        }
    };
    auto store = [&](int buf) {
        unsigned short *b = stage + buf * kChStageHalves + srow * kHalfPitch + scol;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            *reinterpret_cast<uint4 *>(b + 32 * j * kHalfPitch) = half_keep(okq[j], rq[j]);
            *reinterpret_cast<uint4 *>(b + (kChQT + 32 * j) * kHalfPitch) = half_keep(okc[j], rh[j]);
            *reinterpret_cast<uint4 *>(b + (kChQT + kChCT + 32 * j) * kHalfPitch) = half_keep(okc[j], rl[j]);
        }
    };
    // (one wave)  every list of this wave's queries that has more than `room` pending entries: sorted, and the bounds reloaded
    auto settle = [&](int room) {
        coarse_wave_sync();                                  // (the appends of this wave are in LDS)
        const unsigned need = (unsigned)__ballot(cnt[qi] > room);     // (the two lanes of a query agree: the low 32 bits say it all)
        if (need == 0) return;
        coarse_half_sort<M>(le + 32 * wave * M, cnt + 32 * wave, bound_s + 32 * wave, bound_i + 32 * wave, P, need, lane);
        bs = bound_s[qi];
        bi = bound_i[qi];
    };

    for (long tile = lo; tile < hi; ++tile) {
        // the tile's terms.  Buffer tile % 2: a wave that is still in the epilogue of the tile before reads the other one, and
        // the readers of this one passed a barrier since
        float *tw = tt + (tile & 1) * kChCT;
        if constexpr (METRIC != kMetricIP) {
            if (tid < kChCT) {
                const long cl = tile * kChCT + tid;
                tw[tid] = terms[cl < L ? cl : L - 1];
            }
        }
        load(tile, 0);
        store(0);
        __syncthreads();
        coarse_f32x16 ah[kChBlocks], al[kChBlocks];
#pragma unroll
        for (int ci = 0; ci < kChBlocks; ++ci)
#pragma unroll
            for (int r = 0; r < 16; ++r) ah[ci][r] = al[ci][r] = 0.f;
        for (int c = 0; c < chunks; ++c) {
            if (c + 1 < chunks) load(tile, c + 1);
            const unsigned short *b = stage + (c & 1) * kChStageHalves + 8 * half;
            const unsigned short *qa = b + qi * kHalfPitch;
            const unsigned short *ha = b + (kChQT + frow) * kHalfPitch;
            const unsigned short *la = ha + kChCT * kHalfPitch;
#pragma unroll
            for (int s = 0; s < kHalfDC / 16; ++s) {
                half_f16x8 yh[kChBlocks], yl[kChBlocks];
                const half_f16x8 x = *reinterpret_cast<const half_f16x8 *>(qa + 16 * s);
#pragma unroll
                for (int ci = 0; ci < kChBlocks; ++ci) {
                    yh[ci] = *reinterpret_cast<const half_f16x8 *>(ha + 32 * ci * kHalfPitch + 16 * s);
                    yl[ci] = *reinterpret_cast<const half_f16x8 *>(la + 32 * ci * kHalfPitch + 16 * s);
                }
#pragma unroll
                for (int ci = 0; ci < kChBlocks; ++ci)       // step 2 c + s of the blocks: into A_hi, then into A_lo
                    ah[ci] = __builtin_amdgcn_mfma_f32_32x32x16_f16(yh[ci], x, ah[ci], 0, 0, 0);
#pragma unroll
                for (int ci = 0; ci < kChBlocks; ++ci)
                    al[ci] = __builtin_amdgcn_mfma_f32_32x32x16_f16(yl[ci], x, al[ci], 0, 0, 0);
            }
            if (c + 1 < chunks) store((c + 1) & 1);
            __syncthreads();
        }
        // the offers of this lane's query, a block of 32 centroids at a time
        const int first = (int)(tile * kChCT), left = L - first;
#pragma unroll
        for (int ci = 0; ci < kChBlocks; ++ci) {
            settle(M - P - 32);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c0 = 32 * ci + 8 * (r / 4) + 4 * half + (r % 4);
                const float low = al[ci][r] * (1.f / kHalfLoScale);
                const float dot = ah[ci][r] + low;
                float sc;
                if constexpr (METRIC == kMetricL2) sc = tw[c0] - dot;
                else if constexpr (METRIC == kMetricIP) sc = -dot;
                else sc = -(dot * tw[c0]);
                if (qthere && c0 < left && pair_less(sc, first + c0, bs, bi)) {
                    const int slot = P + atomicAdd(&cnt[qi], 1);
                    // (a block appends at most 32: the check is defence alone)
                    if (slot < M) le[qi * M + slot] = make_float2(sc, __int_as_float(first + c0));
                }
            }
        }
    }
    settle(0);
    coarse_wave_sync();
    for (int e = lane; e < 32 * P; e += 64) {
        const int at = 32 * wave + e / P, p = e % P;
        if (q0 + at < Q) {
            const long out = ((q0 + at) * parts + part) * P + p;
            const float2 entry = le[at * M + p];
            const int l = __float_as_int(entry.y);
            part_score[out] = entry.x;
            part_list[out] = l == kNoIndex ? -1 : l;
        }
    }
}

// parts == 0: no centroid at all (L == 0): the tail alone, and no input is read.  k_coarse_finish, the query fp16
template <bool BIAS>
__global__ void __launch_bounds__(64 * kWideWaves)
k_coarse_finish_half(const float *__restrict__ part_score, const int *__restrict__ part_list, int parts, int P,
                     const unsigned short *__restrict__ queries, const float *__restrict__ centroids, int L, int D, int vec,
                     int *__restrict__ out_list, float *__restrict__ out_score, float *__restrict__ out_bias) {
    extern __shared__ __attribute__((aligned(16))) char coarse_half_fin_smem[];
    constexpr int THREADS = 64 * kWideWaves;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool dots = BIAS && parts > 0;
    const int Dq = dots ? rerank_query_floats(D) : 0;
    float *qs = reinterpret_cast<float *>(coarse_half_fin_smem);
    for (int e = tid; e < Dq; e += THREADS) qs[e] = e < D ? rerank_widen<true>(queries, (long)q * D + e) : 0.f;
    WideList<THREADS> list;
    list.init(coarse_half_fin_smem + Dq * 4, P, tid);        // (ends on a barrier: the query is staged)
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

}  // namespace mcq
