// mcq_wide_kernels.h -- gfx950 kernels of the top-k search past 64 neighbours (include/mcq_wide.h, rules 24-27): result
// lists of up to 1,024 entries per query.  Scores, candidates and the order are those of mcq_search_kernels.h -- tile_step +
// score_finish, the step space of k_search_lists, pair_less -- and nothing of that file is changed; what is new is a result
// list wider than a wave and the merge that goes with it.
//
// The wide list (WideList) belongs to a WORKGROUP and lives in LDS behind the tables and the step space, M = 1,024 entries
// for k <= 512 and 2,048 beyond:
//     [0, k)   the k smallest entries seen so far, ascending under pair_less
//     [k, M)   the pending entries: candidates below the bound, in the order they happened to arrive
// The bound is the entry of rank k - 1, the same value in every thread.  A wave offers its 64 scores of a step: those below
// the bound are compacted by ballot and prefix count behind an LDS INTEGER counter (the only atomic of the feature).  The
// waves of a workgroup go in rounds of one step each; at the start of a round every thread adds up what the waves published
// in the round before, and when the pending entries cannot take one more round the workgroup flushes: one bitonic sort of
// all M entries under pair_less, after which [0, k) is again the smallest, the rest is emptied and the bound refreshed.
// pair_less is a strict total order over what the list holds (a NaN never passes the bound, a position is unique among a
// query's candidates, an empty entry is (+inf, kNoIndex), behind every candidate), so the result is a function of scores
// and positions alone, whatever the order of arrival.  A list in LDS rather than in registers costs no template axis (k is
// a runtime value: 42 instantiations) and no registers; at the largest shape, 64 x 256 tables and 4,096 probes, the kernel
// takes 128 KiB + 16 B + 16 KiB + 64 B = 147,536 B of the CU's 160 KiB.
#pragma once
#include "mcq_search_kernels.h"

namespace mcq {

// ---- launch arithmetic (tests/search_wide_grid.py reads these constants from this file and mirrors wide_plan of mcq_api.hip)
constexpr int kWideWaves = 4;             // k_search_wide and k_search_wide_merge: waves per workgroup (256 threads)
constexpr int kWideMaxK = 1024;           // the largest k
constexpr int kWideMergeEntries = 65536;  // wide_plan: entries of half a list times parts of a query, at most

// half the entries of the wide list
__host__ __device__ constexpr int wide_half(int k) { return k <= 512 ? 512 : 1024; }
// LDS: [k_search_lists' regions for (NK, P)][scores: float 2 half][positions: int 2 half][counter; the waves' counts, twice]
__host__ __device__ constexpr int wide_lds_list(int NK, int P) { return (lists_lds_bytes(NK, P) + 15) & ~15; }
__host__ __device__ constexpr int wide_list_bytes(int k) { return 2 * wide_half(k) * 8 + 64; }
__host__ __device__ constexpr int wide_lds_bytes(int NK, int P, int k) { return wide_lds_list(NK, P) + wide_list_bytes(k); }

template <int THREADS>
struct WideList {
    static constexpr int WAVES = THREADS / 64;
    static_assert(2 * WAVES + 1 <= 16, "the counter and the waves' counts fill the 64 bytes behind the entries");
    float *s;
    int *i;
    int *cnt;                                                // entries appended since the last flush (atomic)
    int *seen;                                               // seen[parity][wave]: what a wave had appended by the end of a round
    int M, k;
    int mine;                                                // entries this wave appended since the last flush (wave-uniform)
    float ts;                                                // the bound: the entry of rank k - 1 (the same in every thread)
    int tb;

    // (every thread of the workgroup; ends on a barrier)
    __device__ __forceinline__ void init(char *at, int k_, int tid) {
        k = k_;
        M = 2 * wide_half(k_);
        s = reinterpret_cast<float *>(at);
        i = reinterpret_cast<int *>(at) + M;
        cnt = i + M;
        seen = cnt + 1;
        for (int e = tid; e < M; e += THREADS) {
            s[e] = __builtin_inff();
            i[e] = kNoIndex;
        }
        if (tid < 2 * WAVES + 1) cnt[tid] = 0;
        mine = 0;
        ts = __builtin_inff();
        tb = kNoIndex;
        __syncthreads();
    }

    // a wave offers one candidate per lane (a NaN score compares false and is never taken).  begin_round() keeps room for a
    // round of THREADS offers, so a slot lies below M; the test is defence alone.
    __device__ __forceinline__ void offer(float sc, int b, bool cand, int lane) {
        const bool in = cand && pair_less(sc, b, ts, tb);
        const u64 m = __ballot(in);
        if (m == 0) return;
        int base = 0;
        if (lane == 0) base = atomicAdd(cnt, __popcll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        mine += __popcll(m);
        const int slot = k + base + mbcnt64(m);
        if (in && slot < M) {
            s[slot] = sc;
            i[slot] = b;
        }
    }

    // (every wave, once per round, after its offer or in place of it)  what it has appended, for the next round to read.
    // Two copies by the round's parity: a wave that is already in round r + 1 writes the other copy than the one a slower
    // wave still reads at the start of round r + 1.
    __device__ __forceinline__ void end_round(int parity, int wave, int lane) {
        if (lane == 0) seen[parity * WAVES + wave] = mine;
    }

    // (every thread, at the start of every round but a list's first; `parity` is that of the round before)  one barrier,
    // then the same sum in every thread: a flush when the pending entries cannot take another round
    __device__ __forceinline__ void begin_round(int parity, int tid) {
        __syncthreads();
        int c = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) c += seen[parity * WAVES + v];
        if (c + THREADS > M - k) flush(tid);
    }

    // (every thread, behind a barrier that follows the last offer; ends on one)  all M entries sorted ascending by a
    // bitonic network whose only comparison is pair_less; the pending entries are emptied and the bound read again
    __device__ __forceinline__ void flush(int tid) {
        for (int size = 2; size <= M; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < M / 2; t += THREADS) {
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
                __syncthreads();
            }
        }
        ts = s[k - 1];
        tb = i[k - 1];
        for (int e = k + tid; e < M; e += THREADS) {
            s[e] = __builtin_inff();
            i[e] = kNoIndex;
        }
        if (tid == 0) *cnt = 0;
        mine = 0;
        __syncthreads();
    }
};

// ------------------------------------------------------------------- scoring
// k_search_lists with the wide list: one query per workgroup, part `part` of S of the query's steps, cut by COUNT; the waves
// take the part's steps in turn, codes and w one step ahead.  The waves of a workgroup go through the part in ROUNDS of
// kWideWaves steps, one barrier a round (a wave without a step in the last round offers nothing), because the flush is the
// workgroup's.
// probes == NULL: the whole store as ONE implicit list [0, B) (P is 1, list_offsets and L are not read).
// probe_bias == NULL: no bias.  The bias is no template parameter here: a call without one adds -0.0, and (S + -0.0) has the
// bits of S for every S.  It travels one step ahead as ListCursor's does: read at walk.p once peek() has moved that on.
// The part leaves as k entries, ascending, at list (q, part) of the workspace; an entry without a candidate is (+inf, kNoIndex).
// T: the digit type of the store (CodeChunk).  With uint16_t (include/mcq_code16.h) this kernel serves every k from 1: the
// narrow kernels have no two-byte twin.
template <int N, int M, bool MASKED, typename T = uint8_t>
__global__ void __launch_bounds__(64 * kWideWaves)
k_search_wide(const float *__restrict__ tables, int Q, const T *__restrict__ codes, const float *__restrict__ w,
              long B, int K, int k, int S, const int64_t *__restrict__ list_offsets, long L, const int *__restrict__ probes,
              int P, float *__restrict__ ws_s, int *__restrict__ ws_i, const u64 *__restrict__ mask,
              const float *__restrict__ probe_bias) {
    extern __shared__ __attribute__((aligned(16))) char search_smem[];
    constexpr int CH = N < 8 ? N : 8;
    constexpr int THREADS = 64 * kWideWaves;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / S, part = blockIdx.x % S;
    ListWalk walk;
    long long steps;
    if (probes) {
        steps = walk.build<THREADS>(search_smem, N * K, list_offsets, L, probes + (long)q * P, P, B, tid);
    } else {                                                 // the one list [0, B)
        steps = walk.whole(search_smem, N * K, B, tid);
    }
    const long long lo = steps * part / S, hi = steps * (part + 1) / S;           // (T <= 2^37, S <= 256)
    const long out = ((long)q * S + part) * k;
    if (lo >= hi) {                                          // no step: the empty list, and nothing is staged
        for (int e = tid; e < k; e += THREADS) {
            ws_s[out + e] = __builtin_inff();
            ws_i[out + e] = kNoIndex;
        }
        return;
    }
    tile_stage<1, THREADS>(reinterpret_cast<float *>(search_smem), tables, Q, q, N * K, tid);
    const float *Tl = reinterpret_cast<const float *>(search_smem);
    const float *brow = probe_bias ? probe_bias + (long)q * P : nullptr;
    WideList<THREADS> list;
    list.init(search_smem + wide_lds_list(N * K, P), k, tid);

    CodeChunk<CH, T> cur;
    float t = 0.f;
    ListCursor<MASKED, false> pos;
    long long step = lo + wave;
    pos.start(walk, step, hi, cur, t, codes, w, M, N, mask, nullptr, lane);
    float bias = -0.f, bias_next = -0.f;
    if (brow && step < hi) bias = brow[walk.p];              // (walk.p < P: seek() found the step's slot)
    int parity = 0;
    for (long long first = lo; first < hi; first += kWideWaves) {
        if (first > lo) list.begin_round(parity ^ 1, tid);
        if (step < hi) {
            const long long nstep = step + kWideWaves;
            pos.peek(walk, nstep, hi, mask, nullptr, lane);
            bias_next = bias;
            if (brow && nstep < hi) bias_next = brow[walk.p];            // (at() moved walk.p to the slot of nstep)
            float tn = t;
            float acc[1];
            tile_step<1, CH, N>(acc, cur, tn, Tl, codes, w, M, N, K, pos.b, pos.bnext);
            list.offer(score_finish(acc[0] + bias, t, M), (int)pos.b, pos.offer(), lane);
            t = tn;
            pos.advance();
            bias = bias_next;
            step = nstep;
        }
        list.end_round(parity, wave, lane);
        parity ^= 1;
    }
    __syncthreads();
    list.flush(tid);
    for (int e = tid; e < k; e += THREADS) {
        ws_s[out + e] = list.s[e];
        ws_i[out + e] = list.i[e];
    }
}

// -------------------------------------------------------------------- merge
// One workgroup per query: the S lists of its parts stream through the same wide list, a round of 256 entries at a time
// with the next round's loads in flight, and the final k leave under the same order.  An entry that holds no candidate
// leaves as (+inf, -1), k_search_merge's fill; S == 0 (no candidate anywhere) only writes that fill.
__global__ void __launch_bounds__(64 * kWideWaves)
k_search_wide_merge(const float *__restrict__ ws_s, const int *__restrict__ ws_i, int S, int k, float *__restrict__ out_s,
                    int64_t *__restrict__ out_i) {
    constexpr int THREADS = 64 * kWideWaves;
    __shared__ __attribute__((aligned(16))) char wide_smem[wide_list_bytes(kWideMaxK)];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const long total = (long)S * k, base = (long)q * total;
    WideList<THREADS> list;
    list.init(wide_smem, k, tid);
    float sc = 0.f;
    int b = kNoIndex;
    if (tid < total) {
        sc = ws_s[base + tid];
        b = ws_i[base + tid];
    }
    int parity = 0;
    for (long e0 = 0; e0 < total; e0 += THREADS) {
        if (e0 > 0) list.begin_round(parity ^ 1, tid);
        float sn = 0.f;
        int bn = kNoIndex;
        if (e0 + THREADS + tid < total) {
            sn = ws_s[base + e0 + THREADS + tid];
            bn = ws_i[base + e0 + THREADS + tid];
        }
        list.offer(sc, b, b != kNoIndex, lane);
        list.end_round(parity, tid >> 6, lane);
        sc = sn;
        b = bn;
        parity ^= 1;
    }
    __syncthreads();
    list.flush(tid);
    for (int e = tid; e < k; e += THREADS) {
        const int at = list.i[e];
        out_s[(long)q * k + e] = list.s[e];
        out_i[(long)q * k + e] = (at == kNoIndex) ? (int64_t)-1 : (int64_t)at;
    }
}

}  // namespace mcq
