// mcq_shortlist_kernels.h -- gfx950 kernel of the search over a shortlist (include/mcq_shortlist.h, rules 36-39): score the
// candidates a per-query shortlist names against the stored CODES and keep the k best.  The score is tile_step + score_finish
// of mcq_search_kernels.h, the result list, its order and the merge of the parts are those of mcq_wide_kernels.h (WideList,
// pair_less, k_search_wide_merge), and what a shortlist entry names is rerank_entry's rule of mcq_rerank_kernels.h; nothing
// of those files is changed.  What is new is the step space: a step is 64 consecutive entries of a shortlist row, one per
// lane, and the lane's candidate is whatever row of the store its entry names.
//
// One workgroup per (query, part of its shortlist row), kWideWaves waves; the query's table sits in LDS (tile_stage<1, ..>),
// the wide list behind it.  The parts are cut by step count and the waves of a workgroup take a part's steps in turn, in
// rounds of one barrier, exactly as k_search_wide does.
//
// The dependent loads.  entry -> row_of -> digits / w is a chain of three loads, and tile_step wants the NEXT step's row as
// bnext so that its digits and w travel one step ahead.  The chain is cut into its links, one step apart: in the iteration
// of step s a wave issues the load of the raw entries of step s + 3 rounds, the row_of load of step s + 2 rounds (its
// entries arrived an iteration ago), and -- inside tile_step -- the digits and w of step s + 1 round (its rows arrived an
// iteration ago).  No load waits for another load of the same iteration.  The bias hangs on the SLOT, not on the entry, so
// it is no link of the chain: it is read one step ahead like w.  (kShortAhead 0 resolves the next step's entries in the step
// itself; DESIGN.md section 5 has what either measured.)
//
// The bounds (rule 36): a slot is checked against S before the shortlist is read, an entry against [0, Bs) before row_of is
// read and a row against [0, B) before it is used; a lane without a candidate holds row 0, which exists (B > 0 in every call
// that launches), re-reads its digits and w, and offers nothing.  A digit is masked with K - 1 by CodeChunk.
#pragma once
#include "mcq_wide_kernels.h"

namespace mcq {

// ---- launch arithmetic (tests/search_shortlist_grid.py reads these constants from this file and mirrors short_plan of
// mcq_api.hip)
constexpr int kShortStep = 64;             // shortlist entries per step: one per lane
constexpr int kShortTargetBlocks = 1024;   // workgroups that fill the chip once (4 per CU, 16 waves per CU)
#ifndef MCQ_SHORT_AHEAD
#define MCQ_SHORT_AHEAD 1
#endif
constexpr int kShortAhead = MCQ_SHORT_AHEAD;   // 1: the links of the chain one step apart; 0: a step resolves its successor

// LDS: [the table, N*K floats][the wide list]
__host__ __device__ constexpr int short_lds_table(int NK) { return (NK * 4 + 15) & ~15; }
__host__ __device__ constexpr int short_lds_bytes(int NK, int k) { return short_lds_table(NK) + wide_list_bytes(k); }

// the raw entry of this lane in `step` of the row; -1 (names nothing) past the part or the row
__device__ __forceinline__ int64_t short_raw(const int64_t *__restrict__ srow, int S, long long step, long long hi, int lane) {
    const long long c = step * kShortStep + lane;
    return (step < hi && c < S) ? srow[c] : (int64_t)-1;
}

// an entry -> (position, row), or (kNoIndex, 0) where it names no candidate (rule 36: rerank_entry's rule)
__device__ __forceinline__ void short_resolve(int64_t p, const int64_t *__restrict__ row_of, long Bs, long B, int &pos, int &row) {
    pos = kNoIndex;
    row = 0;
    if (p >= 0 && p < Bs) {
        const int64_t r = row_of ? row_of[p] : p;
        if (r >= 0 && r < B) {
            pos = (int)p;                                    // (Bs < 2^31 - 1: never kNoIndex)
            row = (int)r;
        }
    }
}

// the bias of this lane's slot in `step` (-0.0 without a bias, and past the part or the row: S + -0.0 has the bits of S)
__device__ __forceinline__ float short_bias(const float *__restrict__ brow, int S, long long step, long long hi, int lane) {
    const long long c = step * kShortStep + lane;
    return (brow && step < hi && c < S) ? brow[c] : -0.f;
}

// bias == NULL: no bias; it is no template parameter, as in k_search_wide.  T: the digit type of the store (CodeChunk).
template <int N, int M, typename T>
__global__ void __launch_bounds__(64 * kWideWaves)
k_search_short(const float *__restrict__ tables, int Q, const T *__restrict__ codes, const float *__restrict__ w, long B, int K,
               int k, int parts, const int64_t *__restrict__ shortlist, int S, const int64_t *__restrict__ row_of, long Bs,
               const float *__restrict__ bias, float *__restrict__ ws_s, int *__restrict__ ws_i) {
    extern __shared__ __attribute__((aligned(16))) char search_smem[];
    constexpr int CH = N < 8 ? N : 8;
    constexpr int THREADS = 64 * kWideWaves;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / parts, part = blockIdx.x % parts;
    const long long steps = ((long long)S + kShortStep - 1) / kShortStep;
    const long long lo = steps * part / parts, hi = steps * (part + 1) / parts;
    const long out = ((long)q * parts + part) * k;
    if (lo >= hi) {                                          // no step: the empty list, and nothing is staged
        for (int e = tid; e < k; e += THREADS) {
            ws_s[out + e] = __builtin_inff();
            ws_i[out + e] = kNoIndex;
        }
        return;
    }
    tile_stage<1, THREADS>(reinterpret_cast<float *>(search_smem), tables, Q, q, N * K, tid);
    const float *Tl = reinterpret_cast<const float *>(search_smem);
    WideList<THREADS> list;
    list.init(search_smem + short_lds_table(N * K), k, tid);

    const int64_t *srow = shortlist + (long)q * S;
    const float *brow = bias ? bias + (long)q * S : nullptr;
    long long step = lo + wave;
    // the wave's first steps, link by link: (pos, row) of `step`, (pos1, row1) of the step after it, the raw entries p2 of
    // the one after that
    int pos, row, pos1, row1;
    short_resolve(short_raw(srow, S, step, hi, lane), row_of, Bs, B, pos, row);
    short_resolve(short_raw(srow, S, step + kWideWaves, hi, lane), row_of, Bs, B, pos1, row1);
    int64_t p2 = kShortAhead ? short_raw(srow, S, step + 2 * kWideWaves, hi, lane) : (int64_t)-1;
    CodeChunk<CH, T> cur;
    float t = 0.f;
    if (step < hi) {
        cur.load(codes + (long)row * N);
        if (M != kMetricIP) t = w[row];
    } else {
        cur.clear();
    }
    float bv = short_bias(brow, S, step, hi, lane);
    int parity = 0;
    for (long long first = lo; first < hi; first += kWideWaves) {
        if (first > lo) list.begin_round(parity ^ 1, tid);
        if (step < hi) {
            const long long nstep = step + kWideWaves;
            int pos2 = kNoIndex, row2 = 0;
            int64_t p3 = -1;
            if constexpr (kShortAhead != 0) {
                p3 = short_raw(srow, S, nstep + 2 * kWideWaves, hi, lane);               // three rounds ahead: the entries
                short_resolve(p2, row_of, Bs, B, pos2, row2);                            // two rounds ahead: their rows
            } else {
                short_resolve(short_raw(srow, S, nstep, hi, lane), row_of, Bs, B, pos1, row1);   // the whole chain, now
            }
            const float bv_next = short_bias(brow, S, nstep, hi, lane);
            float tn = t;
            float acc[1];
            tile_step<1, CH, N>(acc, cur, tn, Tl, codes, w, M, N, K, (long)row, (long)row1);   // one round ahead: digits and w
            list.offer(score_finish(acc[0] + bv, t, M), pos, pos != kNoIndex, lane);
            t = tn;
            bv = bv_next;
            pos = pos1;
            row = row1;
            if constexpr (kShortAhead != 0) {
                pos1 = pos2;
                row1 = row2;
                p2 = p3;
            }
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

}  // namespace mcq
