// mcq_range_kernels.h -- gfx950 kernels of the RANGE search over stored codes: every stored vector whose score does not exceed
// a per-query threshold, in CSR form.  Same tables, same tiling and the same score as the top-k scan (mcq_search_kernels.h,
// rules 1, 2, 3, 3' and 6 of include/mcq.h), but no list: one comparison, one ballot and a rare store per candidate.
//
// Arithmetic contract (include/mcq.h, rules 7-9; tests/search_range_grid.py restates 7 and 8 in numpy):
//   7. b is listed for q iff score[q][b] <= thr[q]: one fp32 comparison, inclusive; a NaN on either side lists nothing.
//   8. lims int64[Q + 1], lims[0] = 0; the entries of q occupy [lims[q], lims[q+1]) in ascending position b, as (score, position).
//   9. Q == 0 or B == 0: lims is all zeros and nothing else is written.
// Two sweeps over the store are ONE kernel (k_range_sweep below, over the scan's own tile_step), so they cannot disagree
// about a borderline candidate: the COUNT sweep leaves one count per (query, slice, wave); k_range_offsets and k_range_lims
// turn the counts into lims and into one start offset per (query, slice, wave); the FILL sweep recomputes the scores and
// stores the hits.  A wave owns a CONTIGUOUS run of its slice's steps of 64 candidates, so ascending position is (slice,
// wave, step, lane) and the fill learns its offsets from the counts alone.  Integer sums only: the output is a function of
// scores and thresholds.
// Under a mask (rules 10-12; MASKED) a candidate is a hit iff its bit is set and its score passes, in COUNT and in FILL alike,
// and a wave skips the steps of its run whose word is zero (MaskWalk of mcq_search_kernels.h).  The run itself is unchanged, so
// the offsets are still a matter of the counts alone.
#pragma once
#include "mcq_search_kernels.h"

namespace mcq {

// ---- launch arithmetic (tests/search_range_grid.py reads these constants from this file and mirrors range_plan of mcq_api.hip;
// the tile, LDS and slice caps are kScanQTMax, kScanTableLds, kScanTargetBlocks and kScanMaxSlices of the top-k scan)
constexpr int kRangeWaves = 16;           // k_range_sweep: waves per workgroup (1024 threads).  The tables of a 16 x 8 x 256 tile
                                          // take 128 KiB, so ONE workgroup fits a CU: 16 waves are 4 per SIMD, and with no
                                          // list in registers the sweep stays far below the 128 VGPRs that allows

// QT queries per tile, digits in chunks of CH codebooks (N a multiple of CH), FILL: the second sweep.  The scores are those of
// tile_step and score_finish (mcq_search_kernels.h), the scan's own: a wave owns a contiguous run of steps (so its next
// step is blk + 1) and compares each score with thr[q].
// The metric is a wave-uniform runtime switch at the score's last operation (score_finish; the top-k scan makes it a template
// parameter because its lists sit at the register edge; nothing does here, and it keeps the number of instantiations down).
// ws: int64 [Q][S][kRangeWaves] -- counts out (COUNT), start offsets relative to lims[q] in (FILL).
template <int QT, int CH, bool FILL, bool MASKED>
__global__ void __launch_bounds__(64 * kRangeWaves)
k_range_sweep(const float *__restrict__ tables, int Q, const uint8_t *__restrict__ codes, const float *__restrict__ w, long B,
              int N, int K, int metric, int S, long per_slice, const float *__restrict__ thr, int64_t *__restrict__ ws,
              const int64_t *__restrict__ lims, float *__restrict__ out_s, int64_t *__restrict__ out_i, long capacity,
              const u64 *__restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) char range_smem[];
    float *Tl = reinterpret_cast<float *>(range_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x / S, slice = blockIdx.x % S;
    const int q0 = tile * QT, NK = N * K;
    tile_stage<QT, 64 * kRangeWaves>(Tl, tables, Q, q0, NK, tid);

    // FILL: the slot of this wave's first hit per query, lims[q] + the wave's start offset, waits in LDS behind the tables (it
    // is read only in a step that has a hit; 32 scalar registers of bases would push the 16 x 8 sweep into scratch)
    long *base_at = reinterpret_cast<long *>(range_smem + (size_t)NK * QT * 4) + wave * QT;
    if (FILL && lane < QT)
        base_at[lane] = (q0 + lane < Q) ? lims[q0 + lane] + ws[((long)(q0 + lane) * S + slice) * kRangeWaves + wave] : 0;
    float th[QT];                                            // (uniform) a query past the end of the tile lists nothing: NaN
    int cnt[QT];                                             // (uniform) this wave's hits so far, per query
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        th[q] = (q0 + q < Q) ? thr[q0 + q] : __builtin_nanf("");
        cnt[q] = 0;
    }

    const Slice sl = slice_of(slice, per_slice, B);
    const long run = (sl.steps + kRangeWaves - 1) / kRangeWaves;  // steps per wave: wave v owns [v * run, (v + 1) * run)
    const long first = (long)wave * run;
    const long stop = first + run < sl.steps ? first + run : sl.steps;
    const u64 below = (1ull << lane) - 1;
    CodeChunk<CH> cur;
    float t = 0.f;
    if constexpr (MASKED) {
        // the steps of the run that hold a candidate, in order; the next step is the next of THOSE.  A set bit lies inside the
        // slice (MaskWalk trims the last word), so "bit && valid" is the bit.  The loop without a mask, below, stays the text
        // it was: with the comparison moved into a helper both loops share, hipcc compiles the unmasked sweeps differently.
        MaskWalk walk(mask, sl, first, stop, 1);
        u64 word = 0, word_next = 0;
        int blk = walk.next(word, lane);
        tile_first(cur, t, codes, w, metric, N, sl, blk < 0 ? stop : blk, stop, lane);
        while (blk >= 0) {
            const int nblk = walk.next(word_next, lane);
            float tn = t;
            float acc[QT];
            tile_step(acc, cur, tn, Tl, codes, w, metric, N, K, step_at(sl, blk, lane), step_at(sl, nblk < 0 ? blk : nblk, lane));
            const long bl = sl.begin + (long)blk * 64 + lane;
            const bool bit = (word >> lane) & 1;
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                const float s = score_finish(acc[q], t, metric);
                const bool hit = bit && s <= th[q];              // rules 7 and 11 (a NaN compares false)
                const u64 m = __ballot(hit);
                if constexpr (FILL) {
                    if (m) {                                     // (uniform) hits are rare
                        const long slot = base_at[q] + cnt[q] + __builtin_popcountll(m & below);
                        if (hit && (unsigned long)slot < (unsigned long)capacity) {
                            out_s[slot] = s;
                            out_i[slot] = bl;
                        }
                    }
                }
                cnt[q] += __builtin_popcountll(m);
            }
            t = tn;
            blk = nblk;
            word = word_next;
        }
    } else {
        tile_first(cur, t, codes, w, metric, N, sl, first, stop, lane);
        for (long blk = first; blk < stop; ++blk) {
            const long bl = sl.begin + blk * 64 + lane;
            const long bnext = blk + 1 < stop ? step_at(sl, blk + 1, lane) : step_at(sl, blk, lane);
            float tn = t;
            float acc[QT];
            tile_step(acc, cur, tn, Tl, codes, w, metric, N, K, step_at(sl, blk, lane), bnext);
            const bool valid = bl < sl.end;
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                const float s = score_finish(acc[q], t, metric);
                const bool hit = valid && s <= th[q];            // rule 7 (a NaN compares false)
                const u64 m = __ballot(hit);
                if constexpr (FILL) {
                    if (m) {                                     // (uniform) hits are rare
                        const long slot = base_at[q] + cnt[q] + __builtin_popcountll(m & below);
                        if (hit && (unsigned long)slot < (unsigned long)capacity) {
                            out_s[slot] = s;
                            out_i[slot] = bl;
                        }
                    }
                }
                cnt[q] += __builtin_popcountll(m);
            }
            t = tn;
        }
    }

    if constexpr (!FILL) {
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < QT; ++q)
                if (q0 + q < Q) ws[((long)(q0 + q) * S + slice) * kRangeWaves + wave] = cnt[q];
        }
    }
}

// ---------------------------------------------------------------- the range search list by list (rules 17-20 of include/mcq.h)
// The sweep's hit logic over the step space of k_search_lists: a workgroup is ONE query and part s of S of the steps of ITS
// probes.  The step space, its cut into parts, ListWalk and ListCursor are described once, in mcq_search_kernels.h ("lists");
// what differs here:
//   * a wave owns a CONTIGUOUS run of its part's steps, run = ceil((hi - lo) / W), wave v the steps [lo + v*run, min(lo +
//     (v+1)*run, hi)): the rule of k_range_sweep, not the interleaving of k_search_lists.  So (part, wave, step, lane)
//     ascending IS the flattened step space -- the probe row's own order, ascending position within a list -- and the fill
//     learns its slots from the counts alone, as in the sweep.
//   * the score is tile_step<1, CH> + score_finish with the metric a wave-uniform runtime switch, the comparison, the ballot
//     and the slot are k_range_sweep's.  One query per workgroup: the wave's base slot is one value in a register.
//   * COUNT writes one int64 per (query, part, wave), zeros included (nobody clears the workspace): a part without a step
//     writes its zeros and returns before it stages the table.  k_range_offsets (per = S * kRangeListWaves) and k_range_lims
//     finish the count unchanged.  No atomics of any kind.
//   * with a bias (BIAS; rules 21-23): s = score_finish(S + the bias of the step's slot, w), the bias travelling with the
//     cursor as in k_search_lists; the same step space, runs, counts and slots.
//   * T: the digit type of the store (CodeChunk).  With uint16_t (include/mcq_code16.h) probes == NULL is the whole store as
//     ONE implicit list [0, B) (P is 1, list_offsets and L are not read), as in k_search_wide: parts and runs ascend with
//     the position, so the hits of a query leave in ascending position and two-byte codes need no sweep of their own.  The
//     one-byte instantiations have k_range_sweep for that and do not test the pointer: they are the code they were.
// LDS: lists_lds_bytes of mcq_search_kernels.h.
constexpr int kRangeListWaves = 4;        // k_range_lists: waves per workgroup (256 threads), as kListWaves: a table is N*K
                                          // floats (8 KiB at 8 x 256), so several workgroups share a CU and 4 waves each keep
                                          // 4 per SIMD at 4 workgroups per CU (not measured against 8 or 16)

// ws: int64 [Q][S][kRangeListWaves] -- counts out (COUNT), start offsets relative to lims[q] in (FILL).
template <int CH, bool FILL, bool MASKED, bool BIAS, typename T = uint8_t>
__global__ void __launch_bounds__(64 * kRangeListWaves)
k_range_lists(const float *__restrict__ tables, const T *__restrict__ codes, const float *__restrict__ w, long B,
              int N, int K, int metric, int S, const int64_t *__restrict__ list_offsets, long L, const int *__restrict__ probes,
              int P, const float *__restrict__ thr, int64_t *__restrict__ ws, const int64_t *__restrict__ lims,
              float *__restrict__ out_s, int64_t *__restrict__ out_i, long capacity, const u64 *__restrict__ mask,
              const float *__restrict__ probe_bias) {
    extern __shared__ __attribute__((aligned(16))) char range_smem[];
    constexpr int THREADS = 64 * kRangeListWaves;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / S, part = blockIdx.x % S;
    const int NK = N * K;
    ListWalk walk;
    long long steps;
    if (sizeof(T) > 1 && !probes) {
        steps = walk.whole(range_smem, NK, B, tid);
    } else {
        steps = walk.build<THREADS>(range_smem, NK, list_offsets, L, probes + (long)q * P, P, B, tid);
    }
    const long long lo = steps * part / S, hi = steps * (part + 1) / S;   // (steps <= 2^37, S <= 256)
    int64_t *mine = ws + ((long)q * S + part) * kRangeListWaves;           // this part's kRangeListWaves entries
    if (lo >= hi) {                                          // no step: zeros (COUNT), and nothing is staged
        if (!FILL && tid < kRangeListWaves) mine[tid] = 0;
        return;
    }
    float *Tl = reinterpret_cast<float *>(range_smem);
    tile_stage<1, THREADS>(Tl, tables, q + 1, q, NK, tid);                // (q < Q by the grid)
    const float *brow = BIAS ? probe_bias + (long)q * P : nullptr;

    const long long run = (hi - lo + kRangeListWaves - 1) / kRangeListWaves;   // steps per wave: wave v owns [lo + v*run, ..)
    long long step = lo + wave * run;
    const long long stop = step + run < hi ? step + run : hi;
    const float th = thr[q];
    const u64 below = (1ull << lane) - 1;
    long base = 0;                                           // FILL: the slot of this wave's first hit
    if constexpr (FILL) base = lims[q] + mine[wave];
    long cnt = 0;                                            // (uniform) this wave's hits so far (a list named twice counts twice)

    CodeChunk<CH, T> cur;
    float t = 0.f;
    ListCursor<MASKED, BIAS> pos;
    pos.start(walk, step, stop, cur, t, codes, w, metric, N, mask, brow, lane);
    while (step < stop) {
        const long long nstep = step + 1;
        pos.peek(walk, nstep, stop, mask, brow, lane);
        float tn = t;
        float acc[1];
        tile_step<1, CH>(acc, cur, tn, Tl, codes, w, metric, N, K, pos.b, pos.bnext);
        const float s = score_finish(pos.biased(acc[0]), t, metric);
        const bool hit = pos.offer() && s <= th;             // rules 7, 15 and 17 (a NaN compares false)
        const u64 m = __ballot(hit);
        if constexpr (FILL) {
            if (m) {                                         // (uniform) hits are rare
                const long slot = base + cnt + __builtin_popcountll(m & below);
                if (hit && (unsigned long)slot < (unsigned long)capacity) {
                    out_s[slot] = s;
                    out_i[slot] = pos.b;
                }
            }
        }
        cnt += __builtin_popcountll(m);
        t = tn;
        pos.advance();
        step = nstep;
    }

    if constexpr (!FILL) {
        if (lane == 0) mine[wave] = cnt;
    }
}

// inclusive prefix sum over the 64 lanes of a wave (integers: any order gives the same sum)
__device__ __forceinline__ long wave_scan_incl(long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// One wave per query: its `per` = S * kRangeWaves counts become exclusive start offsets (in place, in (slice, wave) order) and
// their sum goes to lims[q + 1].
__global__ void __launch_bounds__(64)
k_range_offsets(int64_t *__restrict__ ws, int per, int64_t *__restrict__ lims) {
    const int q = blockIdx.x, lane = lane_id();
    int64_t *c = ws + (long)q * per;
    long base = 0;
    for (int e0 = 0; e0 < per; e0 += 64) {
        const long v = (e0 + lane < per) ? (long)c[e0 + lane] : 0;
        const long incl = wave_scan_incl(v, lane);
        if (e0 + lane < per) c[e0 + lane] = base + incl - v;
        base += __shfl(incl, 63, 64);
    }
    if (lane == 0) lims[q + 1] = base;
}

// One wave: lims[0] = 0 and lims[1 .. Q] (the per-query totals) become their inclusive prefix sums.  zero: all of lims is 0.
__global__ void __launch_bounds__(64)
k_range_lims(int64_t *__restrict__ lims, long Q, int zero) {
    const int lane = lane_id();
    if (lane == 0) lims[0] = 0;
    long base = 0;
    for (long e0 = 0; e0 < Q; e0 += 64) {
        const bool live = e0 + lane < Q;
        const long v = (live && !zero) ? (long)lims[1 + e0 + lane] : 0;
        const long incl = wave_scan_incl(v, lane);
        if (live) lims[1 + e0 + lane] = base + incl;
        base += __shfl(incl, 63, 64);
    }
}

}  // namespace mcq
