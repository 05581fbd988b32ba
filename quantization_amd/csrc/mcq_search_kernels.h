// mcq_search_kernels.h -- gfx950 kernels of the search over STORED CODES: which stored vectors are nearest to a query,
// answered from the codes themselves (no decode).  The quantizer is additive, x^_b = sum_n C[n][code[b][n]], so
//     |q - x^_b|^2 = |q|^2 + sum_n T_q[n][code[b][n]] + t_b,     T_q[n][k] = -2 <q, C[n][k]>,     t_b = |x^_b|^2.
//
// Arithmetic contract (include/mcq.h, "search over stored codes"; the tests restate rules 1, 2, 3, 4 and 6 in numpy):
//   1. k_search_tables: T[q][n*K + k] = -2 * (one fp32 chain over d ascending, accumulator starting at +0, each product rounded,
//      then added: -ffp-contract=off).  Chain length = the padded dim (the pad columns of `prepared` are zero).
//   2. k_code_norms: per lane l and float4 group g = l, l + 64, ...: v = ((C[0][c_0] + C[1][c_1]) + ...) per component (N - 1
//      additions), part = (((part + v0*v0) + v1*v1) + v2*v2) + v3*v3, then the xor butterfly 32, 16, 8, 4, 2, 1.  A code digit is
//      masked with K - 1 (as mcq_decode does).
//   3. tile_step + score_finish (in k_search_scan, and in k_range_sweep of mcq_range_kernels.h):
//      s[q][b] = (((T[c_0] + T[c_1]) + ...) + T[c_{N-1}]) + t[b], fp32 additions in exactly this order.
//      With a metric (k_search_scan<QT, N, M>; S is the sum of the N table entries above, w the per-candidate array):
//        kMetricL2   w[b] = t[b]                                   score = S + w[b]      (the line above)
//        kMetricIP   no w: the pointer is never read               score = S             (= -2 <q, x^_b>)
//        kMetricCos  w[b] = r[b] = 1 / sqrt(t[b]), 0 where t == 0  score = S * w[b]      (= -2 |q| cos(q, x^_b); one fp32 product)
//      r[b] is formed by k_code_norms<RNORM = true> / k_rnorms_from_norms: a correctly rounded square root, then a correctly rounded
//      division (no v_rsq_f32, no fast-math: the tests restate it as float32(1) / sqrt(t) in numpy and compare bits).
//   4. the result lists are the k smallest under "(s, b) ascending", listed in that order: pair_less below is the ONLY comparison
//      of the scan and of the merge, so the k indexes are a function of the scores alone.  No floating-point atomics anywhere.
//  10. a mask (k_search_scan<.., MASKED = true>, k_range_sweep likewise) is one bit per stored vector, bit b & 63 of the 64-bit
//      word b >> 6 (k_pack_mask makes one from a byte per vector); bits at positions >= B are ignored.
//  11. rules 3, 3', 4, 7 and 8 hold over the vectors whose bit is set, positions staying the original ones: a score is formed
//      by tile_step and score_finish as without a mask, the mask only decides whether a lane OFFERS its candidate.
//  12. no mask (MASKED = false) is the code as it was.  A step of 64 candidates is one aligned word of the mask (slices start
//      at multiples of 64), so a wave learns from one wave-uniform word that a step is empty and skips it whole: no code
//      load, no gather, no list insert (MaskWalk below).  Behind a cleared bit of a step that is not empty the codes and w are
//      loaded as always (in bounds: step_at) and the score, whatever it is, is never offered.
//  13-15. k_search_lists: the candidates of a query are the lists its row of probes names (and, under a mask, whose bit is set);
//      scores, order and tails are those above over these candidates, positions staying those of the store.
#pragma once
#include "mcq_kernels.h"
#include <hip/hip_fp16.h>

namespace mcq {

// ---- launch arithmetic (tests/search_grid.py reads these constants from this file and mirrors tile_plan and scan_plan of
// mcq_api.hip)
constexpr int kTabRows = 64;              // k_search_tables: table rows (n*K + k) per workgroup
constexpr int kTabQueries = 16;           //                  queries per workgroup
constexpr int kTabChunk = 32;             //                  features staged per step
constexpr int kNormWaves = 4;             // k_code_norms: stored vectors per workgroup, one wave each
constexpr int kPieceRows = 32 * 1024 * 1024;   // rows per launch of the kernels that spend a wave (64 threads) or more on a row
                                          // (k_code_norms, the per-vector decodes): 2^31 threads.  A launch of 2^32 threads or
                                          // more is not rejected by the runtime on gfx950: it returns 0 and runs the thread
                                          // count modulo 2^32 (launch_in_pieces of mcq_api.hip; DESIGN.md section 4,
                                          // "Stores past 2^26 rows")
constexpr int kScanWaves = 8;             // k_search_scan: waves per workgroup (512 threads)
constexpr int kScanQTMax = 16;            //                queries per tile at most
constexpr int kScanTableLds = 128 * 1024; //                bytes of LDS the tables of a tile may take (160 KiB per CU)
constexpr int kScanTargetBlocks = 256;    //                workgroups that fill the chip once (one per CU)
constexpr int kScanMaxSlices = 256;       //                cap of the slice count: the workspace stops growing with B here
constexpr int kMaskWindow = 64;           // MaskWalk: steps of a wave whose mask words one refill reads, one word per lane
constexpr int kNoIndex = 0x7fffffff;      // position of a list entry that holds no candidate (B <= 2^31 - 1: never a real one)
// the finishing operation of a candidate's score (MCQ_SEARCH_L2 / _IP / _COS of include/mcq.h): a template parameter of the scan
constexpr int kMetricL2 = 0;
constexpr int kMetricIP = 1;
constexpr int kMetricCos = 2;

// ---------------------------------------------------------------- the order
__device__ __forceinline__ bool pair_less(float s, int b, float ts, int tb) { return s < ts || (s == ts && b < tb); }

__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// The wave's list: lane l holds the entry of rank l under (s, b) (ls, li); (ts, tb) is the entry of rank k - 1 (uniform).
// Every lane offers one candidate (s, b) when `cand`; those below the current worst are inserted one by one (a NaN score
// compares false and is never inserted).  After warm-up inserts are rare: about k * ln(candidates / k) per list.
__device__ __forceinline__ void list_insert(float &ls, int &li, float &ts, int &tb, float s, int b, bool cand, int k, int lane) {
    u64 m = __ballot(cand && pair_less(s, b, ts, tb));
    while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const float ns = readlane_f(s, j);
        const int nb = __builtin_amdgcn_readlane(b, j);
        if (!pair_less(ns, nb, ts, tb)) continue;           // (uniform) the worst moved up since the ballot
        const float us = __shfl_up(ls, 1, 64);
        const int ui = __shfl_up(li, 1, 64);
        const bool after = pair_less(ns, nb, ls, li);       // my entry ranks after the new one: it moves down one lane
        const bool up_after = lane > 0 && pair_less(ns, nb, us, ui);
        if (after) {
            ls = up_after ? us : ns;
            li = up_after ? ui : nb;
        }
        ts = readlane_f(ls, k - 1);
        tb = __builtin_amdgcn_readlane(li, k - 1);
    }
}

// ------------------------------------------------------------------- tables
// T[q][r] = -2 * sum_d q[d] * C[r][d], r = n*K + k: an LDS-tiled fp32 product, 64 rows x 16 queries per workgroup, thread
// (r = tid & 63, g = tid >> 6) forms the four queries 4g .. 4g+3 of row r.  One chain over d ascending per entry.
__global__ void __launch_bounds__(256)
k_search_tables(const void *__restrict__ qv, int q_is_fp16, int Q, const float *__restrict__ C, int NK, int D, int Dp,
                float *__restrict__ T) {
    __shared__ float cs[kTabRows][kTabChunk + 1];           // (+1: lane r reads bank (r + d) mod 32)
    __shared__ float qs[kTabQueries][kTabChunk];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    const int r0 = blockIdx.y * kTabRows, q0 = blockIdx.x * kTabQueries;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < Dp; d0 += kTabChunk) {
        for (int e = tid; e < kTabRows * kTabChunk; e += 256) {
            const int rr = e / kTabChunk, dd = e % kTabChunk;
            cs[rr][dd] = (r0 + rr < NK && d0 + dd < Dp) ? C[(long)(r0 + rr) * Dp + d0 + dd] : 0.f;
        }
        for (int e = tid; e < kTabQueries * kTabChunk; e += 256) {
            const int qq = e / kTabChunk, dd = e % kTabChunk;
            float v = 0.f;
            if (q0 + qq < Q && d0 + dd < D) {
                const long at = (long)(q0 + qq) * D + d0 + dd;
                v = q_is_fp16 ? __half2float(static_cast<const __half *>(qv)[at]) : static_cast<const float *>(qv)[at];
            }
            qs[qq][dd] = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int dd = 0; dd < kTabChunk; ++dd) {
            const float c = cs[r][dd];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = acc[i] + qs[4 * g + i][dd] * c;
        }
        __syncthreads();
    }
    if (r0 + r < NK) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (q0 + 4 * g + i < Q) T[(long)(q0 + 4 * g + i) * NK + r0 + r] = -2.f * acc[i];
    }
}

// -------------------------------------------------------------------- norms
// r = 1 / sqrt(t), and 0 for t == 0 (an all-zero reconstruction scores 0 under the cosine, never NaN).  A negative or NaN t
// gives NaN, which no list ever takes.
__device__ __forceinline__ float rnorm_of(float t) { return t == 0.f ? 0.f : 1.0f / sqrtf(t); }

// t[b] = |sum_n C[n][code[b][n]]|^2: the decode body without the store.  One wave per stored vector.  RNORM: r[b] leaves instead.
// BASED: t[b] = |base[assign[b]] + sum_n C[n][code[b][n]]|^2 (rule 22), the norms of a store of RESIDUAL codes, whose vector b
// is its list's coarse centroid plus the decode of its code: one more addition per feature -- the codebook rows n ascending,
// THEN the base element, then the same per-lane chains and butterfly.  base is float[L][D] with row stride D (not the padded
// Dp; a row need not be 16-byte aligned, so it is read element by element), features d >= D get no base (the pad columns of
// C are zero: they contribute zero).  assign[b] outside [0, L) adds no base row.  Without BASED the four last arguments are
// never read.
// T: the type of a stored digit, uint8_t or uint16_t (two-byte codes, include/mcq_code16.h rule 32): lane n reads digit n as
// one element of T.
template <bool RNORM, bool BASED, typename T = uint8_t>
__global__ void __launch_bounds__(64 * kNormWaves)
k_code_norms(const T *__restrict__ codes, long B, const float *__restrict__ C, int N, int K, int Dp,
             float *__restrict__ norms, const float *__restrict__ base, long L, int D, const int *__restrict__ assign) {
    const long b = (long)blockIdx.x * kNormWaves + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = lane_id();
    const int mine = (lane < N) ? (codes[b * N + lane] & (K - 1)) : 0;     // lane n holds digit n (N <= 64)
    bool based = false;                                      // (uniform: one stored vector per wave)
    const float *row = nullptr;
    if constexpr (BASED) {
        const int a = assign[b];
        based = a >= 0 && a < L;
        row = base + (based ? (long)a * D : 0);
    }
    float part = 0.f;
    for (int g0 = 0; g0 < Dp / 4; g0 += 64) {                // (uniform trip count: the digits are read from ALL lanes below)
        const int g = g0 + lane;
        const bool live = g < Dp / 4;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int n = 0; n < N; ++n) {
            const int kk = __builtin_amdgcn_readlane(mine, n);
            const f32x4 c = live ? *reinterpret_cast<const f32x4 *>(C + ((long)n * K + kk) * Dp + 4 * g) : v;
            v = (n == 0) ? c : v + c;
        }
        if (!live) v = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if constexpr (BASED) {
                if (based && 4 * g + c < D) v[c] = v[c] + row[4 * g + c];
            }
            part = part + v[c] * v[c];
        }
    }
    part = wave_sum_butterfly(part);
    if (lane == 0) norms[b] = RNORM ? rnorm_of(part) : part;
}

// r[b] from t[b] a store already keeps (code_norms): no center is gathered again
__global__ void __launch_bounds__(256)
k_rnorms_from_norms(const float *__restrict__ norms, long B, float *__restrict__ rnorms) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b < B) rnorms[b] = rnorm_of(norms[b]);
}

// --------------------------------------------------------------------- scan
// A workgroup owns a tile of QT queries and one slice of the stored codes.  The tile's tables sit in LDS INTERLEAVED by
// query, Tl[(n*K + k) * QT + q]: the QT entries a candidate needs for codebook n are one contiguous run (QT / 4 ds_read_b128
// at one address) instead of QT scattered ds_read_b32.  Each lane takes one candidate per step: it loads the N code bytes once
// (one vector load) and reuses them for every query of the tile.  Every wave keeps one sorted list per query in registers, one
// entry per lane; the waves' lists are merged per query through LDS (the tables are dead by then) and the workgroup leaves one
// list of k entries per (query, slice) in the workspace.
// Up to 8 codebooks' digits of one candidate: one vector load.  T is the type of a stored digit: uint8_t (the default: every
// kernel written before two-byte codes existed is the instantiation it was), four digits to a word, or uint16_t
// (include/mcq_code16.h rule 32), two digits to a word and a load of 2, 4, 8 or 16 bytes.  Either way a digit is masked with
// K - 1 by the caller's kmask, so whatever bits a stored element holds the LDS read stays inside the table.
template <int CH, typename T = uint8_t>
struct CodeChunk {
    static_assert(sizeof(T) == 1 || sizeof(T) == 2, "one-byte or two-byte digits");
    static constexpr int PER = 4 / (int)sizeof(T);           // digits per 32-bit word
    static constexpr int WORDS = (CH + PER - 1) / PER;
    uint32_t w[WORDS];
    __device__ __forceinline__ void load(const T *__restrict__ p) {
        static_assert(CH == 1 || CH == 2 || CH == 4 || CH == 8, "chunks of 1, 2, 4 or 8 codebooks");
        if constexpr (CH * sizeof(T) <= 1) {
            w[0] = p[0];
        } else if constexpr (CH * sizeof(T) == 2) {
            w[0] = *reinterpret_cast<const uint16_t *>(p);
        } else if constexpr (CH * sizeof(T) == 4) {
            w[0] = *reinterpret_cast<const uint32_t *>(p);
        } else if constexpr (CH * sizeof(T) == 8) {
            const uint2 v = *reinterpret_cast<const uint2 *>(p);
            w[0] = v.x;
            w[1] = v.y;
        } else {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            w[0] = v.x;
            w[1] = v.y;
            w[2] = v.z;
            w[3] = v.w;
        }
    }
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < WORDS; ++i) w[i] = 0;
    }
    __device__ __forceinline__ int digit(int n, int kmask) const {
        if constexpr (sizeof(T) == 1) return (int)(w[n >> 2] >> (8 * (n & 3))) & kmask;
        return (int)(w[n >> 1] >> (16 * (n & 1))) & kmask;
    }
};

// ---- the tile scorer: everything k_search_scan and k_range_sweep (mcq_range_kernels.h) share -- the staging of the tables,
// the digit stream with its loads one step ahead, the N additions of rule 3 and the metric's last operation.  They exist
// HERE and nowhere else, so the two kernels cannot disagree about a score; a kernel decides only which steps a wave owns
// and what becomes of a step's QT scores.

// the finishing operation of rule 3 / 3'.  The scan passes its template parameter M (the switch folds away), the sweep a
// wave-uniform runtime value.
__device__ __forceinline__ float score_finish(float S, float w, int metric) {
    return metric == kMetricL2 ? S + w : (metric == kMetricCos ? S * w : S);
}

// the tile's tables -> LDS, interleaved by query: Tl[(n*K + k) * QT + q]; a query past the end of the call reads as zeros
template <int QT, int THREADS>
__device__ __forceinline__ void tile_stage(float *Tl, const float *__restrict__ tables, int Q, int q0, int NK, int tid) {
    for (int e = tid; e < NK * QT; e += THREADS) {
        const int q = e % QT, j = e / QT;
        Tl[e] = (q0 + q < Q) ? tables[(long)(q0 + q) * NK + j] : 0.f;
    }
    __syncthreads();
}

// candidates [begin, end) of the store, in `steps` steps of 64 (one candidate per lane)
struct Slice {
    long begin, end, steps;
};
__device__ __forceinline__ Slice slice_of(int slice, long per_slice, long B) {
    const long begin = (long)slice * per_slice;
    const long end = (begin + per_slice < B) ? begin + per_slice : B;
    return {begin, end, (end - begin + 63) / 64};
}

// the candidate of this lane in step `step` of the slice; lanes past the end of the slice re-read its last candidate (in
// bounds) and offer nothing
__device__ __forceinline__ long step_at(const Slice &sl, long step, int lane) {
    const long b = sl.begin + step * 64 + lane;
    return b < sl.end ? b : sl.end - 1;
}

// What a step needs from HBM travels one step ahead, in two plain locals of the kernel: `cur`, its first CH digits, and its
// w (t[b] under L2, r[b] under the cosine, never read under kMetricIP).  tile_first loads those of a wave's first step (none
// when it has no step: first >= stop).  `metric` and N may be compile-time values of the caller here and in tile_step.
template <int CH, typename T>
__device__ __forceinline__ void tile_first(CodeChunk<CH, T> &cur, float &t, const T *__restrict__ codes,
                                           const float *__restrict__ w, int metric, int N, const Slice &sl, long first, long stop,
                                           int lane) {
    if (first < stop) {
        cur.load(codes + step_at(sl, first, lane) * N);
        if (metric != kMetricIP) t = w[step_at(sl, first, lane)];
    } else {
        cur.clear();
    }
}

// ---- the mask (rules 10-12): which of a wave's steps are worth taking.  The wave's steps are first, first + stride, ... below
// stop (stride kScanWaves in the scan, 1 in the sweeps).  A refill reads the words of the next kMaskWindow of them, one per
// lane (none past stop; the last step of the slice keeps only the bits below the slice's end, which drops the bits at
// positions >= B); a ballot of "non-zero" is the set of steps of the window that hold a candidate, and next() walks its set
// bits.  Everything but `mine` is wave-uniform (first comes through readfirstlane), so the kernels' loops over next() branch
// on scalars.
struct MaskWalk {
    const u64 *words;                                        // word i belongs to step i of the slice
    int ahead, stop, stride, last;                           // `ahead`: the first step no refill has read yet; last: steps - 1
    int base;                                                // the step of lane 0's word
    u64 tail, live, mine;                                    // live: the window's non-empty steps not yet handed out

    __device__ __forceinline__ MaskWalk(const u64 *__restrict__ mask, const Slice &sl, long first, long stop_, int stride_)
        : words(mask + sl.begin / 64), ahead(__builtin_amdgcn_readfirstlane((int)first)),
          stop(__builtin_amdgcn_readfirstlane((int)stop_)), stride(stride_), last((int)sl.steps - 1), base(0), live(0), mine(0) {
        const int c = (int)(sl.end - sl.begin) - 64 * last;  // candidates of the slice's last step: 1 .. 64
        tail = c == 64 ? ~0ull : (1ull << c) - 1;
    }

    // -> the wave's next step that holds a candidate, and its word (bit l: lane l offers its candidate); -1: there is none
    __device__ __forceinline__ int next(u64 &word, int lane) {
        while (live == 0) {
            if (ahead >= stop) return -1;
            const int step = ahead + lane * stride;
            mine = step < stop ? words[step] : 0;
            if (step == last) mine &= tail;
            base = ahead;
            ahead += kMaskWindow * stride;
            live = __ballot(mine != 0);
        }
        const int j = __builtin_ctzll(live);
        live &= live - 1;
        word = readlane_u64(mine, j);
        return base + j * stride;
    }
};

// a byte per stored vector -> the mask of rule 10: a wave reads 64 flags and one ballot is the word (the bits past B are zero)
constexpr int kPackWaves = 4;
__global__ void __launch_bounds__(64 * kPackWaves)
k_pack_mask(const uint8_t *__restrict__ flags, long B, u64 *__restrict__ mask) {
    const long word = (long)blockIdx.x * kPackWaves + (threadIdx.x >> 6);
    const long b = word * 64 + lane_id();
    const u64 m = __ballot(b < B && flags[b] != 0);
    if (lane_id() == 0 && word * 64 < B) mask[word] = m;
}

// One step of one wave against the QT queries of the staged tile: acc[q] = the N table additions of rule 3 in codebook order,
// the digits arriving in N / CH chunks of CH codebooks.  b is the lane's candidate of this step and bnext that of the wave's
// next step (b again in its last), both from step_at: the kernel says which step comes next.  `cur` holds the digits of b on
// entry and those of bnext on return; w[bnext] goes to tn (untouched under kMetricIP).
// NCONST: N where the caller has it as a template parameter (the scan), 0 where N is a runtime value (the sweep).  The chunk
// count has to be a constant BEFORE inlining: without it the scans of two chunks (N = 16) under kMetricIP compile to a branch
// where the loop had a select, and take up to 13 VGPRs more.
// T: the digit type, deduced from `cur` and `codes`; the chunks of a row sit CH elements of T apart.
template <int QT, int CH, int NCONST = 0, typename T>
__device__ __forceinline__ void tile_step(float (&acc)[QT], CodeChunk<CH, T> &cur, float &tn, const float *Tl,
                                          const T *__restrict__ codes, const float *__restrict__ w, int metric, int N, int K,
                                          long b, long bnext) {
    const int kmask = K - 1, nch = NCONST ? NCONST / CH : N / CH;
    const T *p = codes + b * N;
#pragma unroll
    for (int q = 0; q < QT; ++q) acc[q] = -0.f;              // (-0) + x == x for every x, signed zeros included
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
        CodeChunk<CH, T> nxt;                                // the next step's digits travel while this one gathers
        if (c + 1 < nch) {
            nxt.load(p + (c + 1) * CH);
        } else {
            nxt.load(codes + bnext * N);
            if (metric != kMetricIP) tn = w[bnext];
        }
#pragma unroll
        for (int n = 0; n < CH; ++n) {
            const float *row = Tl + ((c * CH + n) * K + cur.digit(n, kmask)) * QT;
            if constexpr (QT >= 4) {
#pragma unroll
                for (int q4 = 0; q4 < QT / 4; ++q4) {
                    const f32x4 v = reinterpret_cast<const f32x4 *>(row)[q4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[4 * q4 + i] = acc[4 * q4 + i] + v[i];
                }
            } else {
#pragma unroll
                for (int q = 0; q < QT; ++q) acc[q] = acc[q] + row[q];
            }
        }
        cur = nxt;
    }
}

// M: what finishes a score (rule 3).  w is t[b] (L2) or r[b] (cosine); the inner-product scan has no w and loads none.
// MASKED: `mask` decides which candidates are offered (rules 10-12); without it the pointer is never read.
template <int QT, int N, int M, bool MASKED>
__global__ void __launch_bounds__(64 * kScanWaves)
k_search_scan(const float *__restrict__ tables, int Q, const uint8_t *__restrict__ codes, const float *__restrict__ w,
              long B, int K, int k, int S, long per_slice, float *__restrict__ ws_s, int *__restrict__ ws_i,
              const u64 *__restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) char search_smem[];
    constexpr int CH = N < 8 ? N : 8;                        // a candidate's digits arrive in N / CH chunks of CH
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x / S, slice = blockIdx.x % S;
    const int q0 = tile * QT;
    tile_stage<QT, 64 * kScanWaves>(reinterpret_cast<float *>(search_smem), tables, Q, q0, N * K, tid);

    float ls[QT], ts[QT];
    int li[QT], tb[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        ls[q] = ts[q] = __builtin_inff();
        li[q] = tb[q] = kNoIndex;
    }

    // the waves of a workgroup take the steps of its slice in turn: wave v owns v, v + kScanWaves, ...
    const Slice sl = slice_of(slice, per_slice, B);
    const float *Tl = reinterpret_cast<const float *>(search_smem);
    CodeChunk<CH> cur;
    float t = 0.f;
    if constexpr (MASKED) {
        // the same loop over the wave's steps that hold a candidate: "next step" is the next of THOSE, and its digits and w
        // travel ahead as below.  A wave without one loads nothing and its lists stay kNoIndex.
        MaskWalk walk(mask, sl, wave, sl.steps, kScanWaves);
        u64 word = 0, word_next = 0;
        int blk = walk.next(word, lane);
        tile_first(cur, t, codes, w, M, N, sl, blk < 0 ? sl.steps : blk, sl.steps, lane);
        while (blk >= 0) {
            const int nblk = walk.next(word_next, lane);
            const long bl = sl.begin + (long)blk * 64 + lane;
            float tn = t;
            float acc[QT];
            tile_step<QT, CH, N>(acc, cur, tn, Tl, codes, w, M, N, K, step_at(sl, blk, lane), step_at(sl, nblk < 0 ? blk : nblk, lane));
#pragma unroll
            for (int q = 0; q < QT; ++q)             // (a set bit lies inside the slice: MaskWalk trims the last word)
                list_insert(ls[q], li[q], ts[q], tb[q], score_finish(acc[q], t, M), (int)bl, (word >> lane) & 1, k, lane);
            t = tn;
            blk = nblk;
            word = word_next;
        }
    } else {
        tile_first(cur, t, codes, w, M, N, sl, wave, sl.steps, lane);
        for (long blk = wave; blk < sl.steps; blk += kScanWaves) {
            const long bl = sl.begin + blk * 64 + lane;
            const long bnext = blk + kScanWaves < sl.steps ? step_at(sl, blk + kScanWaves, lane) : step_at(sl, blk, lane);
            float tn = t;
            float acc[QT];
            tile_step<QT, CH, N>(acc, cur, tn, Tl, codes, w, M, N, K, step_at(sl, blk, lane), bnext);
#pragma unroll
            for (int q = 0; q < QT; ++q)
                list_insert(ls[q], li[q], ts[q], tb[q], score_finish(acc[q], t, M), (int)bl, bl < sl.end, k, lane);
            t = tn;
        }
    }

    // the waves' lists -> LDS -> one list per query of the tile
    __syncthreads();
    float *Ls = reinterpret_cast<float *>(search_smem);
    int *Li = reinterpret_cast<int *>(search_smem + (size_t)QT * kScanWaves * 64 * 4);
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        Ls[(q * kScanWaves + wave) * 64 + lane] = ls[q];
        Li[(q * kScanWaves + wave) * 64 + lane] = li[q];
    }
    __syncthreads();
    for (int q = wave; q < QT; q += kScanWaves) {
        if (q0 + q >= Q) break;
        float ms = __builtin_inff(), mts = __builtin_inff();
        int mi = kNoIndex, mtb = kNoIndex;
        for (int w = 0; w < kScanWaves; ++w) {
            const float s = Ls[(q * kScanWaves + w) * 64 + lane];
            const int b = Li[(q * kScanWaves + w) * 64 + lane];
            list_insert(ms, mi, mts, mtb, s, b, lane < k && b != kNoIndex, k, lane);
        }
        if (lane < k) {
            const long at = ((long)(q0 + q) * S + slice) * k + lane;
            ws_s[at] = ms;
            ws_i[at] = mi;
        }
    }
}

// -------------------------------------------------------------------- merge
// One wave per query: the S lists of its slices -> the final k under the same order.  An entry that holds no candidate
// (fewer than k stored vectors) leaves as (+inf, -1).  S == 0 (an empty store) only writes that fill.
__global__ void __launch_bounds__(64)
k_search_merge(const float *__restrict__ ws_s, const int *__restrict__ ws_i, int S, int k, float *__restrict__ out_s,
               int64_t *__restrict__ out_i) {
    const int q = blockIdx.x, lane = lane_id();
    const long total = (long)S * k, base = (long)q * total;
    float ms = __builtin_inff(), mts = __builtin_inff();
    int mi = kNoIndex, mtb = kNoIndex;
    float s = 0.f;
    int b = kNoIndex;
    if (lane < total) {
        s = ws_s[base + lane];
        b = ws_i[base + lane];
    }
    for (long e0 = 0; e0 < total; e0 += 64) {
        float sn = 0.f;
        int bn = kNoIndex;
        if (e0 + 64 + lane < total) {
            sn = ws_s[base + e0 + 64 + lane];
            bn = ws_i[base + e0 + 64 + lane];
        }
        list_insert(ms, mi, mts, mtb, s, b, b != kNoIndex, k, lane);
        s = sn;
        b = bn;
    }
    if (lane < k) {
        out_s[(long)q * k + lane] = ms;
        out_i[(long)q * k + lane] = (mi == kNoIndex) ? (int64_t)-1 : (int64_t)mi;
    }
}

// -------------------------------------------------------------------- lists
// The search list by list (rules 13-16): the store is in list order, list l is [list_offsets[l], list_offsets[l + 1]), and
// query q is scored against the lists its row of `probes` names and no others.  The candidate sets differ per query, so a
// code is no longer shared by the queries of a tile: a workgroup is ONE query (QT = 1) and part s of S of ITS candidates.
//   * step space: per probe the range clamped to [0, B] (begin >= end, and a probe outside [0, L), are empty) and its steps
//     of 64 candidates, ceil(len / 64); an exclusive prefix sum over the probes flattens them into T steps.  Part s owns
//     the steps [s*T/S, (s+1)*T/S): the candidates are cut by COUNT, whichever lists they sit in (a cut by position leaves
//     one part all the work when the candidates are one run).  A part's waves take its steps in turn.
//   * a step is (probe p, offset j in its list) with pre[p] <= step < pre[p + 1]: found once per wave by bisection, then by
//     a pointer that walks up (the steps of a wave ascend).  The lane's candidate is begin + 64*j + lane, lanes past the
//     list's end re-read its last candidate and offer nothing (step_at over the list as a Slice).
//   * the score is tile_step<1, CH, N> + score_finish, as everywhere; the next step's candidate, across a list boundary too,
//     is the bnext of tile_step, so codes and w still travel one step ahead.  Under a mask each lane tests its own bit.
//   * the waves' lists are merged through LDS as in k_search_scan and leave as list (q, s) of the workspace: k_search_merge
//     finishes the call.  No atomics of any kind.
//   * with a bias (BIAS; residual codes, rules 21-23 of include/mcq_residual.h): list l keeps the codes of x - c_l, so a
//     candidate's score lacks the share of its list's centroid, bias[q][p] = -2 <q, c_{probes[q][p]}>: one value per (query,
//     probe slot), added to the table sum of every candidate of that slot's list BEFORE the metric's finishing operation,
//         score = score_finish(S + bias[q*P + p], w[b], metric)         S: the chain tile_step leaves (rule 3)
//     and w then holds |c_l + r^_b|^2 or its reciprocal root (k_code_norms<.., BASED>).  The bias is a flag of k_search_lists
//     and k_range_lists: probe_bias is their last argument, and without the flag it is null and never read.
//     The bias of a step belongs to the step's probe slot, walk.p as seek() or at() left it.  peek() moves walk.p on to the
//     NEXT step's slot before the current step's score is finished, so the bias travels as b, live and word do: bias for the
//     current step, bias_next set in peek() and moved in advance().  It is read from global memory (one address per wave:
//     the row is P floats, hot in L2 after the first part of a query) one step ahead of its use, as the codes and w are; a
//     slot that names no list has no step, so its bias is never read.
// LDS: [the table, N*K floats; later the waves' lists][pre: int64 P + 1][begin: int32 P][end: int32 P].
constexpr int kListWaves = 4;             // k_search_lists: waves per workgroup (256 threads)
constexpr int kListTargetBlocks = 1024;   //                 workgroups that fill the chip once (4 per CU, 4 waves per SIMD)
// probes per query at most.  A query's per-probe ranges and prefix sums take 16 bytes per probe (8 + 4 + 4) and live in LDS
// beside up to 64 KiB of tables (N*K = 64 * 256 floats): 64 KiB + 4096 * 16 B + 8 B = 128 KiB + 8 B of the CU's 160 KiB.
// Twice as many probes would need 192 KiB.
constexpr int kListMaxProbes = 4096;

// bytes of the first LDS region: the table, and after the scoring the kListWaves lists of 64 (score, position) pairs
__host__ __device__ constexpr int lists_lds_head(int NK) {
    return ((NK * 4 > kListWaves * 64 * 8 ? NK * 4 : kListWaves * 64 * 8) + 15) & ~15;
}
__host__ __device__ constexpr int lists_lds_bytes(int NK, int P) { return lists_lds_head(NK) + (P + 1) * 8 + P * 8; }

// The step space of one query, in LDS behind the first region, and the (probe, list) of a step.  build() is called by every
// thread of a workgroup of THREADS: it lays out pre / begin / end, fills them from the query's row of `probes` and hands back T,
// the number of steps.  seek() finds a wave's first step by bisection; at() walks p up from there until pre[p] <= step <
// pre[p + 1] (step < T; probes without a step are passed).  j: the step's offset in its list, in steps.
struct ListWalk {
    long long *pre;
    int *lbeg, *lend;
    int P, p;

    template <int THREADS>
    __device__ __forceinline__ long long build(char *smem, int NK, const int64_t *__restrict__ list_offsets, long L,
                                               const int *__restrict__ row, int P_, long B, int tid) {
        const int lane = tid & 63, wave = tid >> 6;
        pre = reinterpret_cast<long long *>(smem + lists_lds_head(NK));
        lbeg = reinterpret_cast<int *>(pre + P_ + 1);
        lend = lbeg + P_;
        P = P_;
        p = 0;
        // clamped ranges and step counts, then the prefix sums in chunks of 64 through wave 0
        for (int e = tid; e < P; e += THREADS) {
            const int l = row[e];
            long a = 0, z = 0;
            if (l >= 0 && l < L) {
                a = list_offsets[l];
                z = list_offsets[l + 1];
                a = a < 0 ? 0 : (a > B ? B : a);             // (defence: a range never leaves [0, B], whatever the offsets hold)
                z = z < 0 ? 0 : (z > B ? B : z);
                if (a >= z) a = z = 0;
            }
            lbeg[e] = (int)a;
            lend[e] = (int)z;
            pre[e + 1] = (z - a + 63) / 64;
        }
        __syncthreads();
        if (wave == 0) {
            long long carry = 0;
            for (int c0 = 0; c0 < P; c0 += 64) {
                const int e = c0 + lane;
                long long v = e < P ? pre[e + 1] : 0;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const long long u = __shfl_up(v, d, 64);
                    if (lane >= d) v += u;
                }
                v += carry;
                if (e < P) pre[e + 1] = v;
                carry = __shfl(v, 63, 64);
            }
            if (lane == 0) pre[0] = 0;
        }
        __syncthreads();
        return pre[P];
    }
    // (every thread of the workgroup; k_range_lists over two-byte codes) the whole store as ONE implicit list [0, B), laid
    // out as build() lays out a row of one probe -> its steps
    __device__ __forceinline__ long long whole(char *smem, int NK, long B, int tid) {
        pre = reinterpret_cast<long long *>(smem + lists_lds_head(NK));
        lbeg = reinterpret_cast<int *>(pre + 2);
        lend = lbeg + 1;
        P = 1;
        p = 0;
        const long long T = (B + 63) / 64;
        if (tid == 0) {
            pre[0] = 0;
            pre[1] = T;
            lbeg[0] = 0;
            lend[0] = (int)B;
        }
        __syncthreads();
        return T;
    }
    __device__ __forceinline__ Slice seek(long long step, long &j) {
        int a = 0, z = P;                                    // pre[a] <= step < pre[z]
        while (z - a > 1) {
            const int mid = (a + z) >> 1;
            if (pre[mid] <= step) a = mid; else z = mid;
        }
        p = a;
        return at(step, j);
    }
    __device__ __forceinline__ Slice at(long long step, long &j) {
        while (p + 1 < P && pre[p + 1] <= step) ++p;
        j = (long)(step - pre[p]);
        return {lbeg[p], lend[p], 0};
    }
};

// This lane's candidate in the current step of a wave, and in the step the wave takes next: the position b (lanes past the
// end of the list re-read its last candidate, step_at over the list as a Slice), whether it lies inside its list, and under
// MASKED the mask word that holds its bit (lists do not start at multiples of 64: every lane tests its own).  The kernel owns
// the steps -- which comes next, and where the wave stops -- and the score; the next step's b is the bnext of tile_step.
// BIAS: the bias of the step's probe slot (see "lists" above) travels as b, live and word do; brow is the query's row of
// probe_bias, null and never read without one.
template <bool MASKED, bool BIAS>
struct ListCursor {
    long b, bnext;
    bool live, live_next;
    u64 word, word_next;
    float bias, bias_next;

    // the wave's first step: its digits and w go to cur and t (tile_first: one step, or none when step >= stop)
    template <int CH, typename T>
    __device__ __forceinline__ void start(ListWalk &walk, long long step, long long stop, CodeChunk<CH, T> &cur, float &t,
                                          const T *__restrict__ codes, const float *__restrict__ w, int metric, int N,
                                          const u64 *__restrict__ mask, const float *__restrict__ brow, int lane) {
        Slice sl{0, 1, 0};
        long j = 0;
        if (step < stop) sl = walk.seek(step, j);
        tile_first(cur, t, codes, w, metric, N, sl, j, step < stop ? j + 1 : j, lane);
        b = step_at(sl, j, lane);
        live = sl.begin + j * 64 + lane < sl.end;
        word = 0;
        if constexpr (MASKED) {
            if (step < stop) word = mask[b >> 6];
        }
        if constexpr (BIAS) {
            bias = 0.f;
            if (step < stop) bias = brow[walk.p];            // (walk.p < P: seek() found the step's slot)
        }
    }
    // the step after the current one is nstep (none when nstep >= stop: b again, offering nothing)
    __device__ __forceinline__ void peek(ListWalk &walk, long long nstep, long long stop, const u64 *__restrict__ mask,
                                         const float *__restrict__ brow, int lane) {
        bnext = b;
        live_next = false;
        if (nstep < stop) {
            long j;
            const Slice sl = walk.at(nstep, j);
            bnext = step_at(sl, j, lane);
            live_next = sl.begin + j * 64 + lane < sl.end;
        }
        word_next = 0;
        if constexpr (MASKED) word_next = mask[bnext >> 6];
        if constexpr (BIAS) {
            bias_next = bias;
            if (nstep < stop) bias_next = brow[walk.p];      // (at() moved walk.p to the slot of nstep)
        }
    }
    __device__ __forceinline__ bool offer() const {
        if constexpr (MASKED) return live && ((word >> (b & 63)) & 1);
        return live;
    }
    // the table sum S of the current step with its slot's bias: what score_finish takes
    __device__ __forceinline__ float biased(float S) const {
        if constexpr (BIAS) return S + bias;
        return S;
    }
    __device__ __forceinline__ void advance() {
        b = bnext;
        live = live_next;
        word = word_next;
        if constexpr (BIAS) bias = bias_next;
    }
};

template <int N, int M, bool MASKED, bool BIAS>
__global__ void __launch_bounds__(64 * kListWaves)
k_search_lists(const float *__restrict__ tables, int Q, const uint8_t *__restrict__ codes, const float *__restrict__ w,
               long B, int K, int k, int S, const int64_t *__restrict__ list_offsets, long L, const int *__restrict__ probes,
               int P, float *__restrict__ ws_s, int *__restrict__ ws_i, const u64 *__restrict__ mask,
               const float *__restrict__ probe_bias) {
    extern __shared__ __attribute__((aligned(16))) char search_smem[];
    constexpr int CH = N < 8 ? N : 8;
    constexpr int THREADS = 64 * kListWaves;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / S, part = blockIdx.x % S;
    ListWalk walk;
    const long long T = walk.build<THREADS>(search_smem, N * K, list_offsets, L, probes + (long)q * P, P, B, tid);
    const long long lo = T * part / S, hi = T * (part + 1) / S;           // (T <= 2^37, S <= 256)
    if (lo >= hi) {                                          // no step: the empty list, and nothing is staged
        if (tid < k) {
            const long at = ((long)q * S + part) * k + tid;
            ws_s[at] = __builtin_inff();
            ws_i[at] = kNoIndex;
        }
        return;
    }
    tile_stage<1, THREADS>(reinterpret_cast<float *>(search_smem), tables, Q, q, N * K, tid);
    const float *Tl = reinterpret_cast<const float *>(search_smem);
    const float *brow = BIAS ? probe_bias + (long)q * P : nullptr;

    float ls = __builtin_inff(), ts = __builtin_inff();
    int li = kNoIndex, tb = kNoIndex;
    CodeChunk<CH> cur;
    float t = 0.f;
    ListCursor<MASKED, BIAS> pos;
    long long step = lo + wave;
    pos.start(walk, step, hi, cur, t, codes, w, M, N, mask, brow, lane);
    while (step < hi) {
        const long long nstep = step + kListWaves;
        pos.peek(walk, nstep, hi, mask, brow, lane);
        float tn = t;
        float acc[1];
        tile_step<1, CH, N>(acc, cur, tn, Tl, codes, w, M, N, K, pos.b, pos.bnext);
        list_insert(ls, li, ts, tb, score_finish(pos.biased(acc[0]), t, M), (int)pos.b, pos.offer(), k, lane);
        t = tn;
        pos.advance();
        step = nstep;
    }

    // the waves' lists -> LDS -> the list of (query, part)
    __syncthreads();
    float *Ls = reinterpret_cast<float *>(search_smem);
    int *Li = reinterpret_cast<int *>(search_smem + (size_t)kListWaves * 64 * 4);
    Ls[wave * 64 + lane] = ls;
    Li[wave * 64 + lane] = li;
    __syncthreads();
    if (wave == 0) {
        float ms = __builtin_inff(), mts = __builtin_inff();
        int mi = kNoIndex, mtb = kNoIndex;
        for (int v = 0; v < kListWaves; ++v) {
            const float s = Ls[v * 64 + lane];
            const int c = Li[v * 64 + lane];
            list_insert(ms, mi, mts, mtb, s, c, lane < k && c != kNoIndex, k, lane);
        }
        if (lane < k) {
            const long at = ((long)q * S + part) * k + lane;
            ws_s[at] = ms;
            ws_i[at] = mi;
        }
    }
}

}  // namespace mcq
