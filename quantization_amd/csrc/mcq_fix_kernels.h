// mcq_fix_kernels.h -- the three inner-product tables of the path (logits :277-279, x.C and the Gram matrix of the
// centers: oracle/mcq_oracle.c "fixdot") as EXACT fixed-point products on the i8 matrix cores of gfx950.
//
// A row v is held as 30-bit fixed point against its own largest magnitude (row exponent e: max|v| < 2^e,
// q = rint(v * 2^(30-e))) and q as four signed 8-bit limbs, q = l0*2^24 + l1*2^16 + l2*2^8 + l3.  The product of two rows is
//     T_s = sum_k sum_{i+j=s} la_i[k] * lb_j[k]          s = 0..3: ten limb products, four i32 accumulator sets
//     t   = fma(T_0, 2^24, fma(T_1, 2^16, fma(T_2, 2^8, (float)T_3)))     (int -> float conversions round to nearest even)
//     fixdot = ldexp(t, ea + eb - 36)
// The T_s are exact integers, so nothing depends on the order the matrix cores add in; products of weight 2^-32 and
// below (i + j >= 4) are dropped.  v_mfma_i32_32x32x32_i8 runs at 32x the rate of the fp32 MFMA; ten of them replace one
// fp32 product step.
//
// Layout of a limb matrix with R rows (R a multiple of 128) and Dq columns (a multiple of 128): one "plane" per
// (16-column chunk c, limb l), each plane R x 16 bytes:  byte ((c * 4 + l) * R + row) * 16 + (k % 16).  A 128-row tile of
// one plane is 2 KB contiguous: the GEMM brings it into LDS with two 1 KB LDS-DMA loads and reads MFMA fragments
// (16 consecutive k of one row) straight out of it with ds_read_b128, 16 lanes per 256 contiguous bytes.
#pragma once
#include "mcq_kernels.h"

namespace mcq {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kFixTile = 128;          // rows per tile, both operands
constexpr int kFixColPad = 128;        // columns are padded to a multiple of this (four k steps of 32)
constexpr int kFixRing = 4;            // LDS ring slots, one k step (32 columns) each
constexpr int kFixSlot = 32768;        // 2 operands x 8 planes x 2 KB
constexpr int kFixOperand = 16384;
constexpr int kFixInfo = kFixRing * kFixSlot;      // per-tile row / column data after the ring (4 KB)
constexpr int kFixLds = kFixInfo + 4096;
constexpr int kFixLdsScreen = kFixLds + 1024;      // k_fgemm<FG_SCREEN>: two more arg-max exchange arrays after the info area

__host__ __device__ inline long fix_round_rows(long r) { return (r + kFixTile - 1) / kFixTile * kFixTile; }
__host__ __device__ inline int fix_round_cols(int d) { return (d + kFixColPad - 1) / kFixColPad * kFixColPad; }
// bytes of the planes / of the exponents of an R x D matrix
__host__ __device__ inline size_t fix_plane_bytes(long R, int D) { return (size_t)fix_round_rows(R) * fix_round_cols(D) * 4; }

// ------------------------------------------------------------------ rows -> limb planes
__device__ __forceinline__ int fix_q(float v, int e) {
    float s = ldexpf(v, 30 - e);
    s = fminf(fmaxf(s, -1073741824.0f), 1073741824.0f);
    return (int)rintf(s);
}

// Workgroup = RW rows (4 is what ships: one row per wave), wave w takes RW / 4 of them.  Pass 1: the row
// exponent (and, for frames, |x|^2 as the sum of squares of the path is formed: lane l adds the float4 groups l, l + 64,
// ... then the butterfly); rows of up to 1,024 columns stay in registers for pass 2.  Pass 2, per block of 512 columns:
// limbs to LDS as [plane][row][16 bytes], then runs of RW x 16 bytes (RW rows of one plane) to the planes.
// src: fp32 rows of `ld` floats (or fp16 rows of `ld` halves when xh), D valid columns; rows >= R are written as zeros.
// bias_src / bias_dst: optional copy of R floats riding along (the classifier's bias into `prepared`).
struct FixRowsArgs {
    const float *src;
    int xh;
    long R, Rp;
    int D;
    long ld;
    int Dq;
    int8_t *planes;
    int *exps;
    float *xx;
    const float *bias_src;
    float *bias_dst;
    // centering (oracle "CENTERING": every table of the search is formed from rows / frames with the codebook means taken
    // out): row r is written as src[r] - sub[(r / sub_per) * sub_ld] (one fp32 subtraction per element; sub_per == 0: every
    // row takes sub[0 .. D)); planes / exps / xx receive the CENTERED row.
    const float *sub;
    long sub_per, sub_ld;
    // optional: dot_out[r] = fixdot(row r, dot_vec[0 .. D)) -- the exact fixed-point product of the path, formed from the limbs this
    // kernel has in its registers anyway (the classifier rows against the data mean: what centering the frame takes out of a logit)
    const float *dot_vec;
    float *dot_out;
    unsigned *clear;      // optional: one word this launch sets to zero (the counter of the screened logits' recheck list)
};

template <int RW, bool DOT>      // DOT: also the rows' fixed-point products with a.dot_vec (the classifier rows of mcq_prepare)
__device__ __forceinline__ void fix_rows_body(const FixRowsArgs &a, unsigned bid) {
    const float *__restrict__ src = a.src;
    const int xh = a.xh, D = a.D, Dq = a.Dq;
    const long R = a.R, Rp = a.Rp, ld = a.ld;
    float *__restrict__ xx = a.xx;
    const float *__restrict__ bias_src = a.bias_src;
    float *__restrict__ bias_dst = a.bias_dst;
    const float *__restrict__ sub = a.sub;
    int8_t *__restrict__ planes = a.planes;
    constexpr int RPW = RW / 4;
    __shared__ __attribute__((aligned(16))) unsigned tile[128 * RW * 4];      // [plane of the block][row][4 words]
    __shared__ int es[RW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)bid * RW;
    if (bias_src && tid < RW && row0 + tid < R) bias_dst[row0 + tid] = bias_src[row0 + tid];
    if (a.clear && bid == 0 && tid == 0) *a.clear = 0u;
    const _Float16 *srch = reinterpret_cast<const _Float16 *>(src);
    const bool vec_ok = ((ld & 3) == 0) && ((D & 3) == 0) && ((reinterpret_cast<uintptr_t>(src) & (xh ? 7 : 15)) == 0);
    auto load4 = [&](long row, int q) -> f32x4 {      // float4 group q of a row, zero past D
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row >= R || 4 * q >= D) return v;
        if (vec_ok) return xh ? load_h4(srch + row * ld + 4 * q) : *reinterpret_cast<const f32x4 *>(src + row * ld + 4 * q);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * q + c < D) v[c] = xh ? (float)srch[row * ld + 4 * q + c] : src[row * ld + 4 * q + c];
        return v;
    };
    // group q of a D-vector (zeros past D): what is taken out of a row (`sub`; nothing for the padding rows, which stay zero rows)
    // or what the rows are multiplied with (`dot_vec`)
    auto vec4 = [&](const float *p, int q) -> f32x4 {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (4 * q >= D) return v;
        if (((D & 3) == 0) && ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) return *reinterpret_cast<const f32x4 *>(p + 4 * q);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * q + c < D) v[c] = p[4 * q + c];
        return v;
    };
    auto sub4 = [&](long row, int q) -> f32x4 {
        if (!sub || row >= R) return f32x4{0.f, 0.f, 0.f, 0.f};
        return vec4(sub + (a.sub_per ? (row / a.sub_per) * a.sub_ld : 0), q);
    };
    // the exponent of dot_vec (every wave forms it: max |.| over the vector)
    int ev = 0;
    if (DOT && a.dot_vec) {
        float mv = 0.f;
        for (int q = lane; q < (D + 3) / 4; q += 64) {
            const f32x4 v = vec4(a.dot_vec, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) mv = fmaxf(mv, fabsf(v[c]));
        }
        for (int s = 32; s >= 1; s >>= 1) mv = fmaxf(mv, __shfl_xor(mv, s, 64));
        const int be = (int)((__float_as_uint(mv) >> 23) & 0xff);
        ev = (be < 1 ? 1 : be) - 126;
    }
    const bool cached = (RW == 4) && D <= 1024;      // (16-row workgroups measured slower with the rows held, 0.126 vs 0.083 ms, and slower than 4-row ones either way)
    f32x4 cache[RW == 4 ? RPW : 1][4];
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const long row = row0 + RPW * wave + rr;
        float m = 0.f, pe = 0.f;
        if (cached) {
            // (the row and what is taken out of it are requested together, then subtracted: written as load - load per group the
            // compiler waited for each pair in turn, 61 -> 71 us per 65,536 frames)
            f32x4 raw[4], sv4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = load4(row, lane + 64 * j);
#pragma unroll
            for (int j = 0; j < 4; ++j) sv4[j] = sub4(row, lane + 64 * j);
#pragma unroll
            for (int j = 0; j < 4; ++j) cache[RW == 4 ? rr : 0][j] = sub ? raw[j] - sv4[j] : raw[j];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    m = fmaxf(m, fabsf(cache[RW == 4 ? rr : 0][j][c]));
                    pe = fmaf(cache[RW == 4 ? rr : 0][j][c], cache[RW == 4 ? rr : 0][j][c], pe);      // (groups past D are zeros: fmaf(0, 0, pe) == pe)
                }
        } else {
            for (int q = lane; q < (D + 3) / 4; q += 64) {
                const f32x4 raw = load4(row, q);
                const f32x4 v = sub ? raw - sub4(row, q) : raw;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    m = fmaxf(m, fabsf(v[c]));
                    pe = fmaf(v[c], v[c], pe);
                }
            }
        }
        for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
        if (xx) pe = wave_sum_butterfly(pe);
        if (lane == 0) {
            const int be = (int)((__float_as_uint(m) >> 23) & 0xff);
            const int e = (be < 1 ? 1 : be) - 126;
            es[RPW * wave + rr] = e;
            if (row < Rp) a.exps[row] = e;
            if (xx && row < R) xx[row] = pe;
        }
    }
    __syncthreads();
    int T[RPW][4];      // limb-product sums of the rows against dot_vec (oracle: fixdot), this lane's columns
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr)
#pragma unroll
        for (int i = 0; i < 4; ++i) T[rr][i] = 0;
    auto limbs4 = [&](const f32x4 &v, int e, unsigned (&w)[4]) {      // four columns -> one word per limb (most significant first)
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = 0u;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            int r = fix_q(v[c], e);
#pragma unroll
            for (int i = 3; i >= 1; --i) {
                const int l = (int)(int8_t)(r & 0xff);
                w[i] |= (unsigned)(l & 0xff) << (8 * c);
                r = (r - l) >> 8;
            }
            w[0] |= (unsigned)(r & 0xff) << (8 * c);
        }
    };
    for (int c0 = 0; c0 < Dq; c0 += 512) {
        const int ncol = (Dq - c0 < 512) ? Dq - c0 : 512;          // columns of this block (a multiple of 128)
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int rl = RPW * wave + rr;
            const int e = es[rl];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int q = lane + 64 * j;
                if (q >= ncol / 4) continue;
                f32x4 v;
                if (cached) v = cache[RW == 4 ? rr : 0][((c0 >> 9) * 2 + j) & 3];
                else v = sub ? load4(row0 + rl, c0 / 4 + q) - sub4(row0 + rl, c0 / 4 + q) : load4(row0 + rl, c0 / 4 + q);
                unsigned w[4];
                limbs4(v, e, w);
                if (DOT && a.dot_vec) {
                    unsigned mw[4];
                    limbs4(vec4(a.dot_vec, c0 / 4 + q), ev, mw);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int jj = 0; i + jj < 4; ++jj) T[rr][i + jj] = __builtin_amdgcn_sdot4((int)w[i], (int)mw[jj], T[rr][i + jj], false);
                }
                const int chunk = q >> 2, word = q & 3;
#pragma unroll
                for (int i = 0; i < 4; ++i) tile[((chunk * 4 + i) * RW + rl) * 4 + word] = w[i];
            }
        }
        __syncthreads();
        const int nplanes = ncol / 16 * 4;
        for (int p = tid / RW; p < nplanes; p += 256 / RW) {
            const int rl = tid % RW;
            if (row0 + rl < Rp) {
                const i32x4 v = *reinterpret_cast<const i32x4 *>(&tile[(p * RW + rl) * 4]);
                *reinterpret_cast<i32x4 *>(planes + (((long)(c0 / 16) * 4 + p) * Rp + row0 + rl) * 16) = v;
            }
        }
        __syncthreads();
    }
    if (DOT && a.dot_vec) {
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            int t4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int t = T[rr][i];
                for (int s = 32; s >= 1; s >>= 1) t += __shfl_xor(t, s, 64);      // exact integers: no order to speak of
                t4[i] = t;
            }
            const long row = row0 + RPW * wave + rr;
            if (lane == 0 && row < R) {
                float tt = (float)t4[3];
                tt = __builtin_fmaf((float)t4[2], 256.0f, tt);
                tt = __builtin_fmaf((float)t4[1], 65536.0f, tt);
                tt = __builtin_fmaf((float)t4[0], 16777216.0f, tt);
                a.dot_out[row] = ldexpf(tt, es[RPW * wave + rr] + ev - 36);
            }
        }
    }
}

template <int RW>
__global__ void __launch_bounds__(256) k_fix_rows(const FixRowsArgs a) { fix_rows_body<RW, false>(a, blockIdx.x); }

// two matrices in one launch (the centers and the classifier rows of mcq_prepare: one launch boundary less per trainer step)
template <int RW>
__global__ void __launch_bounds__(256) k_fix_rows2(const FixRowsArgs a, const FixRowsArgs b, unsigned blocks_a) {
    if (blockIdx.x < blocks_a) fix_rows_body<RW, false>(a, blockIdx.x);
    else fix_rows_body<RW, true>(b, blockIdx.x - blocks_a);
}

// ------------------------------------------------------------------ the GEMM
// out-of-kernel description of what the epilogue does with a tile of t values
// FG_SCREEN: the logits product for callers that want the ARG MAX only, from limbs 0-2 of both operands (six limb
// products, T_0 .. T_2); pairs whose winner the dropped class T_3 could change go to a list for k_fscreen_recheck
enum { FG_STORE = 0, FG_LOGITS = 1, FG_SCREEN = 2 };

struct FixGemm {
    const int8_t *A, *B;           // limb planes: A rows are the tile rows (M), B rows the tile columns (N)
    const int *ea, *eb;            // row exponents
    long RA, RB;                   // padded row counts (multiples of 128)
    long M, N;                     // valid rows / columns
    int Dq;                        // padded inner dimension
    int walk_rows;                 // 0: an XCD owns row tiles and walks the column tiles (A streams, B is the table);
                                   // 1: the other way round (B streams)
    // FG_STORE: out[row * ldo + col] = fixdot
    float *out;
    long ldo;
    // FG_LOGITS: rows are (codebook, entry) pairs, columns are frames; value = fixdot * lscale + bias[row];
    //            (value = (fixdot + wmu[row]) * lscale + bias[row]: see wmu)
    //            logits[col * ldo + row] = value when logits != nullptr; idx[col * ncb + codebook] = first arg max
    const float *bias;
    const float *wmu;              // fixdot(data mean, W[row]): the frames of this product are centered (x - mean), the logit is (t + wmu) * lscale + bias
    const float *lscale_ptr;       // device scalar, or nullptr: lscale
    float lscale;
    float *logits;
    void *idx;                     // uint8 [N cols][ncb], or uint16 when idx_wide (codebooks of more than 256 entries)
    int idx_wide;
    int K, ncb;
    // FG_SCREEN: the undecided (frame, codebook) pairs, two words each (col * ncb + codebook; the second's entry, bit 31: more than
    // two contenders), appended at atomicAdd(und_cnt, 1)
    unsigned *und_cnt, *und_list;
    unsigned und_cap;
};

__device__ __forceinline__ void fg_store_idx(const FixGemm &g, long pos, long entry) {
    if (g.idx_wide) static_cast<uint16_t *>(g.idx)[pos] = (uint16_t)entry;
    else static_cast<uint8_t *>(g.idx)[pos] = (uint8_t)entry;
}

// Persistent workgroups (one per CU: 132 KB of LDS): workgroup w takes the tiles w, w + grid, ... of an XCD-aware order and
// runs their k steps as ONE stream through the LDS ring -- the first steps of the next tile are in flight while this one
// finishes and stores.  EIGHT waves, two per SIMD, each a 64 x 32 corner of the 128 x 128 tile (2 MFMA tiles x 4 accumulator
// sets = 128 of its 256 registers).  A k step of a wave: 20 MFMAs against 12 ds_read_b128 (the fragments of the next step)
// and 4 LDS-DMA pieces of 1 KB (the step four ahead), dealt in four groups.  With one wave per SIMD (four waves of 64 x 64,
// the first version) a wave's DMA issue -- tens of cycles per piece in its in-order stream -- its fragment reads and its
// waits left the matrix pipe idle: 0.72-0.75 ms per product at 65,536 x 2,048 x 512; two waves cover each other: 0.58.
//
// vmcnt bookkeeping: a wave's pieces of stage s are requested in step s - 4; before the fragment reads of stage s + 1 (the
// sync of step s) it waits until only its pieces of the two later stages are outstanding (loads complete in the order they
// were issued; the stores and the few extra pieces of a tile boundary only make that count conservative), then the
// barrier makes every wave's pieces visible.  The row exponents and biases the epilogue needs reach LDS the same way (six
// 256-byte DMA pieces per tile, requested when the tile starts).  Measured and dropped: draining the queue before the
// epilogue's stores so that the next tile's first syncs need no count (0.566 against 0.549 ms).
template <int MODE>
__global__ void __launch_bounds__(512)
k_fgemm(const FixGemm g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // FG_SCREEN runs the same walk with limbs 0-2 only: NL pieces per wave and stage, NL accumulator sets, 6 limb pairs
    constexpr bool SCREEN = MODE == FG_SCREEN, LOGITS = MODE != FG_STORE;
    constexpr int NL = SCREEN ? 3 : 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;          // 64-row half, 32-column quarter of the tile
    const int r32 = lane & 31, kh = lane >> 5;
    const long MT = g.RA / kFixTile, NT = g.RB / kFixTile;
    // K = 256 logits: the two row tiles of a codebook are consecutive tiles of one workgroup (running arg max in registers)
    const int H = (LOGITS && g.K > kFixTile) ? g.K / kFixTile : 1;
    const long big = g.walk_rows ? NT : MT, small_units = (g.walk_rows ? MT : NT) / H;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
    auto tile_of = [&](long t, long &m0, long &n0) -> bool {      // t-th tile of this workgroup
        const long unit = t / H, half = t % H;
        const long idx = slot + unit * per_xcd;
        const long bt = (idx / small_units) * 8 + xcd, st = (idx % small_units) * H + half;
        m0 = (g.walk_rows ? st : bt) * kFixTile;
        n0 = (g.walk_rows ? bt : st) * kFixTile;
        return bt < big;
    };
    i32x16 acc[2][NL];
    const int nst = g.Dq / 32;
    // this wave's 4 pieces of a stage (1 KB each): waves 0..3 bring operand A, 4..7 operand B; bit 1 of the wave picks the
    // 16-column chunk, bit 0 the 64-row half, g4 = 0..3 the limb plane
    const int wu = __builtin_amdgcn_readfirstlane(wave);
    const int op = wu >> 2, chunk = (wu >> 1) & 1, half = wu & 1;
    const long R = op ? g.RB : g.RA;
    const long pl = R * 16, sstride = 8 * R * 16;
    const unsigned dbase = (unsigned)(size_t)smem + op * kFixOperand + (4 * chunk) * 2048 + half * 1024;
    const unsigned voff = lane * 16, voff4 = lane * 4;
    auto base_of = [&](long m0, long n0) { return (op ? g.B + n0 * 16 : g.A + m0 * 16) + (long)(4 * chunk) * R * 16 + half * 1024; };
    // (m0 is written without being declared clobbered -- the compiler rejects it as a reserved register; nothing else in
    // this kernel uses m0: LDS instructions need no m0 on gfx9+, and the kernel has no LDS-DMA builtin, movrel or GWS)
    auto issue1 = [&](const int8_t *p, int st, int g4) {
        const int8_t *pg = p + g4 * pl;
        const unsigned d = dbase + (st % kFixRing) * kFixSlot + g4 * 2048;
        asm volatile(
            "s_mov_b32 m0, %[d]\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %[vo], %[p]\n\t"
            :
            : [vo] "v"(voff), [p] "s"(pg), [d] "s"(d)
            : "memory");
    };
    // the tile's row exponents ea (waves 0, 1), column exponents eb (2, 3) and, for the logits, row biases (4, 5) and the rows'
    // products with the data mean (6, 7) -> info: 64 words per piece; [0..127] ea, [128..255] eb, [256..383] bias, [384..639]
    // arg-max exchange, [640..767] wmu.  (Rows past M read whatever follows the bias / wmu inside `prepared`: they never reach an
    // output.)
    auto issue_info = [&](long m0, long n0) {
        if (wu < (LOGITS ? 8 : 4)) {
            const void *src = wu < 2 ? static_cast<const void *>(g.ea + m0 + 64 * wu)
                                     : (wu < 4 ? static_cast<const void *>(g.eb + n0 + 64 * (wu - 2))
                                               : (wu < 6 ? static_cast<const void *>(g.bias + m0 + 64 * (wu - 4))
                                                         : static_cast<const void *>(g.wmu + m0 + 64 * (wu - 6))));
            const unsigned d = (unsigned)(size_t)smem + kFixInfo + 256 * (wu < 6 ? wu : wu + 4);
            asm volatile(
                "s_mov_b32 m0, %[d]\n\ts_nop 0\n\t"
                "global_load_lds_dword %[vo], %[p]\n\t"
                :
                : [vo] "v"(voff4), [p] "s"(src), [d] "s"(d)
                : "memory");
        }
    };
    long m0, n0, m0n = 0, n0n = 0;
    if (!tile_of(0, m0, n0)) return;
    const int8_t *pcur = base_of(m0, n0), *pnext = pcur;
    auto step = [&](int st, const i32x4 (&a)[2][NL], const i32x4 (&b)[NL], i32x4 (&an)[2][NL], i32x4 (&bn)[NL]) {
        const char *base = smem + ((st + 1) % kFixRing) * kFixSlot;
        // (after the last tile the stage four ahead does not exist: the pieces are requested all the same, from the start of
        // the current tile (pnext == pcur then) into a slot nobody reads any more -- no branch round the DMA)
        const int8_t *p = (st + 4 < nst) ? pcur + (st + 4) * sstride : pnext + (st + 4 - nst) * sstride;
        constexpr int PI[10] = {0, 0, 1, 0, 1, 2, 0, 1, 2, 3};      // limb pairs (i, j), i + j <= 3, dealt 3, 3, 2, 2
        constexpr int PJ[10] = {0, 1, 0, 2, 1, 0, 3, 2, 1, 0};
        // (FG_SCREEN: the first six pairs, i + j <= 2, dealt 2, 2, 2 -- every pair of a group has its limbs read by then)
        constexpr int LO[5] = {0, SCREEN ? 2 : 3, SCREEN ? 4 : 6, SCREEN ? 6 : 8, 10};
#pragma unroll
        for (int g4 = 0; g4 < NL; ++g4) {
            issue1(p, st, g4);
#pragma unroll
            for (int t = 0; t < 2; ++t)
                an[t][g4] = *reinterpret_cast<const i32x4 *>(base + (kh * 4 + g4) * 2048 + (64 * wm + 32 * t + r32) * 16);
            bn[g4] = *reinterpret_cast<const i32x4 *>(base + kFixOperand + (kh * 4 + g4) * 2048 + (32 * wn + r32) * 16);
#pragma unroll
            for (int q = LO[g4]; q < LO[g4 + 1]; ++q)
#pragma unroll
                for (int ta = 0; ta < 2; ++ta)
                    acc[ta][PI[q] + PJ[q]] =
                        __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ta][PI[q]], b[PJ[q]], acc[ta][PI[q] + PJ[q]], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);      // (everything requested up front instead: 0.59 against 0.53 ms)
        }
    };
    i32x4 a0[2][NL], b0[NL], a1[2][NL], b1[NL];
    issue_info(m0, n0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int g4 = 0; g4 < NL; ++g4) issue1(pcur + q * sstride, q, g4);
    // stage 0 has landed when only the NL pieces of each of the three later stages are outstanding
    if constexpr (SCREEN) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int l = 0; l < NL; ++l) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
            a0[t][l] = *reinterpret_cast<const i32x4 *>(smem + (kh * 4 + l) * 2048 + (64 * wm + 32 * t + r32) * 16);
        b0[l] = *reinterpret_cast<const i32x4 *>(smem + kFixOperand + (kh * 4 + l) * 2048 + (32 * wn + r32) * 16);
    }
    int *info = reinterpret_cast<int *>(smem + kFixInfo);
    float *infof = reinterpret_cast<float *>(smem + kFixInfo);
    // running arg max of a codebook that spans several row tiles: per lane, its column
    float runv = 0.f;
    int runk = 0;
    float runs = 0.f, runt = 0.f, runq = 0.f;      // FG_SCREEN: the running second / third value, magnitude, second's row and
    int runj = 0, rune = 0;                        // largest row exponent (see the epilogue)
    for (long t = 0;; ++t) {
        const bool has_next = tile_of(t + 1, m0n, n0n);
        pnext = has_next ? base_of(m0n, n0n) : pcur;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int s = 0; s < NL; ++s)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[a][s][v] = 0;
        // before the reads of stage st + 1: it has landed everywhere and every wave has left slot st % ring.  Two later
        // stages stay in flight: 2 * NL pieces of this wave
        for (int st = 0; st < nst; st += 2) {
            if constexpr (SCREEN) asm volatile("s_waitcnt vmcnt(6)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            step(st, a0, b0, a1, b1);
            if constexpr (SCREEN) asm volatile("s_waitcnt vmcnt(6)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            step(st + 1, a1, b1, a0, b0);      // (reads past the end of the last tile hit a slot nobody uses)
        }
        // ---- epilogue.  The info words of this tile landed during its first steps (requested at its start, made visible by
        // the step barriers)
        auto value = [&](int ta, int v, int e) -> float {
            float tt;
            if constexpr (SCREEN) tt = __fmul_rn((float)acc[ta][2][v], 256.0f);      // t' of the six products (exact: a power of two)
            else tt = __builtin_fmaf((float)acc[ta][2][v], 256.0f, (float)acc[ta][NL - 1][v]);
            tt = __builtin_fmaf((float)acc[ta][1][v], 65536.0f, tt);
            tt = __builtin_fmaf((float)acc[ta][0][v], 16777216.0f, tt);
            return ldexpf(tt, e);
        };
        // lane-dependent offsets are formed anew for every tile (hoisted out of the tile loop they would cost registers)
        int rbase = 64 * wm + 4 * kh, cbase = 32 * wn + r32;
        asm volatile("" : "+v"(rbase), "+v"(cbase));
        // the exponents (and biases) of this lane's 32 rows: eight 16-byte LDS reads up front
        i32x4 er[2][4];
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
            for (int q = 0; q < 4; ++q) er[ta][q] = *reinterpret_cast<const i32x4 *>(&info[rbase + 32 * ta + 8 * q]);
        const bool full = (m0 + kFixTile <= g.M) && (n0 + kFixTile <= g.N);      // whole tile inside: no per-element guards
        const int ecol = info[128 + cbase] - 36;
        const int rows_left = (int)((g.M - m0 - rbase) > 128 ? 128 : (g.M - m0 - rbase));
        if (MODE == FG_STORE) {
            const bool col_ok = n0 + cbase < g.N;
            float *orow = g.out + (m0 + rbase) * g.ldo + n0 + cbase;
            if (full) {
#pragma unroll
                for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int ro = 32 * ta + 8 * (v >> 2) + (v & 3);          // row of the lane's block
                        orow[(long)ro * g.ldo] = value(ta, v, er[ta][v >> 2][v & 3] + ecol);
                    }
            } else {
#pragma unroll
                for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int ro = 32 * ta + 8 * (v >> 2) + (v & 3);
                        const float val = value(ta, v, er[ta][v >> 2][v & 3] + ecol);
                        if (col_ok && ro < rows_left) orow[(long)ro * g.ldo] = val;
                    }
            }
        } else if constexpr (SCREEN) {
            // The screened logit of a row is the chain of FG_LOGITS applied to t' (limbs 0-2) instead of t (all ten products):
            //     y = ldexp(t, e)   s1 = fl(y + wmu)   s2 = fl(s1 * ls)   L = fl(s2 + bias)        (y', s1', s2', L' from t')
            // The winner of (frame, codebook) is DECIDED when best' - second' > margin, where margin >= 2 max_r |L_r - L'_r|:
            // then L_b - L_r >= (L'_b - L'_r) - |L_b - L'_b| - |L_r - L'_r| > 0 for every other row r, so the exact first arg max is b.
            // Everything else (equal screened values included: their difference is 0) goes to the list of k_fscreen_recheck.
            //
            // Bound of |L - L'| for one row.  u = 2^-24, A = 128 * 128 * Dq (Dq columns of limb products, |limb| <= 128), so
            // |T_s| <= (s + 1) A.  Both chains convert the SAME integers T_0, T_1, T_2 to the same floats c_0, c_1, c_2
            // (|c_s| <= (s + 1) A (1 + u)); they differ in
            //     exact:     r3 = fl(T_3)   r2 = fl(c_2 2^8 + r3)   r1 = fl(c_1 2^16 + r2)    t  = fl(c_0 2^24 + r1)
            //     screened:                 r2' = c_2 2^8 (exact)   r1' = fl(c_1 2^16 + r2')  t' = fl(c_0 2^24 + r1')
            // (a) |r3| <= 4 A (1 + u); |r2 - r2'| <= |r3| + u |c_2 2^8 + r3| <= A (1 + u) (4 + 772 u).
            // (b) |r1 - r1'| <= |r2 - r2'| + u (|c_1 2^16 + r2| + |c_1 2^16 + r2'|) <= A (4 + 2^-5).
            // (c) |t - t'| <= |r1 - r1'| + u (|t| + |t'|) / (1 - u), and |t| <= |t'| + |t - t'|, hence
            //     |t - t'| <= 4.0625 A + 2^-22 |t'|;  |t'| <= 2^24 A (1 + 2^-7 + 2^-14) (1 + u)^4, so |t - t'| <= 8.1 A =: dt.
            // (d) ldexp is exact (a result in the subnormal range is rounded by at most 2^-150: the constant added last covers
            //     it), so |y - y'| <= d = dt 2^e, e = ea[row] + eb[col] - 36.  Rounding to nearest is monotone and moves a value
            //     x by at most u |x|; for reals p, p' that gives |fl(p) - fl(p')| <= |p - p'| (1 + u) + 2 u |fl(p')| / (1 - u).
            //     Applied three times (ls > 0 scales a difference by ls):
            //     |L - L'| <= (1 + u)^3 ls d + 2 u (1 + u)^2 / (1 - u)^2 (ls |s1'| + |s2'| + |L'|),  ls |s1'| <= |s2'| / (1 - u)
            //             <= 1.000001 ls d + 2^-22 * 3 max(|s2'|, |L'|).
            // margin = 16.5 A 2^e ls + 2^-19 q + 2^-120, with e from the LARGEST row exponent of the tile(s) of the codebook and q the
            // largest max(|s2'|, |L'|) among the rows this merge path has seen for the frame (a superset of the codebook's rows):
            // 16.5 > 2 * 8.1 * 1.000001 and 2^-19 > 2 * 3 * 2^-22 leave 1.8 % and 25 % for the few fp32 roundings in forming the
            // margin and the difference.  An infinite or NaN margin or difference fails the test and lists the pair.
            const float ls = g.lscale_ptr ? *g.lscale_ptr : g.lscale;
            // An undecided pair whose THIRD-best screened value is below best' - margin has two contenders only (every row whose
            // exact logit can reach the winner's has L' >= best' - margin): the list carries the second's row, and the recheck
            // forms two exact logits instead of K.  Which of two equal screened values counts as the better one is immaterial
            // here: a decided pair has best' > second', an undecided one is settled by exact values (lower row on equal ones).
            float bv[4], sv[4], tv[4], qm = 0.f;   // best / second / third value of the 16-row group, this lane's 8 rows of it
            int bk[4], sk[4];                      // rows of the best and the second
            const long col = n0 + cbase;
#pragma unroll
            for (int ta = 0; ta < 2; ++ta) {
#pragma unroll
                for (int v4 = 0; v4 < 4; ++v4) {
                    const f32x4 br4 = *reinterpret_cast<const f32x4 *>(&infof[256 + rbase + 32 * ta + 8 * v4]);
                    const f32x4 wm4 = *reinterpret_cast<const f32x4 *>(&infof[640 + rbase + 32 * ta + 8 * v4]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int v = 4 * v4 + c;
                        const int rl = rbase + 32 * ta + 8 * v4 + c;
                        const float s2 = __fmul_rn(__fadd_rn(value(ta, v, er[ta][v4][c] + ecol), wm4[c]), ls);
                        const float val = __fadd_rn(s2, br4[c]);
                        qm = fmaxf(qm, fmaxf(fabsf(s2), fabsf(val)));
                        const int gi = 2 * ta + (v4 >> 1);
                        if ((v4 & 1) == 0 && c == 0) { bv[gi] = val; bk[gi] = sk[gi] = rl; sv[gi] = tv[gi] = -INFINITY; }
                        else {
                            const bool c1 = val > bv[gi], c2 = val > sv[gi];
                            tv[gi] = __builtin_amdgcn_fmed3f(tv[gi], sv[gi], val);      // (tv <= sv <= bv: the middle one is the new third,
                            sv[gi] = __builtin_amdgcn_fmed3f(sv[gi], bv[gi], val);      //  the new second)
                            sk[gi] = c1 ? bk[gi] : (c2 ? rl : sk[gi]);
                            bk[gi] = c1 ? rl : bk[gi];
                            bv[gi] = fmaxf(bv[gi], val);
                        }
                    }
                }
            }
            // the largest row exponent of this tile (every wave forms it)
            int em = info[lane] > info[lane + 64] ? info[lane] : info[lane + 64];
            for (int s = 32; s >= 1; s >>= 1) { const int o = __shfl_xor(em, s, 64); em = o > em ? o : em; }
            // the three largest values (and the rows of two) of the union of two disjoint sets of rows, each given by its own three
            auto merge = [](float &b1, int &k1, float &s1, int &j1, float &t1, float b2, int k2, float s2, int j2, float t2) {
                if (b2 > b1) {      // the set with the larger best first
                    float f = b1; b1 = b2; b2 = f;
                    f = s1; s1 = s2; s2 = f;
                    t1 = t2;        // (the other set's third is below its second: it cannot be among the union's three)
                    int i = k1; k1 = k2; k2 = i;
                    j1 = j2;
                }
                if (b2 > s1) { t1 = fmaxf(s1, s2); s1 = b2; j1 = k2; }      // b1 >= b2 > s1
                else t1 = fmaxf(t1, b2);                                   // b1 >= s1 >= b2
            };
            const float cA = 16.5f * 16384.0f * (float)g.Dq;
            auto undecided = [&](float v, float s, float q, int e) {
                const float margin = __fadd_rn(__fadd_rn(__fmul_rn(ldexpf(cA, e + ecol), ls), __fmul_rn(q, 1.9073486328125e-6f)), 7.5231638452626401e-37f);
                return !(__fsub_rn(v, s) > margin);
            };
            // a list entry: the pair and the second's entry of the codebook, bit 31 set when more than two rows contend
            auto append = [&](long pos, unsigned second_entry, bool many) {
                const unsigned at = atomicAdd(g.und_cnt, 1u);
                if (at < g.und_cap) {
                    g.und_list[2 * (size_t)at] = (unsigned)pos;
                    g.und_list[2 * (size_t)at + 1] = second_entry | (many ? 0x80000000u : 0u);
                }
            };
            const int K = g.K;
#pragma unroll
            for (int gi = 0; gi < 4; ++gi)
                merge(bv[gi], bk[gi], sv[gi], sk[gi], tv[gi], __shfl_xor(bv[gi], 32, 64), __shfl_xor(bk[gi], 32, 64),
                      __shfl_xor(sv[gi], 32, 64), __shfl_xor(sk[gi], 32, 64), __shfl_xor(tv[gi], 32, 64));
            qm = fmaxf(qm, __shfl_xor(qm, 32, 64));
            if (K >= 32) {
                merge(bv[0], bk[0], sv[0], sk[0], tv[0], bv[1], bk[1], sv[1], sk[1], tv[1]);
                merge(bv[2], bk[2], sv[2], sk[2], tv[2], bv[3], bk[3], sv[3], sk[3], tv[3]);
            }
            if (K >= 64) merge(bv[0], bk[0], sv[0], sk[0], tv[0], bv[2], bk[2], sv[2], sk[2], tv[2]);
            if (K <= 64) {
                if (kh == 0) {
                    const int span = K / 16;
#pragma unroll
                    for (int gi = 0; gi < 4; ++gi) {
                        const long row = m0 + bk[gi];
                        if ((gi % span) == 0 && col < g.N && row < g.M) {
                            fg_store_idx(g, col * g.ncb + row / K, row % K);
                            if (undecided(bv[gi], sv[gi], qm, em))
                                append(col * g.ncb + row / K, (unsigned)((m0 + sk[gi]) % K), undecided(bv[gi], tv[gi], qm, em));
                        }
                    }
                }
            } else {
                // (words 768 .. 1023 of the info area, where no DMA piece lands, and the kilobyte after it)
                float *exv = infof + 384, *exs = infof + 768, *exq = infof + 896;
                int *exk = info + 384 + 128;
                float *ext = reinterpret_cast<float *>(smem + kFixInfo + 4096);
                int *exj = reinterpret_cast<int *>(smem + kFixInfo + 4096 + 512);
                if (wm == 1 && kh == 0) {
                    exv[cbase] = bv[0]; exk[cbase] = bk[0]; exs[cbase] = sv[0]; exq[cbase] = qm;
                    ext[cbase] = tv[0]; exj[cbase] = sk[0];
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (wm == 0 && kh == 0) {
                    const int hf = (int)(t % H);
                    float v = bv[0], s = sv[0], t3 = tv[0], q = fmaxf(qm, exq[cbase]);
                    int kk = bk[0], jj = sk[0];
                    merge(v, kk, s, jj, t3, exv[cbase], exk[cbase], exs[cbase], exj[cbase], ext[cbase]);
                    kk += (int)m0;      // rows of the whole matrix from here on
                    jj += (int)m0;
                    if (hf > 0) {
                        merge(v, kk, s, jj, t3, runv, runk, runs, runj, runt);
                        q = fmaxf(q, runq);
                        em = em > rune ? em : rune;
                    }
                    runv = v; runk = kk; runs = s; runj = jj; runt = t3; runq = q; rune = em;
                    const long k = kk;
                    if (hf == H - 1 && col < g.N && k < g.M) {
                        fg_store_idx(g, col * g.ncb + k / K, k % K);
                        if (undecided(v, s, q, em)) append(col * g.ncb + k / K, (unsigned)(jj % K), undecided(v, t3, q, em));
                    }
                }
            }
        } else {
            const float ls = g.lscale_ptr ? *g.lscale_ptr : g.lscale;
            // per lane: one column (frame), rows 64 wm + 32 ta + 8 (v >> 2) + 4 kh + (v & 3), ascending in (ta, v)
            float bv[4];          // best of the 16-row group (ta, v >> 3), this lane's 8 rows of it
            int bk[4];
            const long col = n0 + cbase;
            float *lrow = g.logits ? g.logits + col * g.ldo + m0 + rbase : nullptr;
            // the two 32-row halves one after the other, each with its own biases / mean products read where they are used: with
            // all 32 rows' worth held from the top of the epilogue (32 + 32 registers beside the 128 accumulators, the next
            // tile's first fragments and the exponents) the kernel ran out of its 256 registers (24 spilled, 0.56 -> 0.74 ms)
#pragma unroll
            for (int ta = 0; ta < 2; ++ta) {
#pragma unroll
                for (int v4 = 0; v4 < 4; ++v4) {
                    const f32x4 br4 = *reinterpret_cast<const f32x4 *>(&infof[256 + rbase + 32 * ta + 8 * v4]);
                    const f32x4 wm4 = *reinterpret_cast<const f32x4 *>(&infof[640 + rbase + 32 * ta + 8 * v4]);
                    f32x4 q4;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int v = 4 * v4 + c;
                        const int rl = rbase + 32 * ta + 8 * v4 + c;
                        const float val = __fadd_rn(__fmul_rn(__fadd_rn(value(ta, v, er[ta][v4][c] + ecol), wm4[c]), ls), br4[c]);
                        q4[c] = val;
                        const int gi = 2 * ta + (v4 >> 1);
                        if ((v4 & 1) == 0 && c == 0) { bv[gi] = val; bk[gi] = rl; }
                        else if (val > bv[gi]) { bv[gi] = val; bk[gi] = rl; }
                    }
                    if (lrow && (full || (col < g.N && 32 * ta + 8 * v4 < rows_left)))
                        *reinterpret_cast<f32x4 *>(lrow + 32 * ta + 8 * v4) = q4;
                }
            }
            if (g.idx) {
                // a value beats another when it is larger, or equal with the lower row
                auto better = [](float v1, int k1, float v2, int k2) { return (v1 > v2) | ((v1 == v2) & (k1 < k2)); };
                const int K = g.K;
                // the other half-wave holds the other 8 rows of every 16-row group
#pragma unroll
                for (int gi = 0; gi < 4; ++gi) {
                    const float ov = __shfl_xor(bv[gi], 32, 64);
                    const int ok = __shfl_xor(bk[gi], 32, 64);
                    if (better(ov, ok, bv[gi], bk[gi])) { bv[gi] = ov; bk[gi] = ok; }
                }
                // groups of 16 rows -> codebooks of K rows inside this wave's 64 rows (the later group wins only with a
                // strictly larger value)
                if (K >= 32) {
                    if (bv[1] > bv[0]) { bv[0] = bv[1]; bk[0] = bk[1]; }
                    if (bv[3] > bv[2]) { bv[2] = bv[3]; bk[2] = bk[3]; }
                }
                if (K >= 64 && bv[2] > bv[0]) { bv[0] = bv[2]; bk[0] = bk[2]; }
                if (K <= 64) {
                    if (kh == 0) {
                        const int span = K / 16;
#pragma unroll
                        for (int gi = 0; gi < 4; ++gi) {
                            const long row = m0 + bk[gi];
                            if ((gi % span) == 0 && col < g.N && row < g.M) fg_store_idx(g, col * g.ncb + row / K, row % K);
                        }
                    }
                } else {
                    // K = 128: the two waves of a column meet in LDS; K = 256: and the two row tiles in registers
                    float *exv = infof + 384;
                    int *exk = info + 384 + 128;
                    if (wm == 1 && kh == 0) { exv[cbase] = bv[0]; exk[cbase] = bk[0]; }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    if (wm == 0 && kh == 0) {
                        const int hf = (int)(t % H);
                        float v = bv[0];
                        long k = m0 + bk[0];
                        if (better(exv[cbase], exk[cbase], bv[0], bk[0])) { v = exv[cbase]; k = m0 + exk[cbase]; }
                        if (hf > 0 && !(v > runv)) { v = runv; k = runk; }      // earlier rows win ties
                        runv = v;
                        runk = (int)k;
                        if (hf == H - 1 && col < g.N && k < g.M) fg_store_idx(g, col * g.ncb + k / K, k % K);
                    }
                }
            }
        }
        if (!has_next) break;
        // the info words are rewritten for the next tile: every wave must have read them (and every wave has waited for its
        // pieces: the next tile's first stages have landed everywhere)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        m0 = m0n;
        n0 = n0n;
        pcur = pnext;
        issue_info(m0, n0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the pieces still on their way to this workgroup's LDS
}

// ------------------------------------------------------------------ the exact recheck of the screened arg max
// The pairs k_fgemm<FG_SCREEN> could not decide: a wave per listed (frame, codebook) recomputes the logits of the contenders from
// the full ten limb products (integer dot products of the limb planes, the same three fmas and the same chain as the FG_LOGITS
// epilogue) and overwrites the code with the first arg max.  Two contenders (the screened winner, whose entry is the code
// already written, and the second the list names): half a wave per row, a lane per 16-column chunk.  More than two: all K
// rows, a lane per row (K * Dq * 4 bytes of planes per pair: rare by construction, slow when it is not).  A fixed grid strides
// over the list; the count is read on the device.
struct FixRecheck {
    const int8_t *W, *X;           // limb planes of the classifier rows / of the frames
    const int *ew, *ex;
    long RW, RX;                   // padded row counts
    int Dq;
    const float *bias, *wmu, *lscale_ptr;
    float lscale;
    void *idx;
    int idx_wide;
    int K, ncb;
    const unsigned *cnt, *list;
    unsigned cap;
};

__global__ void __launch_bounds__(256) k_fscreen_recheck(const FixRecheck a) {
    const int lane = threadIdx.x & 63;
    const unsigned wv = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), nwv = gridDim.x * 4;
    unsigned n = *a.cnt;
    n = n < a.cap ? n : a.cap;
    const float ls = a.lscale_ptr ? *a.lscale_ptr : a.lscale;
    const int K = a.K, nch = a.Dq / 16;
    for (unsigned i = wv; i < n; i += nwv) {
        const unsigned pos = a.list[2 * (size_t)i], snd = a.list[2 * (size_t)i + 1];
        const long col = pos / (unsigned)a.ncb;
        const int cb = (int)(pos % (unsigned)a.ncb);
        const int ecol = a.ex[col] - 36;
        auto chunk = [&](int (&T)[4], int c, long row) {      // the ten limb products of one 16-column chunk
            i32x4 xl[4], wl[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                xl[l] = *reinterpret_cast<const i32x4 *>(a.X + (((long)c * 4 + l) * a.RX + col) * 16);
                wl[l] = *reinterpret_cast<const i32x4 *>(a.W + (((long)c * 4 + l) * a.RW + row) * 16);
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; p + q < 4; ++q)
#pragma unroll
                    for (int d = 0; d < 4; ++d) T[p + q] = __builtin_amdgcn_sdot4(wl[p][d], xl[q][d], T[p + q], false);
        };
        auto logit = [&](const int (&T)[4], long row) -> float {
            float tt = (float)T[3];
            tt = __builtin_fmaf((float)T[2], 256.0f, tt);
            tt = __builtin_fmaf((float)T[1], 65536.0f, tt);
            tt = __builtin_fmaf((float)T[0], 16777216.0f, tt);
            return __fadd_rn(__fmul_rn(__fadd_rn(ldexpf(tt, a.ew[row] + ecol), a.wmu[row]), ls), a.bias[row]);
        };
        float bv = -INFINITY;
        int bk = 0x7fffffff;
        if ((snd & 0x80000000u) == 0) {
            const int first = a.idx_wide ? (int)static_cast<const uint16_t *>(a.idx)[pos] : (int)static_cast<const uint8_t *>(a.idx)[pos];
            const int j = (lane < 32) ? first : (int)snd;
            const long row = (long)cb * K + j;
            int T[4] = {0, 0, 0, 0};
            for (int c = lane & 31; c < nch; c += 32) chunk(T, c, row);
#pragma unroll
            for (int p = 0; p < 4; ++p)
                for (int sft = 16; sft >= 1; sft >>= 1) T[p] += __shfl_xor(T[p], sft, 64);      // exact integers, within each half
            bv = logit(T, row);
            bk = j;
        } else {
            for (int j = lane; j < K; j += 64) {      // ascending rows per lane: a later one wins only with a larger value
                const long row = (long)cb * K + j;
                int T[4] = {0, 0, 0, 0};
                // (four chunks' loads in flight: one such pair among thousands of two-row ones is the launch's critical path, and a
                // chunk at a time it took 60 us)
#pragma unroll 4
                for (int c = 0; c < nch; ++c) chunk(T, c, row);
                const float val = logit(T, row);
                if (j == lane || val > bv) { bv = val; bk = j; }
            }
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const float ov = __shfl_xor(bv, s, 64);
            const int ok = __shfl_xor(bk, s, 64);
            if ((ov > bv) | ((ov == bv) & (ok < bk))) { bv = ov; bk = ok; }
        }
        if (lane == 0) {
            if (a.idx_wide) static_cast<uint16_t *>(a.idx)[pos] = (uint16_t)bk;
            else static_cast<uint8_t *>(a.idx)[pos] = (uint8_t)bk;
        }
    }
}

}  // namespace mcq
