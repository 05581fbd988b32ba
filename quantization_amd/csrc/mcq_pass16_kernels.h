// mcq_pass16_kernels.h -- the refinement passes of 16 (or 8) codebooks of 16 entries (QuantizerTrainer's first phase at 8 (4) bytes per
// frame, /root/reference/quantization/quantization.py:308-547 at K = 16) with the GRAM MATRIX RESIDENT IN LDS.  (Described for N = 16; with
// 8 codebooks there are 28 blocks, two workgroups per CU and one combine level less.)
//
// This is the one shape where "codebooks staged once in LDS" (BASELINE.json north_star) is literally possible for the table form:
// G is 256 x 256, symmetric bit for bit, and a pass never reads a same-codebook entry off the diagonal, so the 120 blocks
// (n, m), n < m, of 16 x 16 floats -- 122,880 bytes -- plus the diagonal (E / R) hold everything a pass reads.  One persistent
// workgroup of eight waves per CU fills them by LDS-DMA; each WAVE then carries one vector at a time through ALL passes of the
// call -- E / R, stage 0, the four combine levels, the winner's walk -- with every Gram read a ds_read, the candidate lists in 4 KB
// of wave-private LDS, the indexes in registers between passes: one launch per call instead of five per pass, no list traffic
// through global memory, no dependent L2 round trips (the separate kernels' waves live 3.6 us at 4,096 vectors, nearly all of it
// waiting for L2-hit gathers and for the lists the launch before wrote).
//
// Same arithmetic as the separate kernels, expression for expression (oracle/mcq_oracle.c, "TABLE FORM"): the sums of stage 0
// in ascending m, the leaf ((g - u) - v) + w, the group tables ((t00 + t01) + t10) + t11 (formed one child table at a time, the
// partial sums in registers in exactly that order), the scores ((Sx + Sy) - E) + 2 T, the shortlists as sets in ascending
// position, E / R of tf_er_wave.  tests/test_gpu_parity.py runs it against the oracle on every fixture of this shape;
// tests/test_gpu_pass16_lists.py compares the lists of every level, E, R and the early exit pass by pass (k_tf_pass16_probe below).
#pragma once
#include "mcq_tf_kernels.h"

namespace mcq {

struct Pass16Args {
    const float *G;        // [256][256] Gram matrix of the centered scaled centers
    const float *XC;       // [B][256]   x . C products of the call
    const float *xx;       // [B]        |x - mean|^2
    const float *Q;        // [256]      |C - mean|^2
    uint8_t *idx;          // [B][16]    indexes, refined in place
    long B;
    int iters;
    int64_t *out_i64;      // optional: the result as int64 [B][16]
    uint8_t *out_u8;       // optional: the result as bytes [B][16]
};

constexpr int kP16Waves = 8;
template <int N> constexpr int p16_blocks() { return N * (N - 1) / 2; }                           // codebook pairs n < m
template <int N> constexpr int p16_gram_floats() { return p16_blocks<N>() * 256 + 2 * N * 16; }   // blocks, diagonal, Q
// wave-private scratch (byte offsets)
constexpr int kP16Ent0 = 0;          // u8  [16][8]     level-0 lists: entries
constexpr int kP16Pos1 = 128;        // u8  [8][8][2]   level-1 lists: positions in the halves' lists
constexpr int kP16Pos2 = 256;        // u8  [4][16][2]
constexpr int kP16Pos3 = 384;        // u8  [2][16][2]
constexpr int kP16S0 = 512;          // f32 [16][8]
constexpr int kP16S1 = 1024;         // f32 [8][8]
constexpr int kP16S2 = 1280;         // f32 [4][16]
constexpr int kP16S3 = 1536;         // f32 [2][16]
constexpr int kP16T1 = 1664;         // f32 [8][9]      one level-1 table at a time (rows of 9: odd stride)
constexpr int kP16T2 = 1952;         // f32 [16][17]    one level-2 table at a time
constexpr int kP16Sel = 3040;        // u64 [128]       selection scratch
constexpr int kP16Scratch = 4096;
// one record of k_tf_pass16_probe (byte offsets): the list part of the scratch as it lies, then what the pass held in registers
constexpr int kP16Lists = kP16T1;    // bytes [0, kP16Lists) of the scratch: ent0, pos1 .. pos3, S0 .. S3
constexpr int kP16RecE = kP16Lists;            // f32          E
constexpr int kP16RecR = kP16RecE + 4;         // f32 [16]     R[n], n < N
constexpr int kP16RecIdx = kP16RecR + 64;      // u8  [16]     the new indexes, n < N
constexpr int kP16RecMark = kP16RecIdx + 16;   // u32          kP16RecWritten
constexpr int kP16Rec = kP16RecMark + 4;
constexpr uint32_t kP16RecWritten = 0x36315021u;
// the arrays of a record in the order mcq_test_pass16_layout reports them: offset, and the bytes N codebooks use of it
constexpr int kP16RecArrays = 12;
constexpr int kP16RecOff[kP16RecArrays] = {kP16Ent0, kP16Pos1, kP16Pos2, kP16Pos3, kP16S0, kP16S1, kP16S2, kP16S3,
                                           kP16RecE, kP16RecR, kP16RecIdx, kP16RecMark};
constexpr int p16_rec_bytes(int N, int a) {     // lists of 8 at levels 0 and 1, of 16 above; the last combine keeps no list
    const int levels = N == 16 ? 4 : 3;
    switch (a) {
    case 0: return N * 8;
    case 1: case 2: case 3: return a < levels ? (N >> a) * (a == 1 ? 8 : 16) * 2 : 0;
    case 4: return N * 8 * 4;
    case 5: case 6: case 7: return a - 4 < levels ? (N >> (a - 4)) * (a == 5 ? 8 : 16) * 4 : 0;
    case 8: return 4;
    case 9: return N * 4;
    case 10: return N;
    default: return 4;
    }
}
static_assert(kP16Ent0 + p16_rec_bytes(16, 0) <= kP16Pos1 && kP16Pos1 + p16_rec_bytes(16, 1) <= kP16Pos2 &&
              kP16Pos2 + p16_rec_bytes(16, 2) <= kP16Pos3 && kP16Pos3 + p16_rec_bytes(16, 3) <= kP16S0 &&
              kP16S0 + p16_rec_bytes(16, 4) <= kP16S1 && kP16S1 + p16_rec_bytes(16, 5) <= kP16S2 &&
              kP16S2 + p16_rec_bytes(16, 6) <= kP16S3 && kP16S3 + p16_rec_bytes(16, 7) <= kP16Lists && kP16Rec % 4 == 0, "");
template <int N> constexpr int p16_lds_bytes() { return p16_gram_floats<N>() * 4 + kP16Waves * kP16Scratch; }      // 157,696 (N = 16), 62,464 (N = 8)
static_assert(kP16Sel + kSelectLdsU64 * 8 <= kP16Scratch && kP16T2 + 16 * 17 * 4 <= kP16Sel && kP16T1 + 8 * 9 * 4 <= kP16T2, "");

__device__ __forceinline__ int shfl_i(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }

// first float of block (n, m), n < m
template <int N>
__device__ __forceinline__ int p16_blk(int n, int m) { return ((n * (2 * N - 1 - n)) / 2 + m - n - 1) * 256; }

// G[(n, i)][(m, j)], n != m, from the triangular store (G is symmetric bit for bit)
template <int N>
__device__ __forceinline__ float p16_g(const float *Gt, int n, int i, int m, int j) {
    const bool lt = n < m;
    const int lo = lt ? n : m, hi = lt ? m : n, a = lt ? i : j, b = lt ? j : i;
    return Gt[p16_blk<N>(lo, hi) + a * 16 + b];
}

// leaf entry D[n][m] (n < m) for the entries ea of n and eb of m; on / om the current entries: ((g - u) - v) + w
__device__ __forceinline__ float p16_leaf(const float *blk, int ea, int eb, int on, int om) {
    const float g = blk[ea * 16 + eb], u = blk[ea * 16 + om], v = blk[on * 16 + eb], w = blk[on * 16 + om];
    return ((g - u) - v) + w;
}

// T_1[X][Y][i][j] of two level-1 groups X < Y (pairs of codebooks) for this lane's candidates i of X and j of Y
template <int N>
__device__ __forceinline__ float p16_t1(const float *Gt, const uint8_t *ent0, const uint8_t *pos1, int e, int X, int Y, int i, int j) {
    const unsigned pi = *reinterpret_cast<const uint16_t *>(pos1 + (X * 8 + i) * 2), pj = *reinterpret_cast<const uint16_t *>(pos1 + (Y * 8 + j) * 2);
    const int i0 = pi & 0xff, i1 = pi >> 8, j0 = pj & 0xff, j1 = pj >> 8;
    const int ea0 = ent0[(2 * X) * 8 + i0], ea1 = ent0[(2 * X + 1) * 8 + i1], eb0 = ent0[(2 * Y) * 8 + j0], eb1 = ent0[(2 * Y + 1) * 8 + j1];
    const int on0 = __builtin_amdgcn_readlane(e, 2 * X), on1 = __builtin_amdgcn_readlane(e, 2 * X + 1);
    const int om0 = __builtin_amdgcn_readlane(e, 2 * Y), om1 = __builtin_amdgcn_readlane(e, 2 * Y + 1);
    const float d00 = p16_leaf(Gt + p16_blk<N>(2 * X, 2 * Y), ea0, eb0, on0, om0);
    const float d01 = p16_leaf(Gt + p16_blk<N>(2 * X, 2 * Y + 1), ea0, eb1, on0, om1);
    const float d10 = p16_leaf(Gt + p16_blk<N>(2 * X + 1, 2 * Y), ea1, eb0, on1, om0);
    const float d11 = p16_leaf(Gt + p16_blk<N>(2 * X + 1, 2 * Y + 1), ea1, eb1, on1, om1);
    return ((d00 + d01) + d10) + d11;
}

// The pass itself is mcq_pass16_body.inc, compiled twice.  k_tf_pass16_probe (for mcq_test_pass16 of include/mcq_probe.h): after the
// winner's walk of every pass the wave also leaves one record of (vector b, pass) at dump + (b * iters + pass) * kP16Rec, before
// it leaves a vector at its fixed point; nothing else differs, and none of it is compiled into k_tf_pass16
template <int N>
__global__ void __launch_bounds__(64 * kP16Waves)
k_tf_pass16(Pass16Args a) {
    constexpr bool PROBE = false;
    [[maybe_unused]] uint8_t *const dump = nullptr;
#include "mcq_pass16_body.inc"
}

template <int N>
__global__ void __launch_bounds__(64 * kP16Waves)
k_tf_pass16_probe(Pass16Args a, uint8_t *dump) {
    constexpr bool PROBE = true;
#include "mcq_pass16_body.inc"
}

}  // namespace mcq
