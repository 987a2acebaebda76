// The feed-forward Transformer block's convolutional feed-forward and add + LayerNorm (tacotron2_amd/transformer.py, DESIGN.md
// section 23): what csrc/fft_block.hip (the two MFMA products) and csrc/fft_block_rows.hip (the row kernels, the limits and the
// workspace entry) share: the limits, the plan of the weight gradient's reduction, the workspace layouts and the argument checks.
//   x            element (b, t, i) of a convolution's input lies at x[b xb + t xt + i]: unit channel stride, the other strides
//                multiples of 4 floats, the base on 16 bytes.  Every other tensor is contiguous (B, T, C) channel-last.
//   weight image [Cout][k Cin], tap-major: image[o][j Cin + i] = w(o, i, j); the dx image is that of the flipped, transposed
//                weights, [Cin][k Cout] with image[i][j Cout + o] = w(o, i, k - 1 - j).
//   dw reduction the flattened index q = b Tp + t with Tp = T rounded up to 32, cut into S slices of L indices (FfbDwPlan; S and
//                L depend on B and T alone).  Workspace `which` 1: [gT: S slabs [Cout][L] | partials: S [k Cin][Cout]].
//   column sums  P partial sums over the rows p RP .. p RP + RP - 1 of the flattened (b, t) (FfbSumPlan).  Workspace `which` 2:
//                [P][2][C].
#pragma once
#include "common.h"

#define FFB_MAX_T 4096
#define FFB_MAX_C 4096
#define FFB_MAX_TAPS 9
#define FFB_MIN_LN 32
#define FFB_MAX_B 65535                 /* utterances: grid.z, grid.y */
#define FFB_DW_SLICE 512                /* reduction indices a slice aims at */
#define FFB_DW_MAX_SLICES 8
#define FFB_SUM_MAX_PARTS 64


struct FfbDwPlan {
    int Tp, S, L;                       // frames an utterance takes in the reduction; slices; indices a slice
};
static inline FfbDwPlan ffb_dw_plan(int B, int T) {
    FfbDwPlan p;
    p.Tp = (int)t2_round_up(T, 32);
    const long long K = (long long)B * p.Tp;
    long long S = (K + FFB_DW_SLICE - 1) / FFB_DW_SLICE;
    p.S = (int)(S > FFB_DW_MAX_SLICES ? FFB_DW_MAX_SLICES : S);
    p.L = (int)t2_round_up((K + p.S - 1) / p.S, 32);
    return p;
}

struct FfbSumPlan {
    int P;                              // partial sums
    long long RP;                       // rows a partial sum
};
static inline FfbSumPlan ffb_sum_plan(int B, int T) {
    const long long rows = (long long)B * T;
    long long P = (rows + 63) / 64;
    FfbSumPlan p;
    p.P = (int)(P > FFB_SUM_MAX_PARTS ? FFB_SUM_MAX_PARTS : P);
    p.RP = (rows + p.P - 1) / p.P;
    return p;
}

struct FfbDwWs {
    long long gt, part, bytes;
};
static inline FfbDwWs ffb_dw_ws(int B, int T, int Cin, int Cout, int k) {
    const FfbDwPlan d = ffb_dw_plan(B, T);
    FfbDwWs w;
    w.gt = 0;
    w.part = 4LL * d.S * Cout * d.L;
    w.bytes = w.part + 4LL * d.S * k * Cin * Cout;
    return w;
}
static inline long long ffb_sum_bytes(int B, int T, int C) { return 4LL * ffb_sum_plan(B, T).P * 2 * C; }

// the limits of a convolution; `who` is the entry's name inside the error text
static inline int ffb_check_conv(const char* who, int B, int T, int Cin, int Cout, int k) {
    char msg[200];
    const char* what = !(B >= 1 && T >= 1)                                    ? "at least 1 utterance and 1 frame"
                       : !(B <= FFB_MAX_B)                                    ? "at most 65535 utterances"
                       : !(T <= FFB_MAX_T)                                    ? "at most 4096 frames"
                       : !(k >= 1 && k <= FFB_MAX_TAPS && k % 2 == 1)         ? "an odd kernel width from 1 to 9"
                       : !(Cin >= 32 && Cin <= FFB_MAX_C && Cin % 32 == 0)    ? "input channels must be a multiple of 32, at most 4096"
                       : !(Cout >= 32 && Cout <= FFB_MAX_C && Cout % 32 == 0) ? "output channels must be a multiple of 32, at most 4096"
                                                                              : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, sizeof(msg), "fft_block: %s: %s: B %d frames %d channels %d to %d width %d", who, what, B, T, Cin, Cout, k);
    T2_FAIL(msg);
}

// the limits of a row kernel over (B, T, C)
static inline int ffb_check_rows(const char* who, int B, int T, int C, int min_c) {
    char msg[200];
    const char* what = !(B >= 1 && T >= 1)                            ? "at least 1 utterance and 1 frame"
                       : !(B <= FFB_MAX_B)                            ? "at most 65535 utterances"
                       : !(T <= FFB_MAX_T)                            ? "at most 4096 frames"
                       : !(C >= min_c && C <= FFB_MAX_C && C % 4 == 0) ? "channels must be a multiple of 4, from 32 to 4096"
                                                                      : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, sizeof(msg), "fft_block: %s: %s: B %d frames %d channels %d", who, what, B, T, C);
    T2_FAIL(msg);
}

// a strided (B, T, C) input: aligned, strides that are multiples of 4 floats and hold a row
static inline int ffb_check_x(const char* who, const float* x, long long xb, long long xt, int B, int T, int C) {
    char msg[200];
    const char* what = !x                                              ? "null operand"
                       : !t2_aligned16(x)                              ? "x is not aligned to 16 bytes"
                       : !(xb >= 0 && xt >= 0)                         ? "x has a negative stride"
                       : !(xb % 4 == 0 && xt % 4 == 0)                 ? "x strides must be multiples of 4 floats"
                       : !((T == 1 || xt >= C) && (B == 1 || xb >= C)) ? "x strides are shorter than a row"
                                                                       : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, sizeof(msg), "fft_block: %s: %s", who, what);
    T2_FAIL(msg);
}
