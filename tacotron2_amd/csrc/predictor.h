// The thin ends of a temporal predictor (tacotron2_amd/fastpitch.py): what the entries of
// csrc/predictor_rows.hip share: the limits, the workspace layouts and the argument checks.
//   thin projection  h (B, T, C), w [P][C], bias [P] -> y (B, T, P), 1 <= P <= 4.
//   thin embedding   v (B, T, P) scalar tracks, weight image [P k][C] with image[p k + j][c] = w(c, p, j), bias [C], base
//                    (B, T, C) -> y (B, T, C).
//   sums             P parts over runs of the flattened (b, t), the plan of the FFT block's column sums (FfbSumPlan).  Workspace
//                    `which` 1 (the projection's dw and db): [parts][P C | 4]; `which` 2 (the embedding's): [parts][P k + 1][C],
//                    the last row of a part being the bias sum.
#pragma once
#include "fft_block.h"

#define PRED_MAX_T FFB_MAX_T
#define PRED_MAX_C FFB_MAX_C
#define PRED_MIN_C 32
#define PRED_MAX_TAPS FFB_MAX_TAPS
#define PRED_MAX_P 4
#define PRED_MAX_B FFB_MAX_B

static inline long long pred_project_sum_bytes(int B, int T, int C, int P) { return 4LL * ffb_sum_plan(B, T).P * ((long long)P * C + 4); }
static inline long long pred_embed_sum_bytes(int B, int T, int C, int P, int k) {
    return 4LL * ffb_sum_plan(B, T).P * ((long long)P * k + 1) * C;
}

// the limits of every entry; `who` is the entry's name inside the error text
static inline int pred_check(const char* who, int B, int T, int C, int P, int k) {
    char msg[200];
    const char* what = !(B >= 1 && T >= 1)                                       ? "at least 1 utterance and 1 frame"
                       : !(B <= PRED_MAX_B)                                      ? "at most 65535 utterances"
                       : !(T <= PRED_MAX_T)                                      ? "at most 4096 frames"
                       : !(C >= PRED_MIN_C && C <= PRED_MAX_C && C % 4 == 0)     ? "channels must be a multiple of 4, from 32 to 4096"
                       : !(P >= 1 && P <= PRED_MAX_P)                            ? "1 to 4 scalar tracks"
                       : !(k >= 1 && k <= PRED_MAX_TAPS && k % 2 == 1)           ? "an odd kernel width from 1 to 9"
                                                                                 : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, sizeof(msg), "predictor: %s: %s: B %d frames %d channels %d tracks %d width %d", who, what, B, T, C, P, k);
    T2_FAIL(msg);
}
