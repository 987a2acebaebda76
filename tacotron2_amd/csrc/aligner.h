// Learned-aligner scores (tacotron2_amd/alignment.py): what csrc/aligner.hip (the three MFMA products) and
// csrc/aligner_rows.hip (the row passes, the packing kernels, the prior) share: the limits, the argument check and the layout
// of the two workspaces.  Every region starts on a multiple of 16 bytes.
//   forward  [Kp  B N_max Cp  the keys, a row of C rounded up to 32, zeros beyond C and in rows at and beyond N_b]
//            [kn  B N_max     |k_n|^2 (0 at and beyond N_b)]
//            [lse B T_max     only where kept: the row logsumexp of z]
//   backward [dz  B T_max Np  z, then dz in place; a row of N_max rounded up to 32]
//            [KT  B C Np      the keys transposed, zeros at and beyond N_b]
//            [QT  B C Tp      the queries transposed, a row of T_max rounded up to 32, zeros at and beyond T_b]
//            [cs  B N_max     the column sums of dz]
#pragma once
#include "common.h"

#define AL_MAX_T 4096
#define AL_MAX_N 1024
#define AL_MAX_C 512
#define AL_MAX_B 65535                  /* utterances: grid.z of the products */
#define AL_ROWS 16                      /* rows of a workgroup of the row passes: 4 waves, 4 rows each */


struct AlFwdWs {
    long long kp, kn, lse, bytes;       // byte offsets
    int Cp;
};
struct AlBwdWs {
    long long dz, kt, qt, cs, bytes;
    int Np, Tp;
};

static inline AlFwdWs al_fwd_ws(int B, int T_max, int N_max, int C, int keep) {
    AlFwdWs w;
    w.Cp = (int)t2_round_up(C, 32);
    w.kp = 0;
    w.kn = w.kp + 4LL * B * N_max * w.Cp;
    w.lse = w.kn + 4 * t2_round_up((long long)B * N_max, 4);
    w.bytes = w.lse + (keep ? 4 * t2_round_up((long long)B * T_max, 4) : 0);
    return w;
}

static inline AlBwdWs al_bwd_ws(int B, int T_max, int N_max, int C) {
    AlBwdWs w;
    w.Np = (int)t2_round_up(N_max, 32);
    w.Tp = (int)t2_round_up(T_max, 32);
    w.dz = 0;
    w.kt = w.dz + 4LL * B * T_max * w.Np;
    w.qt = w.kt + 4LL * B * C * w.Np;
    w.cs = w.qt + 4LL * B * C * w.Tp;
    w.bytes = w.cs + 4 * t2_round_up((long long)B * N_max, 4);
    return w;
}

// the limits every entry shares; `who` is the entry's prefix of the error text
static inline int al_check(const char* who, int B, int T_max, int N_max, int C) {
    char msg[160];
    const char* what = !(B >= 1 && B <= AL_MAX_B)    ? "1 to 65535 utterances"
                       : !(T_max >= 1 && N_max >= 1) ? "at least 1 frame and 1 token"
                       : !(T_max <= AL_MAX_T)        ? "at most 4096 frames"
                       : !(N_max <= AL_MAX_N)        ? "at most 1024 tokens"
                       : !(C >= 1 && C <= AL_MAX_C)  ? "1 to 512 channels"
                                                     : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, sizeof(msg), "%s: %s: B %d frames %d tokens %d channels %d", who, what, B, T_max, N_max, C);
    T2_FAIL(msg);
}
