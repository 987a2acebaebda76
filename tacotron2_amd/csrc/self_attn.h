// Masked multi-head self-attention (tacotron2_amd/transformer.py): what csrc/self_attn.hip (the three MFMA
// kernels) and csrc/self_attn_rows.hip (the delta pass, the limits and the workspace entry) share: the limits, the description of
// a strided (B, T, H, D) operand, the argument checks and the workspace layout.
//   operand   element (b, t, h, d) of q, k, v and g lies at base + b sb + t st + h sh + d: the last axis has stride 1, the other
//             strides are multiples of 4 floats and the base is aligned to 16 bytes, so every row of D floats is read as float4.
//   o, dq, dk, dv   contiguous (B, T, H, D);  lse, delta   contiguous (B, H, T).
//   workspace which 0 (forward, nothing kept): 0 bytes;  1 (forward with lse kept): [lse B H T];  2 (backward): [delta B H T].
//             Each is 4 B H T bytes rounded up to 16; lse itself is the caller's tensor, `which` 1 only reports its size.
#pragma once
#include "common.h"

#define SA_MAX_T 4096
#define SA_MAX_H 16
#define SA_MIN_D 32
#define SA_MAX_D 128
#define SA_MAX_BH 65535                 /* utterances times heads: grid.y */
#define SA_BM 128                       /* rows of a workgroup: 4 waves of 32 */
#define SA_FWD_BN 64                    /* keys of a forward step */
#define SA_BWD_BN 32                    /* queries (dK, dV) or keys (dQ) of a backward step */

struct SaOperand {
    const float* p;
    long long sb, st, sh;
};

static inline long long sa_rows_bytes(int B, int T, int H) { return 4 * t2_round_up((long long)B * H * T, 4); }

// bytes from the operand's base to the end of its last row
static inline long long sa_span(const SaOperand& x, int B, int T, int H, int D) {
    return t2_span_bytes(x.sb, x.st, B, T, (H - 1) * x.sh + D);
}

// the limits every entry shares; `who` is the entry's name inside the error text
static inline int sa_check(const char* who, int B, int T, int H, int D) {
    char msg[200];
    const char* what = !(B >= 1 && T >= 1)                                    ? "at least 1 utterance and 1 frame"
                       : !(T <= SA_MAX_T)                                     ? "at most 4096 frames"
                       : !(H >= 1 && H <= SA_MAX_H)                           ? "1 to 16 heads"
                       : !(D >= SA_MIN_D && D <= SA_MAX_D && D % 32 == 0)     ? "a head width of 32, 64, 96 or 128"
                       : !((long long)B * H <= SA_MAX_BH)                     ? "at most 65535 utterances times heads"
                                                                              : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, sizeof(msg), "self_attn: %s: %s: B %d frames %d heads %d width %d", who, what, B, T, H, D);
    T2_FAIL(msg);
}

// a strided input: not null, aligned, strides that are multiples of 4 floats; `name` is the operand's
static inline int sa_check_operand(const char* who, const char* name, const SaOperand& x) {
    char msg[200];
    const char* what = !x.p                                                           ? "null operand"
                       : !t2_aligned16(x.p)                                           ? "is not aligned to 16 bytes"
                       : !(x.sb >= 0 && x.st >= 0 && x.sh >= 0)                       ? "has a negative stride"
                       : !(x.sb % 4 == 0 && x.st % 4 == 0 && x.sh % 4 == 0)           ? "strides must be multiples of 4 floats"
                                                                                      : nullptr;
    if (!what) return T2AMD_OK;
    if (!x.p)
        snprintf(msg, sizeof(msg), "self_attn: %s: %s", who, what);
    else
        snprintf(msg, sizeof(msg), "self_attn: %s: %s %s", who, name, what);
    T2_FAIL(msg);
}
