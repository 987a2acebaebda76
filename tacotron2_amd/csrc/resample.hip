// Sample-rate conversion (tacotron2_amd/audio.py Resample): band-limited sinc interpolation with a Hann
// window as a polyphase FIR gather, and its adjoint as a gather of the same shape.  With o = orig / gcd, n = new / gcd:
//   resample_fwd:  y[q n + j]   = sum_s tab[j][s] xpad[q o + first[j] + s],   xpad = x with `width` zeros in front
//   resample_bwd:  d_x[q o + r] = sum_s btab[r][s] d_ypad[q n + bfirst[r] + s], d_ypad = d_y with `wpad` zeros in front
// tab (n, S) holds the consecutive non-zero taps of phase j of the dense (n, 2 width + o) table and first[j] the index of the
// first of them; btab (o, Sb) holds the SAME float32 coefficients regrouped by input phase r, in ascending output index, so the
// second launch is the exact transpose of the first.  Both are one tile routine (rs_tile): a workgroup owns a run of `npw`
// consecutive outputs of one utterance, stages the input window those outputs read in LDS (16-byte loads where the row is
// 16-byte aligned, zeros outside the utterance), stages the phase table in LDS when it fits RS_TAB_LDS floats and reads it from
// memory otherwise, then takes one output per lane and adds its taps in ascending s with one fma each.
// Ragged batches: lengths[b] (input samples, clamped to [0, T]); x at or beyond it reads as zero whatever the buffer holds, y is
// exactly 0 at and beyond ceil(n lengths[b] / o); the backward reads no d_y there and writes exactly 0 into d_x at and beyond
// lengths[b].  Every output element has one writer and a fixed summation order, no atomics: two calls give the same bits, and an
// utterance in a ragged batch gives the bits it gives alone.
// No MFMA and no LDS-DMA here, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "common.h"

#define RS_THREADS 256
#define RS_MAX_RUN 1024                 /* outputs of one workgroup, at most */
#define RS_XWIN 4096                    /* floats of the input window in LDS (16 KiB) */
#define RS_TAB_LDS 8192                 /* floats of the phase table and its first-tap indices in LDS (32 KiB) */
#define RS_TAB_MAX 16777216LL           /* taps of a phase table, at most (64 MiB) */

// ADJ = false: the forward (phases n, input period o); ADJ = true: the adjoint (phases o, input period n).  `Kd` bounds
// first[ph] + S, so the outputs of period q read in[q I - wpad, q I - wpad + Kd).
template <bool ADJ>
__device__ __forceinline__ void rs_tile(float* xs, float* ts, const float* __restrict__ in, long long ldi, float* __restrict__ out,
                                        long long ldo, const int* __restrict__ lengths, int T, int Tout, int o, int n,
                                        const float* __restrict__ tab, const int* __restrict__ first, int S, int wpad, int Kd,
                                        int npw, int tab_lds, int vec) {
    const int tid = threadIdx.x, b = blockIdx.y;
    const int P = ADJ ? o : n, I = ADJ ? n : o;
    const int len = lengths ? t2_clamp_count(lengths[b], T) : T;
    const int ylen = (int)(((long long)n * len + o - 1) / o);
    const int in_valid = ADJ ? ylen : len, out_valid = ADJ ? len : ylen, n_out = ADJ ? T : Tout;
    const long long m0 = (long long)blockIdx.x * npw;
    const long long m1 = m0 + npw < n_out ? m0 + npw : n_out;
    const long long me = m1 < out_valid ? m1 : out_valid;               // outputs at and beyond `me` are exact zeros
    in += b * ldi;
    out += b * ldo;
    const int Sp = S | 1;                                               // odd row stride in LDS: adjacent phases, distinct banks
    int* fl = reinterpret_cast<int*>(ts + (tab_lds ? P * Sp : 0));
    long long a0 = 0;
    if (me > m0) {                                                      // uniform over the workgroup
        if (tab_lds) {
            for (int e = tid; e < P * S; e += RS_THREADS) {
                const int ph = e / S;
                ts[ph * Sp + (e - ph * S)] = tab[e];
            }
            for (int ph = tid; ph < P; ph += RS_THREADS) fl[ph] = first[ph];
        }
        const long long q_lo = m0 / P, q_hi = (me - 1) / P;
        const long long g0 = q_lo * I - wpad;
        a0 = g0 - ((g0 % 4) + 4) % 4;                                   // the window starts on a multiple of 4 samples
        const int wlen = (int)(q_hi * I + Kd - wpad - a0);              // <= RS_XWIN - 3 by the launcher's choice of npw
        for (int c = tid; 4 * c < wlen; c += RS_THREADS) {
            const long long gi = a0 + 4 * c;
            float4 v;
            if (vec && gi >= 0 && gi + 4 <= in_valid) {
                v = *reinterpret_cast<const float4*>(in + gi);
            } else {
                v.x = gi >= 0 && gi < in_valid ? in[gi] : 0.0f;
                v.y = gi + 1 >= 0 && gi + 1 < in_valid ? in[gi + 1] : 0.0f;
                v.z = gi + 2 >= 0 && gi + 2 < in_valid ? in[gi + 2] : 0.0f;
                v.w = gi + 3 >= 0 && gi + 3 < in_valid ? in[gi + 3] : 0.0f;
            }
            *reinterpret_cast<float4*>(xs + 4 * c) = v;
        }
        __syncthreads();
    }
    for (long long m = m0 + tid; m < m1; m += RS_THREADS) {
        float acc = 0.0f;
        if (m < me) {
            const int q = (int)m / P, ph = (int)m - q * P;                // m < n_out < 2^31
            int f = tab_lds ? fl[ph] : first[ph];
            f = f < 0 ? 0 : (f > Kd - S ? Kd - S : f);
            const float* xw = xs + (int)((long long)q * I - wpad - a0) + f;
            const float* tw = tab_lds ? ts + ph * Sp : tab + (long long)ph * S;
            for (int s = 0; s < S; ++s) acc = fmaf(tw[s], xw[s], acc);
        }
        out[m] = acc;
    }
}

__global__ void __launch_bounds__(RS_THREADS) resample_fwd_kernel(const float* __restrict__ x, long long ldx,
                                                                  const int* __restrict__ lengths, int T, float* __restrict__ y,
                                                                  long long ldy, int Tout, int o, int n,
                                                                  const float* __restrict__ tab, const int* __restrict__ first,
                                                                  int S, int wpad, int Kd, int npw, int tab_lds, int vec) {
    __shared__ __attribute__((aligned(16))) float xs[RS_XWIN];
    __shared__ __attribute__((aligned(16))) float ts[RS_TAB_LDS];
    rs_tile<false>(xs, ts, x, ldx, y, ldy, lengths, T, Tout, o, n, tab, first, S, wpad, Kd, npw, tab_lds, vec);
}

__global__ void __launch_bounds__(RS_THREADS) resample_bwd_kernel(const float* __restrict__ d_y, long long ldy,
                                                                  const int* __restrict__ lengths, int T, float* __restrict__ d_x,
                                                                  long long ldx, int Tout, int o, int n,
                                                                  const float* __restrict__ btab, const int* __restrict__ bfirst,
                                                                  int Sb, int wpad, int Kd, int npw, int tab_lds, int vec) {
    __shared__ __attribute__((aligned(16))) float xs[RS_XWIN];
    __shared__ __attribute__((aligned(16))) float ts[RS_TAB_LDS];
    rs_tile<true>(xs, ts, d_y, ldy, d_x, ldx, lengths, T, Tout, o, n, btab, bfirst, Sb, wpad, Kd, npw, tab_lds, vec);
}

// The tile of a launch with P phases of S taps, input period I and first[ph] + S <= Kd: the longest run npw in {1024, 768, 512,
// 256} whose input window fits RS_XWIN, and whether the table (P rows of S | 1 floats and P first-tap indices) is staged in LDS.
extern "C" int t2amd_resample_plan(int P, int I, int S, int Kd, int* npw, int* tab_lds) {
    T2_REQUIRE(P > 0 && I > 0 && S > 0 && Kd >= S, "resample: bad table geometry");
    T2_REQUIRE((long long)P * S <= RS_TAB_MAX, "resample: the phase table holds more than 2^24 taps");
    int run = 0;
    for (int cand = RS_MAX_RUN; cand >= RS_THREADS && !run; cand -= RS_THREADS)
        if (((long long)(cand - 1) / P + 1) * I + Kd + 6 <= RS_XWIN) run = cand;
    T2_REQUIRE(run > 0, "resample: the input window of 256 outputs exceeds 4096 samples at this ratio");
    if (npw) *npw = run;
    if (tab_lds) *tab_lds = (long long)P * ((S | 1) + 1) <= RS_TAB_LDS ? 1 : 0;
    return T2AMD_OK;
}

static int rs_check(const char* who, const void* x, long long ldx, const void* y, long long ldy, const void* tab, const void* first,
                    int B, int T, int Tout, int o, int n, int S, long long ntab, char* msg) {
    const char* what = !(x && y && tab && first)                          ? "null operand"
                       : !(B > 0 && B <= 65535)                           ? "1 to 65535 utterances"
                       : !(o > 0 && n > 0 && S > 0)                       ? "bad table geometry"
                       : !(T > 0 && T <= T2_MAX_ROWS && Tout <= T2_MAX_ROWS && ldx <= T2_MAX_ROWS && ldy <= T2_MAX_ROWS)
                           ? "rows of at most 2^31 - 256 samples"
                       : Tout != ((long long)n * T + o - 1) / o           ? "the output has ceil(n T / o) samples"
                       : !(ldx >= T && ldy >= Tout)                       ? "row too short"
                       : !(ntab <= RS_TAB_MAX)                            ? "the phase table holds more than 2^24 taps"
                                                                          : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, 160, "%s: %s", who, what);
    return T2AMD_ERR_ARG;
}

extern "C" int t2amd_resample_fwd_f32(const float* x, long long ldx, const int* lengths, int B, long long T, float* y, long long ldy,
                                      long long Tout, const float* tab, const int* first, int o, int n, int S, int width,
                                      void* stream) {
    char msg[160];
    T2_REQUIRE(T < 2147483648LL && Tout < 2147483648LL, "resample_fwd: rows of at most 2^31 - 256 samples");
    if (rs_check("resample_fwd", x, ldx, y, ldy, tab, first, B, (int)T, (int)Tout, o, n, S, (long long)n * S, msg) != T2AMD_OK)
        T2_FAIL(msg);
    T2_REQUIRE(width >= 0 && width <= 1073741824 - o, "resample_fwd: bad width");
    const int Kd = 2 * width + o;
    int npw, tab_lds;
    T2_PROPAGATE(t2amd_resample_plan(n, o, S, Kd, &npw, &tab_lds));
    const long long xb = ((B - 1) * ldx + T) * 4, yb = ((B - 1) * ldy + Tout) * 4;
    T2_REQUIRE(!t2_overlap(y, yb, x, xb) && !t2_overlap(y, yb, tab, 4LL * n * S) && !t2_overlap(y, yb, first, 4LL * n) &&
                   !(lengths && t2_overlap(y, yb, lengths, 4LL * B)),
               "resample_fwd: y must not be one of the inputs");
    const int vec = t2_aligned16(x) && ldx % 4 == 0;
    T2_LAUNCH(resample_fwd_kernel, dim3((unsigned)((Tout + npw - 1) / npw), (unsigned)B), dim3(RS_THREADS), 0, (hipStream_t)stream, x,
              ldx, lengths, (int)T, y, ldy, (int)Tout, o, n, tab, first, S, width, Kd, npw, tab_lds, vec);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_resample_bwd_f32(const float* d_y, long long ldy, const int* lengths, int B, long long T, long long Tout,
                                      float* d_x, long long ldx, const float* btab, const int* bfirst, int o, int n, int Sb,
                                      int wpad, int Kd, void* stream) {
    char msg[160];
    T2_REQUIRE(T < 2147483648LL && Tout < 2147483648LL, "resample_bwd: rows of at most 2^31 - 256 samples");
    if (rs_check("resample_bwd", d_x, ldx, d_y, ldy, btab, bfirst, B, (int)T, (int)Tout, o, n, Sb, (long long)o * Sb, msg) != T2AMD_OK)
        T2_FAIL(msg);
    T2_REQUIRE(wpad >= 0 && wpad <= 1073741824 && Kd >= Sb, "resample_bwd: bad padding");
    int npw, tab_lds;
    T2_PROPAGATE(t2amd_resample_plan(o, n, Sb, Kd, &npw, &tab_lds));
    const long long xb = ((B - 1) * ldx + T) * 4, yb = ((B - 1) * ldy + Tout) * 4;
    T2_REQUIRE(!t2_overlap(d_x, xb, d_y, yb) && !t2_overlap(d_x, xb, btab, 4LL * o * Sb) && !t2_overlap(d_x, xb, bfirst, 4LL * o) &&
                   !(lengths && t2_overlap(d_x, xb, lengths, 4LL * B)),
               "resample_bwd: d_x must not be one of the inputs");
    const int vec = t2_aligned16(d_y) && ldy % 4 == 0;
    T2_LAUNCH(resample_bwd_kernel, dim3((unsigned)((T + npw - 1) / npw), (unsigned)B), dim3(RS_THREADS), 0, (hipStream_t)stream, d_y,
              ldy, lengths, (int)T, d_x, ldx, (int)Tout, o, n, btab, bfirst, Sb, wpad, Kd, npw, tab_lds, vec);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
