// Vocos vocoder (Siuzdak 2023), the row kernels around the products of vocos.hip (which has the layout and the launch list):
// vc_dwln:  depthwise `taps`-tap convolution over the rows plus LayerNorm over the D channels of every row, one launch; taps = 0
//           is LayerNorm alone (the one after embed and the final one).  One wave per row, 16-byte accesses, the two row
//           reductions as xor butterflies in a fixed order (no atomics): a row's bits do not depend on where it lies.
// vc_polar: head rows [m_0 .. m_{F-1} | p_0 .. p_{F-1}] -> interleaved (re, im) rows min(exp m, 100) (cos p, sin p).
// vc_ola:   overlap-add of the windowed inverse-DFT frames, trimmed per utterance, divided by the squared-window envelope of
//           that utterance's own frames, written into (B, T); zero beyond each utterance.
// Every kernel writes all rows of its output and writes zero on halo rows (rowb0 < 0): a LayerNorm bias or exp(head bias)
// never leaks into a halo.  No MFMA here, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "common.h"

#define VC_MAX_D 512
#define VC_MAX_TAPS 15
#define VC_DWLN_ROWS 4                  /* waves (= rows) per workgroup */

__global__ __launch_bounds__(64 * VC_DWLN_ROWS) void vc_dwln_kernel(const float* X, long long ldx, long long P, int D,
                                                                    const float* w, const float* cb, int taps, const float* lw,
                                                                    const float* lb, float eps, const int* rowb0, float* out,
                                                                    long long ldo) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long p = (long long)blockIdx.x * VC_DWLN_ROWS + wave;
    const bool inside = p < P;
    const bool real = inside && rowb0[p] >= 0;
    const int nq = D >> 2, half = (taps - 1) / 2;
    float4 v[VC_MAX_D / 256];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VC_MAX_D / 256; ++i) {
        const int q = lane + 64 * i;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (real && q < nq) {
            if (taps == 0) {
                a = *reinterpret_cast<const float4*>(X + p * ldx + 4 * q);
            } else {
                a = *reinterpret_cast<const float4*>(cb + 4 * q);
                for (int t = 0; t < taps; ++t) {
                    const long long src = p + t - half;
                    if (src < 0 || src >= P) continue;
                    const float4 x = *reinterpret_cast<const float4*>(X + src * ldx + 4 * q);
                    const float4 k = *reinterpret_cast<const float4*>(w + (long long)t * D + 4 * q);
                    a.x = fmaf(x.x, k.x, a.x);
                    a.y = fmaf(x.y, k.y, a.y);
                    a.z = fmaf(x.z, k.z, a.z);
                    a.w = fmaf(x.w, k.w, a.w);
                }
            }
            s += (a.x + a.y) + (a.z + a.w);
        }
        v[i] = a;
    }
    const float mean = t2_wave_sum(s) / (float)D;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VC_MAX_D / 256; ++i) {
        const int q = lane + 64 * i;
        if (real && q < nq) {
            v[i].x -= mean;
            v[i].y -= mean;
            v[i].z -= mean;
            v[i].w -= mean;
            ss += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        }
    }
    const float rstd = 1.0f / sqrtf(t2_wave_sum(ss) / (float)D + eps);
    if (!inside) return;
#pragma unroll
    for (int i = 0; i < VC_MAX_D / 256; ++i) {
        const int q = lane + 64 * i;
        if (q >= nq) continue;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (real) {
            const float4 g = *reinterpret_cast<const float4*>(lw + 4 * q);
            const float4 b = *reinterpret_cast<const float4*>(lb + 4 * q);
            o.x = fmaf(v[i].x * rstd, g.x, b.x);
            o.y = fmaf(v[i].y * rstd, g.y, b.y);
            o.z = fmaf(v[i].z * rstd, g.z, b.z);
            o.w = fmaf(v[i].w * rstd, g.w, b.w);
        }
        *reinterpret_cast<float4*>(out + p * ldo + 4 * q) = o;
    }
}

extern "C" int t2amd_vc_dwln_f32(const float* X, long long x_floats, long long ldx, long long P, int D, const float* w,
                                 long long w_floats, const float* conv_bias, int taps, const float* ln_w, const float* ln_b,
                                 float eps, const int* rowb0, long long n_rowb, float* out, long long ldout,
                                 long long out_floats, void* stream) {
    T2_REQUIRE(X && ln_w && ln_b && rowb0 && out, "vc_dwln: null operand");
    T2_REQUIRE(P > 0 && P <= T2_MAX_ROWS && n_rowb >= P, "vc_dwln: the row map does not cover the rows (at most 2^31 - 256)");
    T2_REQUIRE(D >= 32 && D % 32 == 0 && D <= VC_MAX_D, "vc_dwln: channels must be a multiple of 32, at most 512");
    T2_REQUIRE(taps == 0 || (taps % 2 == 1 && taps <= VC_MAX_TAPS), "vc_dwln: taps must be 0 (LayerNorm alone) or odd, at most 15");
    T2_REQUIRE(taps == 0 || (w && conv_bias && w_floats >= (long long)taps * D), "vc_dwln: w is shorter than [taps][D]");
    T2_REQUIRE(eps > 0.f, "vc_dwln: eps must be positive");
    T2_REQUIRE(ldx >= D && ldx % 4 == 0 && ldout >= D && ldout % 4 == 0, "vc_dwln: rows must hold D floats at a multiple of 4");
    T2_REQUIRE(t2_aligned16(X) && t2_aligned16(out) && t2_aligned16(ln_w) && t2_aligned16(ln_b) &&
                   (taps == 0 || (t2_aligned16(w) && t2_aligned16(conv_bias))),
               "vc_dwln: operands must be 16-byte aligned");
    T2_REQUIRE(x_floats >= (P - 1) * ldx + D, "vc_dwln: X is shorter than its rows");
    T2_REQUIRE(out_floats >= (P - 1) * ldout + D, "vc_dwln: out is shorter than its rows");
    T2_REQUIRE(X != out, "vc_dwln: out must not be X (a row's window reads its neighbours)");
    T2_LAUNCH(vc_dwln_kernel, dim3(t2_cdiv(P, VC_DWLN_ROWS)), dim3(64 * VC_DWLN_ROWS), 0, (hipStream_t)stream, X, ldx, P, D, w,
              conv_bias, taps, ln_w, ln_b, eps, rowb0, out, ldout);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

__global__ __launch_bounds__(256) void vc_polar_kernel(const float* Y, long long ldy, long long P, int F, float clamp,
                                                       const int* rowb0, float* S, long long lds) {
    const int half = (int)(lds >> 1);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P * half) return;
    const long long p = i / half;
    const int k = (int)(i - p * half);
    float re = 0.f, im = 0.f;
    if (k < F && rowb0[p] >= 0) {
        const float mag = fminf(expf(Y[p * ldy + k]), clamp);
        float sn, cs;
        sincosf(Y[p * ldy + F + k], &sn, &cs);
        re = mag * cs;
        im = mag * sn;
    }
    S[p * lds + 2 * k] = re;
    S[p * lds + 2 * k + 1] = im;
}

extern "C" int t2amd_vc_polar_f32(const float* Y, long long y_floats, long long ldy, long long P, int F, float clamp,
                                  const int* rowb0, long long n_rowb, float* S, long long lds, long long s_floats,
                                  void* stream) {
    T2_REQUIRE(Y && rowb0 && S, "vc_polar: null operand");
    T2_REQUIRE(P > 0 && P <= T2_MAX_ROWS && n_rowb >= P, "vc_polar: the row map does not cover the rows (at most 2^31 - 256)");
    T2_REQUIRE(F >= 1 && F <= 8193 && clamp > 0.f, "vc_polar: 1 to 8193 bins, a positive clamp");
    T2_REQUIRE(ldy >= 2 * F && y_floats >= (P - 1) * ldy + 2 * F, "vc_polar: Y is shorter than its rows of 2 F values");
    T2_REQUIRE(lds >= 2 * F && lds % 2 == 0 && s_floats >= P * lds, "vc_polar: S is shorter than its rows of 2 F values (even stride)");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(Y) & 3u) == 0 && (reinterpret_cast<uintptr_t>(S) & 3u) == 0 && Y != S,
               "vc_polar: Y / S misaligned or the same buffer");
    T2_LAUNCH(vc_polar_kernel, dim3(t2_cdiv(P * (lds / 2), 256)), dim3(256), 0, (hipStream_t)stream, Y, ldy, P, F, clamp, rowb0,
              S, lds);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// utt[2 b] = first packed row of utterance b, utt[2 b + 1] = its frames n_b.  Sample t of utterance b is position s = t + trim
// of its untrimmed overlap-add; it has hop (n_b - 1) + L - 2 trim samples.
__global__ __launch_bounds__(256) void vc_ola_kernel(const float* frames, long long ldf, long long P, const float* wsq,
                                                     const int* utt, int L, int hop, int trim, float* out, long long T) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int b = blockIdx.y;
    const long long row0 = utt[2 * b], n = utt[2 * b + 1];
    float v = 0.f;
    if (t < hop * (n - 1) + L - 2 * trim) {
        const long long s = t + trim;
        long long j1 = s / hop, j0 = (s - L + hop) / hop;            // frames j with 0 <= s - j hop < L
        if (s - L + 1 <= 0) j0 = 0;
        if (j1 > n - 1) j1 = n - 1;
        float acc = 0.f, env = 0.f;
        for (long long j = j0; j <= j1; ++j) {
            const int off = (int)(s - j * hop);
            const long long row = row0 + j;
            if (row < 0 || row >= P) continue;
            acc += frames[row * ldf + off];
            env += wsq[off];
        }
        v = acc / env;
    }
    out[(long long)b * T + t] = v;
}

extern "C" int t2amd_vc_ola_f32(const float* frames, long long f_floats, long long ldf, long long P, const float* wsq,
                                const int* utt, int B, int L, int hop, int trim, float* out, long long T, long long out_floats,
                                void* stream) {
    T2_REQUIRE(frames && wsq && utt && out, "vc_ola: null operand");
    T2_REQUIRE(P > 0 && P <= T2_MAX_ROWS && B >= 1 && B <= 65535, "vc_ola: 1 to 65535 utterances, at most 2^31 - 256 rows");
    T2_REQUIRE(L >= 2 && L <= 16384 && hop >= 1 && hop <= L && L % hop == 0, "vc_ola: hop must divide the frame length (at most 16384)");
    T2_REQUIRE(trim >= 0 && 2 * trim >= L - hop && 2 * trim <= L, "vc_ola: trim must be (L - hop) / 2 to L / 2");
    T2_REQUIRE(ldf >= L && f_floats >= (P - 1) * ldf + L, "vc_ola: frames is shorter than its rows");
    T2_REQUIRE(T >= 1 && T <= T2_MAX_ROWS * 256 && out_floats >= (long long)B * T, "vc_ola: out is shorter than (B, T)");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
               "vc_ola: frames / out misaligned");
    T2_LAUNCH(vc_ola_kernel, dim3(t2_cdiv(T, 256), B), dim3(256), 0, (hipStream_t)stream, frames, ldf, P, wsq, utt, L, hop, trim,
              out, T);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
