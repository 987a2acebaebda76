// Vocos vocoder, the row kernels of the backward pass (tacotron2_amd/vocos.py Vocos.generate; the products of the backward are
// vc_linear and the split-K weight-gradient products of gemm.hip):
// vc_ola_bwd:   gradient of the overlap-add: every frame sample reads the one output sample it was added into, over the same
//               squared-window sum the forward divided by.
// vc_polar_bwd: gradient of min(exp m, clamp) (cos p, sin p) from the kept head rows.
// vc_gelu_bwd:  d_u = d_h (Phi(u) + u phi(u)), exact erf form, in place on d_h.
// vc_gamma_bwd: d_y2 = gamma d_x in place on the recomputed y2, and the column partials of d_gamma = sum_r d_x y2.
// vc_ln_bwd:    LayerNorm backward over the D channels of a row; with taps the depthwise convolution is recomputed from the
//               block's input first (vc_dwln_kernel's own arithmetic, so mean and rstd are the forward's bits).
// vc_dw_bwd:    the depthwise convolution's data, weight and bias gradients over the finished d_z image.
// Every kernel writes all rows of its outputs and zero on halo rows (rowb0 < 0).  A sum over rows is taken in a fixed order:
// a wave walks VCB_WAVE_ROWS consecutive rows and stores its column sums as one partial slot; t2amd_wg_partial_sum_f32 adds
// the slots in order.  No atomics, no LDS.  No MFMA here, so the CPU suite runs this very source on the host stand-in.
#include "common.h"

#define VCB_MAX_D 512
#define VCB_MAX_TAPS 7
#define VCB_WAVES 4                     /* waves per workgroup */
#define VCB_WAVE_ROWS 16                /* consecutive rows per wave = rows per partial slot */

extern "C" int t2amd_vc_bwd_slot_rows() { return VCB_WAVE_ROWS; }

// ---- overlap-add -----------------------------------------------------------------------------------------------------
// Row p of utterance b = rowb0[p], frame j = rowr0[p]: sample t of the frame is position s = j hop + t of the untrimmed
// overlap-add, output sample s - trim.  env is summed over the covering frames in ascending order, as vc_ola_kernel does.
__global__ __launch_bounds__(256) void vc_ola_bwd_kernel(const float* d_audio, long long T, const float* wsq, const int* utt,
                                                         const int* rowb0, const int* rowr0, long long P, int L, int hop,
                                                         int trim, float* d_frames, long long ldf) {
    const int nq = L >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P * nq) return;
    const long long p = i / nq;
    const int t0 = 4 * (int)(i - p * nq);
    const int b = rowb0[p];
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (b >= 0) {
        const long long n = utt[2 * b + 1], j = rowr0[p];
        const long long Tb = hop * (n - 1) + L - 2 * trim;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long s = j * hop + t0 + e, ts = s - trim;
            if (ts < 0 || ts >= Tb || ts >= T) continue;
            long long j1 = s / hop, j0 = (s - L + hop) / hop;
            if (s - L + 1 <= 0) j0 = 0;
            if (j1 > n - 1) j1 = n - 1;
            float env = 0.f;
            for (long long jj = j0; jj <= j1; ++jj) env += wsq[(int)(s - jj * hop)];
            o[e] = d_audio[(long long)b * T + ts] / env;
        }
    }
    t2_st4(d_frames + p * ldf + t0, make_float4(o[0], o[1], o[2], o[3]));
}

extern "C" int t2amd_vc_ola_bwd_f32(const float* d_audio, long long T, long long a_floats, const float* wsq, const int* utt, int B,
                                    const int* rowb0, const int* rowr0, long long n_rowb, long long P, int L, int hop, int trim,
                                    float* d_frames, long long ldf, long long f_floats, void* stream) {
    T2_REQUIRE(d_audio && wsq && utt && rowb0 && rowr0 && d_frames, "vc_ola_bwd: null operand");
    T2_REQUIRE(P > 0 && P <= T2_MAX_ROWS && n_rowb >= P && B >= 1 && B <= 65535,
               "vc_ola_bwd: 1 to 65535 utterances, a row map that covers at most 2^31 - 256 rows");
    T2_REQUIRE(L >= 4 && L % 4 == 0 && L <= 16384 && hop >= 1 && hop <= L && L % hop == 0,
               "vc_ola_bwd: the frame length must be a multiple of 4 (at most 16384) and of hop");
    T2_REQUIRE(trim >= 0 && 2 * trim >= L - hop && 2 * trim <= L, "vc_ola_bwd: trim must be (L - hop) / 2 to L / 2");
    T2_REQUIRE(T >= 1 && T <= T2_MAX_ROWS * 256 && a_floats >= (long long)B * T, "vc_ola_bwd: d_audio is shorter than (B, T)");
    T2_REQUIRE(ldf >= L && ldf % 4 == 0 && t2_aligned16(d_frames) && f_floats >= (P - 1) * ldf + L,
               "vc_ola_bwd: d_frames must hold 16-byte aligned rows of L floats");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(d_audio) & 3u) == 0, "vc_ola_bwd: d_audio misaligned");
    T2_LAUNCH(vc_ola_bwd_kernel, dim3(t2_cdiv(P * (L / 4), 256)), dim3(256), 0, (hipStream_t)stream, d_audio, T, wsq, utt, rowb0,
              rowr0, P, L, hop, trim, d_frames, ldf);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- polar -----------------------------------------------------------------------------------------------------------
// d_y[p] = [d_m (F) | d_p (F) | 0 ...] from Y[p] = [m | p] and d_S[p] = interleaved (d_re, d_im).  Thread k of a row writes
// bin k's two values and padding column 2 F + k.
__global__ __launch_bounds__(256) void vc_polar_bwd_kernel(const float* Y, long long ldy, const float* dS, long long lds,
                                                           long long P, int F, float clamp, const int* rowb0, float* dY,
                                                           long long lddy, int N, int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P * W) return;
    const long long p = i / W;
    const int k = (int)(i - p * W);
    if (k < F) {
        float dm = 0.f, dp = 0.f;
        if (rowb0[p] >= 0) {
            const float e = expf(Y[p * ldy + k]);
            const float mag = fminf(e, clamp);
            float sn, cs;
            sincosf(Y[p * ldy + F + k], &sn, &cs);
            const float dre = dS[p * lds + 2 * k], dim = dS[p * lds + 2 * k + 1];
            dm = e <= clamp ? mag * (cs * dre + sn * dim) : 0.f;
            dp = mag * (cs * dim - sn * dre);
        }
        dY[p * lddy + k] = dm;
        dY[p * lddy + F + k] = dp;
    }
    if (2 * F + k < N) dY[p * lddy + 2 * F + k] = 0.f;
}

extern "C" int t2amd_vc_polar_bwd_f32(const float* Y, long long y_floats, long long ldy, long long P, int F, float clamp,
                                      const float* dS, long long ds_floats, long long lds, const int* rowb0, long long n_rowb,
                                      float* dY, long long lddy, long long dy_floats, int N, void* stream) {
    T2_REQUIRE(Y && dS && rowb0 && dY, "vc_polar_bwd: null operand");
    T2_REQUIRE(P > 0 && P <= T2_MAX_ROWS && n_rowb >= P, "vc_polar_bwd: the row map does not cover the rows (at most 2^31 - 256)");
    T2_REQUIRE(F >= 1 && F <= 8193 && clamp > 0.f, "vc_polar_bwd: 1 to 8193 bins, a positive clamp");
    T2_REQUIRE(ldy >= 2 * F && y_floats >= (P - 1) * ldy + 2 * F, "vc_polar_bwd: Y is shorter than its rows of 2 F values");
    T2_REQUIRE(lds >= 2 * F && ds_floats >= (P - 1) * lds + 2 * F, "vc_polar_bwd: d_S is shorter than its rows of 2 F values");
    T2_REQUIRE(N >= 2 * F && N <= 32768 && lddy >= N && dy_floats >= (P - 1) * lddy + N,
               "vc_polar_bwd: d_Y is shorter than its rows of N >= 2 F values");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(Y) & 3u) == 0 && (reinterpret_cast<uintptr_t>(dS) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(dY) & 3u) == 0 && dY != Y && dY != dS,
               "vc_polar_bwd: operands misaligned or d_Y is one of the inputs");
    const int W = F > N - 2 * F ? F : N - 2 * F;
    T2_LAUNCH(vc_polar_bwd_kernel, dim3(t2_cdiv(P * W, 256)), dim3(256), 0, (hipStream_t)stream, Y, ldy, dS, lds, P, F, clamp,
              rowb0, dY, lddy, N, W);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- GELU ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vcb_gelu_grad(float u) {
    const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * u * u);
    return cdf + u * pdf;
}

__global__ __launch_bounds__(256) void vc_gelu_bwd_kernel(const float* U, long long ldu, long long P, int I, const int* rowb0,
                                                          float* dH, long long ldh) {
    const int nq = I >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P * nq) return;
    const long long p = i / nq;
    const int c = 4 * (int)(i - p * nq);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rowb0[p] >= 0) {
        const float4 u = t2_ld4(U + p * ldu + c), d = t2_ld4(dH + p * ldh + c);
        o.x = d.x * vcb_gelu_grad(u.x);
        o.y = d.y * vcb_gelu_grad(u.y);
        o.z = d.z * vcb_gelu_grad(u.z);
        o.w = d.w * vcb_gelu_grad(u.w);
    }
    t2_st4(dH + p * ldh + c, o);
}

extern "C" int t2amd_vc_gelu_bwd_f32(const float* U, long long u_floats, long long ldu, long long P, int I, const int* rowb0,
                                     long long n_rowb, float* dH, long long ldh, long long dh_floats, void* stream) {
    T2_REQUIRE(U && rowb0 && dH, "vc_gelu_bwd: null operand");
    T2_REQUIRE(P > 0 && P <= T2_MAX_ROWS && n_rowb >= P, "vc_gelu_bwd: the row map does not cover the rows (at most 2^31 - 256)");
    T2_REQUIRE(I >= 32 && I % 32 == 0 && I <= 16416, "vc_gelu_bwd: the width must be a multiple of 32, at most 16416");
    T2_REQUIRE(ldu >= I && ldu % 4 == 0 && ldh >= I && ldh % 4 == 0 && t2_aligned16(U) && t2_aligned16(dH) && U != dH,
               "vc_gelu_bwd: rows must hold I floats at a multiple of 4, 16-byte aligned, in two buffers");
    T2_REQUIRE(u_floats >= (P - 1) * ldu + I, "vc_gelu_bwd: U is shorter than its rows");
    T2_REQUIRE(dh_floats >= (P - 1) * ldh + I, "vc_gelu_bwd: d_H is shorter than its rows");
    T2_LAUNCH(vc_gelu_bwd_kernel, dim3(t2_cdiv(P * (I / 4), 256)), dim3(256), 0, (hipStream_t)stream, U, ldu, P, I, rowb0, dH, ldh);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- gamma -----------------------------------------------------------------------------------------------------------
// partial[slot][D]: slot = the wave's VCB_WAVE_ROWS rows.  Y2 leaves as d_y2 = gamma d_x.
__global__ __launch_bounds__(64 * VCB_WAVES) void vc_gamma_bwd_kernel(const float* dX, long long lddx, float* Y2, long long ldy,
                                                                      long long P, int D, const float* gamma, const int* rowb0,
                                                                      float* partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long slot = (long long)blockIdx.x * VCB_WAVES + wave, p0 = slot * VCB_WAVE_ROWS;
    if (p0 >= P) return;
    const int nq = D >> 2;
    for (int q = lane; q < nq; q += 64) {
        const float4 g = t2_ld4(gamma + 4 * q);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < VCB_WAVE_ROWS; ++j) {
            const long long p = p0 + j;
            if (p >= P) break;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rowb0[p] >= 0) {
                const float4 d = t2_ld4(dX + p * lddx + 4 * q), y = t2_ld4(Y2 + p * ldy + 4 * q);
                acc.x = fmaf(d.x, y.x, acc.x);
                acc.y = fmaf(d.y, y.y, acc.y);
                acc.z = fmaf(d.z, y.z, acc.z);
                acc.w = fmaf(d.w, y.w, acc.w);
                o = make_float4(g.x * d.x, g.y * d.y, g.z * d.z, g.w * d.w);
            }
            t2_st4(Y2 + p * ldy + 4 * q, o);
        }
        t2_st4(partial + slot * D + 4 * q, acc);
    }
}

#define VCB_ROWS_CHECK(who)                                                                                                   \
    T2_REQUIRE(P > 0 && P <= T2_MAX_ROWS && n_rowb >= P, who ": the row map does not cover the rows (at most 2^31 - 256)");   \
    T2_REQUIRE(D >= 32 && D % 32 == 0 && D <= VCB_MAX_D, who ": channels must be a multiple of 32, at most 512")

static inline long long vcb_slots(long long P) { return (P + VCB_WAVE_ROWS - 1) / VCB_WAVE_ROWS; }

extern "C" int t2amd_vc_gamma_bwd_f32(const float* dX, long long dx_floats, long long lddx, long long P, int D, const float* gamma,
                                      const int* rowb0, long long n_rowb, float* Y2, long long ldy, long long y_floats,
                                      float* partial, long long partial_floats, void* stream) {
    T2_REQUIRE(dX && gamma && rowb0 && Y2 && partial, "vc_gamma_bwd: null operand");
    VCB_ROWS_CHECK("vc_gamma_bwd");
    T2_REQUIRE(lddx >= D && lddx % 4 == 0 && ldy >= D && ldy % 4 == 0, "vc_gamma_bwd: rows must hold D floats at a multiple of 4");
    T2_REQUIRE(t2_aligned16(dX) && t2_aligned16(Y2) && t2_aligned16(gamma) && t2_aligned16(partial) && dX != Y2,
               "vc_gamma_bwd: operands must be 16-byte aligned, d_X and Y2 two buffers");
    T2_REQUIRE(dx_floats >= (P - 1) * lddx + D, "vc_gamma_bwd: d_X is shorter than its rows");
    T2_REQUIRE(y_floats >= (P - 1) * ldy + D, "vc_gamma_bwd: Y2 is shorter than its rows");
    T2_REQUIRE(partial_floats >= vcb_slots(P) * D, "vc_gamma_bwd: partial is shorter than [ceil(P / 16)][D]");
    T2_LAUNCH(vc_gamma_bwd_kernel, dim3(t2_cdiv(vcb_slots(P), VCB_WAVES)), dim3(64 * VCB_WAVES), 0, (hipStream_t)stream, dX, lddx,
              Y2, ldy, P, D, gamma, rowb0, partial);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- LayerNorm (after an optional depthwise convolution) -------------------------------------------------------------
// y = conv_bias + depthwise(X) (taps = 0: y = X), xh = (y - mean) rstd, the forward's out = xh lw + lb.  With g = d_out:
//   d_z = rstd (lw g - mean_c(lw g) - xh mean_c(lw g xh)),  partial[slot] = [sum_r g xh (D) | sum_r g (D)].
// d_z may be d_out: a lane reads its own elements of a row before it writes them.
__global__ __launch_bounds__(64 * VCB_WAVES) void vc_ln_bwd_kernel(const float* X, long long ldx, long long P, int D,
                                                                   const float* w, const float* cb, int taps, const float* lw,
                                                                   float eps, const int* rowb0, const float* G, long long ldg,
                                                                   float* dZ, long long lddz, float* partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long slot = (long long)blockIdx.x * VCB_WAVES + wave, p0 = slot * VCB_WAVE_ROWS;
    const int nq = D >> 2, half = (taps - 1) / 2;                // every wave of the workgroup takes every butterfly
    float4 aw[VCB_MAX_D / 256], ab[VCB_MAX_D / 256];
#pragma unroll
    for (int i = 0; i < VCB_MAX_D / 256; ++i) aw[i] = ab[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < VCB_WAVE_ROWS; ++j) {
        const long long p = p0 + j;
        const bool inside = p < P;
        const bool real = inside && rowb0[p] >= 0;
        float4 v[VCB_MAX_D / 256], wd[VCB_MAX_D / 256];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < VCB_MAX_D / 256; ++i) {              // vc_dwln_kernel's arithmetic, operation for operation
            const int q = lane + 64 * i;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (real && q < nq) {
                if (taps == 0) {
                    a = t2_ld4(X + p * ldx + 4 * q);
                } else {
                    a = t2_ld4(cb + 4 * q);
                    for (int t = 0; t < taps; ++t) {
                        const long long src = p + t - half;
                        if (src < 0 || src >= P) continue;
                        const float4 x = t2_ld4(X + src * ldx + 4 * q);
                        const float4 k = t2_ld4(w + (long long)t * D + 4 * q);
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
        for (int i = 0; i < VCB_MAX_D / 256; ++i) {
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
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < VCB_MAX_D / 256; ++i) {
            const int q = lane + 64 * i;
            wd[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (real && q < nq) {
                const float4 g = t2_ld4(G + p * ldg + 4 * q), k = t2_ld4(lw + 4 * q);
                v[i] = make_float4(v[i].x * rstd, v[i].y * rstd, v[i].z * rstd, v[i].w * rstd);
                wd[i] = make_float4(g.x * k.x, g.y * k.y, g.z * k.z, g.w * k.w);
                s1 += (wd[i].x + wd[i].y) + (wd[i].z + wd[i].w);
                s2 += (wd[i].x * v[i].x + wd[i].y * v[i].y) + (wd[i].z * v[i].z + wd[i].w * v[i].w);
                aw[i].x = fmaf(g.x, v[i].x, aw[i].x);
                aw[i].y = fmaf(g.y, v[i].y, aw[i].y);
                aw[i].z = fmaf(g.z, v[i].z, aw[i].z);
                aw[i].w = fmaf(g.w, v[i].w, aw[i].w);
                ab[i].x += g.x;
                ab[i].y += g.y;
                ab[i].z += g.z;
                ab[i].w += g.w;
            }
        }
        const float m1 = t2_wave_sum(s1) / (float)D, m2 = t2_wave_sum(s2) / (float)D;
#pragma unroll
        for (int i = 0; i < VCB_MAX_D / 256; ++i) {
            const int q = lane + 64 * i;
            if (q >= nq || !inside) continue;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (real) {
                o.x = rstd * (wd[i].x - m1 - v[i].x * m2);
                o.y = rstd * (wd[i].y - m1 - v[i].y * m2);
                o.z = rstd * (wd[i].z - m1 - v[i].z * m2);
                o.w = rstd * (wd[i].w - m1 - v[i].w * m2);
            }
            t2_st4(dZ + p * lddz + 4 * q, o);
        }
    }
#pragma unroll
    for (int i = 0; i < VCB_MAX_D / 256; ++i) {
        const int q = lane + 64 * i;
        if (q >= nq || p0 >= P) continue;
        t2_st4(partial + slot * 2 * D + 4 * q, aw[i]);
        t2_st4(partial + slot * 2 * D + D + 4 * q, ab[i]);
    }
}

extern "C" int t2amd_vc_ln_bwd_f32(const float* X, long long x_floats, long long ldx, long long P, int D, const float* w,
                                   long long w_floats, const float* conv_bias, int taps, const float* ln_w, float eps,
                                   const int* rowb0, long long n_rowb, const float* G, long long ldg, long long g_floats, float* dZ,
                                   long long lddz, long long dz_floats, float* partial, long long partial_floats, void* stream) {
    T2_REQUIRE(X && ln_w && rowb0 && G && dZ && partial, "vc_ln_bwd: null operand");
    VCB_ROWS_CHECK("vc_ln_bwd");
    T2_REQUIRE(taps == 0 || (taps % 2 == 1 && taps <= VCB_MAX_TAPS), "vc_ln_bwd: taps must be 0 (LayerNorm alone) or odd, at most 7");
    T2_REQUIRE(taps == 0 || (w && conv_bias && w_floats >= (long long)taps * D), "vc_ln_bwd: w is shorter than [taps][D]");
    T2_REQUIRE(eps > 0.f, "vc_ln_bwd: eps must be positive");
    T2_REQUIRE(ldx >= D && ldx % 4 == 0 && ldg >= D && ldg % 4 == 0 && lddz >= D && lddz % 4 == 0,
               "vc_ln_bwd: rows must hold D floats at a multiple of 4");
    T2_REQUIRE(t2_aligned16(X) && t2_aligned16(G) && t2_aligned16(dZ) && t2_aligned16(ln_w) && t2_aligned16(partial) &&
                   (taps == 0 || (t2_aligned16(w) && t2_aligned16(conv_bias))),
               "vc_ln_bwd: operands must be 16-byte aligned");
    T2_REQUIRE(x_floats >= (P - 1) * ldx + D, "vc_ln_bwd: X is shorter than its rows");
    T2_REQUIRE(g_floats >= (P - 1) * ldg + D, "vc_ln_bwd: d_out is shorter than its rows");
    T2_REQUIRE(dz_floats >= (P - 1) * lddz + D, "vc_ln_bwd: d_Z is shorter than its rows");
    T2_REQUIRE(X != dZ, "vc_ln_bwd: d_Z must not be X (a row's window reads its neighbours)");
    T2_REQUIRE(partial_floats >= vcb_slots(P) * 2 * D, "vc_ln_bwd: partial is shorter than [ceil(P / 16)][2 D]");
    T2_LAUNCH(vc_ln_bwd_kernel, dim3(t2_cdiv(vcb_slots(P), VCB_WAVES)), dim3(64 * VCB_WAVES), 0, (hipStream_t)stream, X, ldx, P, D,
              w, conv_bias, taps, ln_w, eps, rowb0, G, ldg, dZ, lddz, partial);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- depthwise convolution -------------------------------------------------------------------------------------------
// The forward is z[r][c] = bias[c] + sum_t X[r + t - half][c] w[t][c].  Over the finished d_z image (zero on halo rows):
//   d_x[r][c] = res[r][c] + sum_t w[t][c] d_z[r + half - t][c]       (res: the residual branch's gradient, may be d_x)
//   partial[slot] = [sum_r d_z[r][c] X[r + t - half][c] (taps x D) | sum_r d_z[r][c] (D)]
__global__ __launch_bounds__(64 * VCB_WAVES) void vc_dw_bwd_kernel(const float* dZ, long long lddz, const float* X, long long ldx,
                                                                   long long P, int D, const float* w, int taps,
                                                                   const int* rowb0, const float* res, long long ldres, float* dX,
                                                                   long long lddx, float* partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long slot = (long long)blockIdx.x * VCB_WAVES + wave, p0 = slot * VCB_WAVE_ROWS;
    if (p0 >= P) return;
    const int nq = D >> 2, half = (taps - 1) / 2;
    float* part = partial + slot * (taps + 1) * D;
    for (int q = lane; q < nq; q += 64) {
        float4 acc[VCB_MAX_TAPS + 1];
#pragma unroll
        for (int t = 0; t <= VCB_MAX_TAPS; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < VCB_WAVE_ROWS; ++j) {
            const long long p = p0 + j;
            if (p >= P) break;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rowb0[p] >= 0) {
                if (res) o = t2_ld4(res + p * ldres + 4 * q);
                const float4 z = t2_ld4(dZ + p * lddz + 4 * q);
#pragma unroll
                for (int t = 0; t < VCB_MAX_TAPS; ++t) {
                    if (t >= taps) continue;
                    const long long sz = p + half - t, sx = p + t - half;
                    if (sz >= 0 && sz < P) {
                        const float4 zz = t2_ld4(dZ + sz * lddz + 4 * q), k = t2_ld4(w + (long long)t * D + 4 * q);
                        o.x = fmaf(k.x, zz.x, o.x);
                        o.y = fmaf(k.y, zz.y, o.y);
                        o.z = fmaf(k.z, zz.z, o.z);
                        o.w = fmaf(k.w, zz.w, o.w);
                    }
                    if (sx >= 0 && sx < P) {
                        const float4 x = t2_ld4(X + sx * ldx + 4 * q);
                        acc[t].x = fmaf(z.x, x.x, acc[t].x);
                        acc[t].y = fmaf(z.y, x.y, acc[t].y);
                        acc[t].z = fmaf(z.z, x.z, acc[t].z);
                        acc[t].w = fmaf(z.w, x.w, acc[t].w);
                    }
                }
                acc[VCB_MAX_TAPS].x += z.x;
                acc[VCB_MAX_TAPS].y += z.y;
                acc[VCB_MAX_TAPS].z += z.z;
                acc[VCB_MAX_TAPS].w += z.w;
            }
            t2_st4(dX + p * lddx + 4 * q, o);
        }
#pragma unroll
        for (int t = 0; t < VCB_MAX_TAPS; ++t)
            if (t < taps) t2_st4(part + (long long)t * D + 4 * q, acc[t]);
        t2_st4(part + (long long)taps * D + 4 * q, acc[VCB_MAX_TAPS]);
    }
}

extern "C" int t2amd_vc_dw_bwd_f32(const float* dZ, long long dz_floats, long long lddz, long long P, int D, const float* X,
                                   long long x_floats, long long ldx, const float* w, long long w_floats, int taps,
                                   const int* rowb0, long long n_rowb, const float* res, long long ldres, long long res_floats,
                                   float* dX, long long lddx, long long dx_floats, float* partial, long long partial_floats,
                                   void* stream) {
    T2_REQUIRE(dZ && X && w && rowb0 && dX && partial, "vc_dw_bwd: null operand");
    VCB_ROWS_CHECK("vc_dw_bwd");
    T2_REQUIRE(taps >= 1 && taps % 2 == 1 && taps <= VCB_MAX_TAPS && w_floats >= (long long)taps * D,
               "vc_dw_bwd: taps must be odd, at most 7, and w hold [taps][D]");
    T2_REQUIRE(lddz >= D && lddz % 4 == 0 && ldx >= D && ldx % 4 == 0 && lddx >= D && lddx % 4 == 0 &&
                   (!res || (ldres >= D && ldres % 4 == 0)),
               "vc_dw_bwd: rows must hold D floats at a multiple of 4");
    T2_REQUIRE(t2_aligned16(dZ) && t2_aligned16(X) && t2_aligned16(w) && t2_aligned16(dX) && t2_aligned16(partial) &&
                   (!res || t2_aligned16(res)),
               "vc_dw_bwd: operands must be 16-byte aligned");
    T2_REQUIRE(dz_floats >= (P - 1) * lddz + D, "vc_dw_bwd: d_Z is shorter than its rows");
    T2_REQUIRE(x_floats >= (P - 1) * ldx + D, "vc_dw_bwd: X is shorter than its rows");
    T2_REQUIRE(dx_floats >= (P - 1) * lddx + D, "vc_dw_bwd: d_X is shorter than its rows");
    T2_REQUIRE(!res || res_floats >= (P - 1) * ldres + D, "vc_dw_bwd: res is shorter than its rows");
    T2_REQUIRE(dX != dZ && dX != X, "vc_dw_bwd: d_X must not be d_Z or X (a row's window reads their neighbours)");
    T2_REQUIRE(partial_floats >= vcb_slots(P) * (taps + 1) * D, "vc_dw_bwd: partial is shorter than [ceil(P / 16)][taps + 1][D]");
    T2_LAUNCH(vc_dw_bwd_kernel, dim3(t2_cdiv(vcb_slots(P), VCB_WAVES)), dim3(64 * VCB_WAVES), 0, (hipStream_t)stream, dZ, lddz, X,
              ldx, P, D, w, taps, rowb0, res, ldres, dX, lddx, partial);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
