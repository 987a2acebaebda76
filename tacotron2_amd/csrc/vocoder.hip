// Griffin-Lim vocoder on the GPU: the inverse half of the reference's stft.py (STFT.inverse, stft.py:107-141) and the
// phase half of STFT.transform (stft.py:77-105), plus the element passes of the batched Griffin-Lim loop
// (audio_processing.py:59-76).  The two contractions of an iteration run on the dense GEMM of gemm.hip:
//   frames[r][0:L]  = rec[r][0:2Fp] . IB[L][2Fp]^T         (inverse DFT of every frame; IB = windowed pinv basis)
//   spec[r][0:2F]   = padded-as-[R][L] (lda = hop) . FB[2F][L]^T   (forward DFT, rows overlap as in the mel path)
// What is left here is HBM-bound element work, plain C++ (expf / sqrtf / atan2f), no builtins, so that the CPU test-suite
// can run these very kernels through tests/hip_emu.
//
// Packed frame space.  Utterance b with n_b frames owns rows [row0_b, row0_b + n_b + c - 1), c = ceil(L / hop): its
// reflect-padded signal ((n_b - 1) hop + L samples) starts at sample row0_b * hop of one packed buffer, so a single
// lda = hop view serves every utterance with no crossover; the c - 1 gap rows after each utterance are computed by the
// GEMMs and ignored.  The `plan` table (int32, device) describes the packing:
//   plan[0 .. B]          row0_b (plan[B] = R, the packed row count)
//   plan[B+1 .. 2B]       n_b
//   plan[2B+1 .. 2B+R]    utterance of every packed row
// Every entry point also takes the lengths on the host (`n_host`) so that it can check them without reading the device.
// Complex rows are interleaved: rec[r][2f] = real, rec[r][2f+1] = imaginary, columns 2F .. 2Fp zero; spec likewise
// (the forward basis rows are interleaved to match: every output column is its own dot product, the bits do not move).
#include "common.h"

struct alignas(8) t2_f2 { float x, y; };

static __host__ __device__ __forceinline__ long long t2_vreflect(long long i, long long T) {
    if (i < 0) i = -i;
    if (i >= T) i = 2 * (T - 1) - i;
    return i;
}

// Value of the reference's inverse_transform at untrimmed position u of utterance (row0, n): sum over the frames that cover
// u in ascending frame order, divided by the window sum-square where that is > tiny(float32), times L / hop.  The window
// sum-square is rebuilt here in the reference's arithmetic (window_sumsquare: a float32 envelope to which each frame's
// float64 squared window is added, rounded back to float32 after every frame).
static __host__ __device__ __forceinline__ float t2_ola_value(const float* __restrict__ frames, long long ldf,
                                                              const double* __restrict__ wsq, int row0, int n, long long u,
                                                              int L, int hop, float scale) {
    long long jhi = u / hop;
    if (jhi > n - 1) jhi = n - 1;
    const long long jlo = u >= L ? (u - L) / hop + 1 : 0;
    float acc = 0.0f, ws = 0.0f;
    for (long long j = jlo; j <= jhi; ++j) {
        const long long k = u - j * hop;
        acc = acc + frames[(row0 + j) * ldf + k];
        ws = (float)((double)ws + wsq[k]);
    }
    if (ws > 1.17549435e-38f) acc = acc / ws;
    return acc * scale;
}

// mode 0: out = the reflect-padded packed signal of the next forward transform (P samples, gaps and tail zero);
// mode 1: out[b][s] (row stride ldo, s < Tout) = the trimmed signal, zero for s >= T_b.
__global__ void __launch_bounds__(256) gl_overlap_add_kernel(const float* __restrict__ frames, long long ldf,
                                                             const double* __restrict__ wsq, const int* __restrict__ plan,
                                                             int B, int L, int hop, float scale, float* __restrict__ out,
                                                             long long ldo, long long total, int mode, long long Tout) {
    const int* row0 = plan;
    const int* nb = plan + B + 1;
    const int* row_utt = plan + 2 * B + 1;
    const long long R = row0[B];
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        float v = 0.0f;
        if (mode == 0) {
            const long long q = i / hop;
            if (q < R) {
                const int b = row_utt[q];
                const long long local = i - (long long)row0[b] * hop;
                const long long T = (long long)(nb[b] - 1) * hop;
                if (local < T + L) {
                    const long long u = t2_vreflect(local - L / 2, T) + L / 2;
                    v = t2_ola_value(frames, ldf, wsq, row0[b], nb[b], u, L, hop, scale);
                }
            }
            out[i] = v;
        } else {
            const long long b = i / Tout, s = i - b * Tout;
            const long long T = (long long)(nb[b] - 1) * hop;
            if (s < T) v = t2_ola_value(frames, ldf, wsq, row0[b], nb[b], s + L / 2, L, hop, scale);
            out[b * ldo + s] = v;
        }
    }
}

// rec[r] = S[r] * (re, im) / |z| for valid rows (the projection onto the target magnitude: what m cos(atan2(im, re)),
// m sin(atan2(im, re)) computes, without the angle); |z| = 0 gives (S, 0) like cos/sin(atan2(0, 0)).  Pad columns and gap
// rows are written as zeros.
__global__ void __launch_bounds__(256) gl_project_kernel(const float* __restrict__ spec, long long lds,
                                                         const float* __restrict__ S, long long ldS,
                                                         const int* __restrict__ plan, int B, int F, int Fp,
                                                         float* __restrict__ rec, long long ldr, long long total) {
    const int* row0 = plan;
    const int* nb = plan + B + 1;
    const int* row_utt = plan + 2 * B + 1;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long long r = i / Fp;
        const int f = (int)(i - r * Fp);
        const int b = row_utt[r];
        t2_f2 o = {0.0f, 0.0f};
        if (f < F && r - row0[b] < nb[b]) {
            const t2_f2 z = *reinterpret_cast<const t2_f2*>(spec + r * lds + 2 * f);
            const float m = S[r * ldS + f];
            const float a = sqrtf(t2_power(z.x, z.y));
            if (a > 0.0f) {
                o.x = m * (z.x / a);
                o.y = m * (z.y / a);
            } else {
                o.x = m;
            }
        }
        *reinterpret_cast<t2_f2*>(rec + r * ldr + 2 * f) = o;
    }
}

// (magnitude, phase) (B, F, ldn) -> rec = (m cos p, m sin p) in packed rows, and S[r][f] = m when `mag` is given (with
// mag == NULL the magnitudes are read from S, filled earlier).  phase == NULL: phase 0.
__global__ void __launch_bounds__(256) gl_rect_kernel(const float* __restrict__ mag, const float* __restrict__ phase,
                                                      long long ldn, const int* __restrict__ plan, int B, int F, int Fp,
                                                      float* __restrict__ S, long long ldS, float* __restrict__ rec,
                                                      long long ldr, long long total) {
    const int* row0 = plan;
    const int* nb = plan + B + 1;
    const int* row_utt = plan + 2 * B + 1;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long long r = i / Fp;
        const int f = (int)(i - r * Fp);
        const int b = row_utt[r];
        const long long j = r - row0[b];
        t2_f2 o = {0.0f, 0.0f};
        float m = 0.0f;
        const bool valid = f < F && j < nb[b];
        if (valid) {
            const long long src = ((long long)b * F + f) * ldn + j;
            m = mag ? mag[src] : S[r * ldS + f];
            const float p = phase ? phase[src] : 0.0f;
            o.x = m * cosf(p);
            o.y = m * sinf(p);
        }
        if (mag && f < F) S[r * ldS + f] = m;
        *reinterpret_cast<t2_f2*>(rec + r * ldr + 2 * f) = o;
    }
}

// spec rows (B*n, interleaved re/im) -> mag[b][f][j] = sqrt(re^2 + im^2) (products and sum rounded separately, like
// magnitude_kernel of audio.hip), phase[b][f][j] = atan2(im, re).  j is the fast index (coalesced stores).
__global__ void __launch_bounds__(256) gl_polar_kernel(const float* __restrict__ spec, long long lds, int n, int F,
                                                       float* __restrict__ mag, float* __restrict__ phase, long long total) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long long t = i / n;
        const long long j = i - t * n;
        const long long b = t / F;
        const long long f = t - b * F;
        const t2_f2 z = *reinterpret_cast<const t2_f2*>(spec + (b * n + j) * lds + 2 * f);
        if (mag) mag[i] = sqrtf(t2_power(z.x, z.y));
        if (phase) phase[i] = atan2f(z.y, z.x);
    }
}

// out[(b*n + j)*ld + m] = exp(mel[b][m][j]) for m < n_mel and j < lengths[b] (all j when lengths is NULL), else 0:
// the inverse of t2amd_mel_log_compress_f32 (dynamic_range_decompression + the transpose to frame-major rows).
__global__ void __launch_bounds__(256) mel_decompress_kernel(const float* __restrict__ mel, int n_mel, int n,
                                                             const int* __restrict__ lengths, float* __restrict__ out,
                                                             long long ld, long long total) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long long r = i / ld;
        const long long m = i - r * ld;
        const long long b = r / n, j = r - b * n;
        float v = 0.0f;
        if (m < n_mel && (!lengths || j < lengths[b])) v = expf(mel[(b * n_mel + m) * n + j]);
        out[i] = v;
    }
}

// 1-D grid over `total` items, grid-stride beyond 2^20 workgroups (no 65,535 limit anywhere)
static inline unsigned t2_grid1(long long total) {
    long long g = (total + 255) / 256;
    if (g > (1LL << 20)) g = 1LL << 20;
    return (unsigned)(g > 0 ? g : 1);
}

// host-side check of a packing: lengths present, each above the reflect limit, rows adding up to R
// (need_reflect: the packed signal is reflect-padded, which needs (n_b - 1) * hop > L / 2, torch's reflect rule)
static int t2_check_plan(const int* n_host, int B, int L, int hop, long long R, const char* who, bool need_reflect) {
    static thread_local char msg[256];
    if (!n_host) {
        snprintf(msg, sizeof msg, "%s: null lengths", who);
        T2_FAIL(msg);
    }
    const long long c = (L + hop - 1) / hop;
    long long rows = 0;
    for (int b = 0; b < B; ++b) {
        if (n_host[b] < 1 || (need_reflect && (long long)(n_host[b] - 1) * hop <= L / 2)) {
            snprintf(msg, sizeof msg, "%s: utterance %d has %d frames: (n - 1) * hop must exceed L / 2 = %d "
                     "(reflect padding needs a longer signal)", who, b, n_host[b], L / 2);
            T2_FAIL(msg);
        }
        rows += n_host[b] + c - 1;
    }
    if (rows != R) {
        snprintf(msg, sizeof msg, "%s: lengths pack into %lld rows, buffers hold %lld", who, rows, R);
        T2_FAIL(msg);
    }
    return T2AMD_OK;
}

static int t2_check_geometry(int B, int L, int hop, const char* who) {
    static thread_local char msg[160];
    if (!(B > 0 && L >= 2 && L % 2 == 0 && hop > 0 && hop <= L)) {
        snprintf(msg, sizeof msg, "%s: bad geometry (B %d, L %d, hop %d)", who, B, L, hop);
        T2_FAIL(msg);
    }
    return T2AMD_OK;
}

extern "C" long long t2amd_gl_packed_rows(const int* n_host, int B, int L, int hop) {
    if (!n_host || B <= 0 || hop <= 0 || L < hop) return -1;
    const long long c = (L + hop - 1) / hop;
    long long rows = 0;
    for (int b = 0; b < B; ++b) {
        if (n_host[b] < 1) return -1;
        rows += n_host[b] + c - 1;
    }
    return rows;
}

extern "C" int t2amd_gl_overlap_add_f32(const float* frames, long long ldf, const double* wsq, const int* plan,
                                        const int* n_host, int B, long long R, int L, int hop, float scale, float* out,
                                        long long ldo, long long out_len, int mode, void* stream) {
    T2_REQUIRE(frames && wsq && plan && out, "gl_overlap_add: null operand");
    T2_PROPAGATE(t2_check_geometry(B, L, hop, "gl_overlap_add"));
    T2_REQUIRE(R > 0 && ldf >= L, "gl_overlap_add: frame rows too short");
    T2_PROPAGATE(t2_check_plan(n_host, B, L, hop, R, "gl_overlap_add", mode == 0));
    T2_REQUIRE(mode == 0 || mode == 1, "gl_overlap_add: mode must be 0 (padded) or 1 (trimmed)");
    long long total;
    if (mode == 0) {
        T2_REQUIRE(out_len >= (R - 1) * hop + L, "gl_overlap_add: padded buffer shorter than (R - 1) * hop + L");
        total = out_len;
    } else {
        T2_REQUIRE(out_len > 0 && ldo >= out_len, "gl_overlap_add: output row too short");
        for (int b = 0; b < B; ++b)
            T2_REQUIRE((long long)(n_host[b] - 1) * hop <= out_len, "gl_overlap_add: an utterance is longer than the output row");
        total = (long long)B * out_len;
    }
    T2_LAUNCH(gl_overlap_add_kernel, dim3(t2_grid1(total)), dim3(256), 0, (hipStream_t)stream, frames, ldf, wsq, plan, B,
              L, hop, scale, out, ldo, total, mode, out_len);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_gl_project_f32(const float* spec, long long lds, const float* S, long long ldS, const int* plan,
                                    const int* n_host, int B, long long R, int L, int hop, int F, int Fp, float* rec,
                                    long long ldr, void* stream) {
    T2_REQUIRE(spec && S && plan && rec, "gl_project: null operand");
    T2_PROPAGATE(t2_check_geometry(B, L, hop, "gl_project"));
    T2_REQUIRE(R > 0 && F > 0 && Fp >= F, "gl_project: bad dims");
    T2_REQUIRE(lds >= 2LL * F && lds % 2 == 0 && ldS >= F && ldr >= 2LL * Fp && ldr % 2 == 0,
               "gl_project: row too short (or an odd complex row stride)");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(spec) & 7u) == 0 && (reinterpret_cast<uintptr_t>(rec) & 7u) == 0,
               "gl_project: complex rows must be 8-byte aligned");
    T2_PROPAGATE(t2_check_plan(n_host, B, L, hop, R, "gl_project", false));
    const long long total = R * Fp;
    T2_LAUNCH(gl_project_kernel, dim3(t2_grid1(total)), dim3(256), 0, (hipStream_t)stream, spec, lds, S, ldS, plan, B, F,
              Fp, rec, ldr, total);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_gl_rect_f32(const float* mag, const float* phase, long long ldn, const int* plan, const int* n_host,
                                 int B, long long R, int L, int hop, int F, int Fp, float* S, long long ldS, float* rec,
                                 long long ldr, void* stream) {
    T2_REQUIRE(S && plan && rec, "gl_rect: null operand");
    T2_PROPAGATE(t2_check_geometry(B, L, hop, "gl_rect"));
    T2_REQUIRE(R > 0 && F > 0 && Fp >= F, "gl_rect: bad dims");
    T2_REQUIRE(ldS >= F && ldr >= 2LL * Fp && ldr % 2 == 0, "gl_rect: row too short (or an odd complex row stride)");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(rec) & 7u) == 0, "gl_rect: complex rows must be 8-byte aligned");
    T2_PROPAGATE(t2_check_plan(n_host, B, L, hop, R, "gl_rect", false));
    if (mag || phase)
        for (int b = 0; b < B; ++b)
            T2_REQUIRE(n_host[b] <= ldn, "gl_rect: an utterance has more frames than the (B, F, n) input holds");
    const long long total = R * Fp;
    T2_LAUNCH(gl_rect_kernel, dim3(t2_grid1(total)), dim3(256), 0, (hipStream_t)stream, mag, phase, ldn, plan, B, F, Fp, S,
              ldS, rec, ldr, total);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_stft_polar_f32(const float* spec, long long lds, int B, int n, int F, float* mag, float* phase,
                                    void* stream) {
    T2_REQUIRE(spec && (mag || phase), "stft_polar: null operand");
    T2_REQUIRE(B > 0 && n > 0 && F > 0, "stft_polar: bad dims");
    T2_REQUIRE(lds >= 2LL * F && lds % 2 == 0, "stft_polar: row too short (or an odd complex row stride)");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(spec) & 7u) == 0, "stft_polar: complex rows must be 8-byte aligned");
    const long long total = (long long)B * F * n;
    T2_LAUNCH(gl_polar_kernel, dim3(t2_grid1(total)), dim3(256), 0, (hipStream_t)stream, spec, lds, n, F, mag, phase, total);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_mel_decompress_f32(const float* mel, int B, int n_mel, int n, const int* lengths, const int* n_host,
                                        float* out, long long ld, void* stream) {
    T2_REQUIRE(mel && out, "mel_decompress: null operand");
    T2_REQUIRE(B > 0 && n_mel > 0 && n > 0, "mel_decompress: bad dims");
    T2_REQUIRE(ld >= n_mel, "mel_decompress: row too short");
    if (lengths) {
        T2_REQUIRE(n_host, "mel_decompress: device lengths need their host copy");
        for (int b = 0; b < B; ++b)
            T2_REQUIRE(n_host[b] >= 0 && n_host[b] <= n, "mel_decompress: a length exceeds the frames of the input");
    }
    const long long total = (long long)B * n * ld;
    T2_LAUNCH(mel_decompress_kernel, dim3(t2_grid1(total)), dim3(256), 0, (hipStream_t)stream, mel, n_mel, n, lengths, out,
              ld, total);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
